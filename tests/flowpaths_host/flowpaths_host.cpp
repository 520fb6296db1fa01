// flowpaths_host -- TEST-ONLY host build of soilmachine_amd/csrc/soil_paths.h (the bodies of k_path_init, k_path_fold, k_path_up,
// k_path_lengths and k_path_stem) and of hill_jump_group of soil_hills.h, behind the drainage chain of
// tests/drainage_host/drainage_host.cpp, which this file includes.
//
// The same headers the kernels are made of, compiled by g++ (-ffp-contract=off) and run as tests/drainage_host runs them: the lanes of
// a workgroup one after the other, the workgroups of a launch one after the other, both first to last or last to first -- legal
// orders of the device's (the lanes of k_path_fold, which has barriers, always first to last). The maps, the lane groups and the tile
// variants are those of the drainage host build. tests/analysis_host_lib.py builds and binds this file; the product never loads it.
#include "../drainage_host/drainage_host.cpp"
#include "../../soilmachine_amd/csrc/soil_paths.h"

struct PathSetH { uint32_t *J, *S, *G; };
struct PathHostOut {   // what a run leaves: where the planes asked for ended up
  uint32_t *terminal, *straight, *diagonal, *upstream, *source, *stem;
  const uint64_t* drop;
};

// The call as the library queues it: the drainage chain with its statistics through the bare table, pending (AR: the first set's J),
// init, `rounds` jumps between the sets (4, 5, 6) and (7, 8, 9), then fold, up, lengths, the scan and stem on the set the last jump
// wrote; the other set's planes are FS, L and PA. up_order: the order of the up-walk's workgroups (bit 0) and lanes (bit 1), which
// may differ from the other launches'.
template <int TX, int TY, int SLOTS>
static void run_paths(const std::vector<LakeMember>& tab, uint32_t lanes, int descending, int lanes_descending, int up_order, uint32_t rounds,
                      std::vector<std::vector<uint32_t>>& plane, std::vector<uint64_t>& up, std::vector<PathAcc>& acc, uint32_t* nbasins, uint32_t* nprofile,
                      PathOut o, bool want_upstream, bool want_source, PathHostOut& res) {
  static PathTable<SLOTS> table;                     // (the "LDS")
  std::vector<LakeMember> bare(tab);
  for (LakeMember& m : bare) m.cap = 0u;
  Planes p;
  p.T.swap(plane[0]); p.B.swap(plane[1]); p.R.swap(plane[2]); p.P.swap(plane[3]); p.AR.swap(plane[4]);
  std::vector<BasinAcc> none(1);
  run_drainage<TX, TY, SLOTS>(bare, lanes, descending, lanes_descending, false, p, none, nbasins);
  auto each_lane = [&](int desc, int ldesc, auto&& body) {
    for (size_t k = 0; k < tab.size(); k++) {
      const uint32_t nb = (uint32_t)(((uint64_t)tab[k].dimx * tab[k].dimy + lanes - 1) / lanes);
      for (uint32_t b = 0; b < nb; b++)
        for (uint32_t l = 0; l < lanes; l++) {
          DrainHostLane one{lanes, nth(l, lanes, ldesc)};
          body(k, one, nth(b, nb, desc), nb);
        }
    }
  };
  each_lane(descending, lanes_descending, [&](size_t k, DrainHostLane& one, uint32_t b, uint32_t) { drain_pending_group(bare[k], one, b, p.R.data(), p.P.data(), p.AR.data()); });
  p.T.swap(plane[0]); p.B.swap(plane[1]); p.R.swap(plane[2]); p.P.swap(plane[3]); p.AR.swap(plane[4]);
  uint32_t* const T = plane[0].data(); uint32_t* const FH = plane[1].data(); uint32_t* const R = plane[2].data(); uint32_t* const P = plane[3].data();
  const PathSetH set[2] = {{plane[4].data(), plane[5].data(), plane[6].data()}, {plane[7].data(), plane[8].data(), plane[9].data()}};
  each_lane(descending, lanes_descending, [&](size_t k, DrainHostLane& one, uint32_t b, uint32_t nb) { path_init_group(tab[k], one, b, nb, R, set[0].J, set[0].S, set[0].G, FH, acc.data()); });
  for (uint32_t r = 0; r < rounds; r++) {
    const PathSetH &from = set[r & 1u], &to = set[(r + 1u) & 1u];
    each_lane(descending, lanes_descending, [&](size_t k, DrainHostLane& one, uint32_t b, uint32_t) { hill_jump_group(bare[k], one, b, from.J, from.S, from.G, to.J, to.S, to.G); });
  }
  const PathSetH last = set[rounds & 1u], spare = set[(rounds + 1u) & 1u];
  uint32_t* const FS = spare.J; uint32_t* const L = spare.S; uint32_t* const PA = spare.G;
  DrainHostGroup g{lanes};
  for (size_t k = 0; k < tab.size(); k++) {
    const LakeMember& m = tab[k];
    const uint32_t per = lake_stats_cells(SLOTS, lanes);
    const uint32_t nb = (uint32_t)(((uint64_t)m.dimx * m.dimy + per - 1) / per);
    for (uint32_t b = 0; b < nb; b++) path_fold_group<SLOTS>(m, g, nth(b, nb, descending), table, T, R, last.J, last.S, last.G, up.data(), FH, FS, acc.data());
  }
  each_lane(up_order & 1, (up_order >> 1) & 1, [&](size_t k, DrainHostLane& one, uint32_t b, uint32_t) { path_up_group(bare[k], one, b, R, P, up.data()); });
  each_lane(descending, lanes_descending, [&](size_t k, DrainHostLane& one, uint32_t b, uint32_t) { path_lengths_group(bare[k], one, b, T, last.S, last.G, FH, FS, L, nbasins + k); });
  uint32_t run = 0;
  for (size_t i = 0; i < plane[0].size(); i++) { PA[i] = run; run += L[i]; }
  if (want_upstream) o.upstream = R;
  if (want_source) o.source = P;
  each_lane(descending, lanes_descending, [&](size_t k, DrainHostLane& one, uint32_t b, uint32_t) {
    path_stem_group(tab[k], one, b, T, last.J, last.S, last.G, up.data(), FH, FS, PA, acc.data(), nbasins + k, nprofile + k, o);
  });
  res.terminal = last.J; res.straight = last.S; res.diagonal = last.G; res.upstream = R; res.source = P; res.stem = T; res.drop = up.data();
}

extern "C" {

// The flow paths of maps[0..nm) in one go, as smx_ensemble_flowpaths runs it (nm == 1: smx_flowpaths). out: nm * cap records of 64
// bytes, map i's from record i * cap; nbasins / nprofile: one count per map; the planes of all maps one after the other (NULL = skip);
// profile (nm == 1 only, else -2): the first min(profile_cap, nprofile) entries are written; rounds (NULL = skip): the rounds of
// hill_jump that ran. variant: a tile shape of dh_variant; lanes: 64, 128 or 256; order bit 0: every launch runs its workgroups last
// to first; bit 1: the lanes of a workgroup run last to first in the steps without a barrier; bits 2 and 3: the same for the up-walk
// alone, XORed onto bits 0 and 1. 0, or -2 for a bad argument.
int fh_flowpaths(dh_map* const* maps, uint32_t nm, int variant, uint32_t lanes, int launch_order, uint32_t cap, void* out, uint32_t* nbasins, uint32_t* terminal,
                 uint32_t* straight, uint32_t* diagonal, double* drop, uint32_t* upstream, uint32_t* source, uint32_t* stem, uint32_t* profile, uint32_t profile_cap,
                 uint32_t* nprofile, uint32_t* rounds_out) {
  if (nm == 0 || !nbasins || !nprofile || !lanes_ok(lanes) || (profile_cap && (!profile || nm != 1))) return -2;
  const Members pl = plan_members(maps, nm, cap, CAP_CELLS);
  const uint64_t words = pl.words;
  const uint32_t rounds = hill_rounds(pl.largest - 1u);
  if (rounds_out) *rounds_out = rounds;
  std::vector<std::vector<uint32_t>> plane(10);
  for (auto& v : plane) poison({&v}, words);
  std::vector<uint64_t> up(words, 0xABABABABABABABABull);
  std::vector<PathAcc> acc = poisoned_records<PathAcc>(pl.nrec);
  const uint32_t pcap = profile_cap < words ? profile_cap : (uint32_t)words;
  std::vector<uint32_t> prof(pcap ? pcap : 1, 0xDEADBEEFu);
  PathOut o;
  o.want_terminal = terminal ? 1u : 0u; o.want_stem = stem ? 1u : 0u; o.want_drop = drop ? 1u : 0u; o.profile_cap = pcap;
  o.upstream = nullptr; o.source = nullptr; o.profile = pcap ? prof.data() : nullptr;
  const int desc = launch_order & 1, ldesc = (launch_order >> 1) & 1, upo = (launch_order ^ (launch_order >> 2)) & 3;
  PathHostOut res{};
  if (!with_shape<TILE_SHAPES>(variant, [&](auto s) {
        using S = decltype(s);
        run_paths<S::TX, S::TY, S::SLOTS>(pl.tab, lanes, desc, ldesc, upo, rounds, plane, up, acc, nbasins, nprofile, o, upstream != nullptr, source != nullptr, res);
      })) return -2;
  cut_records<PathRec>(pl, nbasins, cap, out, sizeof(PathRec), [&](size_t j, PathRec& rec) { path_finish(acc[j], rec); });
  copy_plane(terminal, res.terminal, words);
  copy_plane(straight, res.straight, words);
  copy_plane(diagonal, res.diagonal, words);
  if (drop) memcpy(drop, res.drop, words * 8);   // (the up-walk's 64-bit words)
  copy_plane(upstream, res.upstream, words);
  copy_plane(source, res.source, words);
  copy_plane(stem, res.stem, words);
  if (pcap) memcpy(profile, prof.data(), (size_t)(pcap < nprofile[0] ? pcap : nprofile[0]) * 4);
  return 0;
}

}  // extern "C"
