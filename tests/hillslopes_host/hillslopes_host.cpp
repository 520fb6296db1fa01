// hillslopes_host -- TEST-ONLY host build of soilmachine_amd/csrc/soil_hills.h (the bodies of k_hill_init, k_hill_jump and
// k_hill_fold) behind the streams chain of tests/streams_host/streams_host.cpp, which this file includes.
//
// The same headers the kernels are made of, compiled by g++ (-ffp-contract=off) and run as tests/streams_host runs them: the lanes of
// a workgroup one after the other, the workgroups of a launch one after the other, both first to last or last to first -- legal
// orders of the device's (the lanes of k_hill_fold, which has barriers, always first to last). The maps, the lane groups and the tile
// variants are those of tests/drainage_host/drainage_host.cpp. tests/analysis_host_lib.py builds and binds this file; the product
// never loads it.
#include "../streams_host/streams_host.cpp"
#include "../../soilmachine_amd/csrc/soil_hills.h"

struct HillSetH { uint32_t *J, *S, *G; };

// The call as the library queues it: the streams chain through the bare table with the segments plane and no record, then init,
// `rounds` jumps between the sets (R, P, AR) and (T, O, H), fold on the set the last jump wrote; entry goes to RE's plane, hillslope to
// the other set's J.
template <int TX, int TY, int SLOTS>
static void run_hills(const std::vector<LakeMember>& tab, uint32_t lanes, int descending, int lanes_descending, uint32_t threshold, uint32_t rounds, StreamPlanes& p,
                      std::vector<double>& h64, std::vector<HillAcc>& acc, uint32_t* nsegments, bool want_entry, bool want_hill, bool want_hand, HillSetH& last,
                      uint32_t*& entry, uint32_t*& hill) {
  static HillTable<SLOTS> table;                     // (the "LDS")
  std::vector<LakeMember> bare(tab);
  for (LakeMember& m : bare) m.cap = 0u;
  std::vector<StreamRec> none(1);
  run_streams<TX, TY>(bare, lanes, descending, lanes_descending, threshold, true, p, none, nsegments);
  const HillSetH set[2] = {{p.R.data(), p.P.data(), p.AR.data()}, {p.T.data(), p.O.data(), p.H.data()}};
  auto each_lane = [&](auto&& body) {
    for (const LakeMember& m : tab) {
      const uint32_t nb = (uint32_t)(((uint64_t)m.dimx * m.dimy + lanes - 1) / lanes);
      for (uint32_t b = 0; b < nb; b++)
        for (uint32_t l = 0; l < lanes; l++) {
          DrainHostLane one{lanes, nth(l, lanes, lanes_descending)};
          body(m, one, nth(b, nb, descending), nb);
        }
    }
  };
  each_lane([&](const LakeMember& m, DrainHostLane& one, uint32_t b, uint32_t nb) { hill_init_group(m, one, b, nb, p.SG.data(), set[0].J, set[0].S, set[0].G, acc.data()); });
  for (uint32_t r = 0; r < rounds; r++) {
    const HillSetH &from = set[r & 1u], &to = set[(r + 1u) & 1u];
    each_lane([&](const LakeMember& m, DrainHostLane& one, uint32_t b, uint32_t) { hill_jump_group(m, one, b, from.J, from.S, from.G, to.J, to.S, to.G); });
  }
  last = set[rounds & 1u];
  entry = p.RE.data(); hill = set[(rounds + 1u) & 1u].J;
  DrainHostGroup g{lanes};
  for (size_t k = 0; k < tab.size(); k++) {
    const LakeMember& m = tab[k];
    const uint32_t per = lake_stats_cells(SLOTS, lanes);
    const uint32_t nb = (uint32_t)(((uint64_t)m.dimx * m.dimy + per - 1) / per);
    for (uint32_t b = 0; b < nb; b++)
      hill_fold_group<SLOTS>(m, g, nth(b, nb, descending), table, last.J, last.S, last.G, p.SG.data(), p.D.data(), p.B.data(), acc.data(), nsegments + k,
                             want_entry ? entry : nullptr, want_hill ? hill : nullptr, want_hand ? h64.data() : nullptr);
  }
}

extern "C" {

// The hillslopes of maps[0..nm) in one go, as smx_ensemble_hillslopes runs it (nm == 1: smx_hillslopes). out: nm * cap records of 64
// bytes, map i's from record i * cap; nsegments: one count per map; entry / hillslope / straight / diagonal / hand: the planes of all
// maps, one after the other (NULL = skip); rounds (NULL = skip): the rounds of hill_jump that ran. variant: a tile shape of dh_variant;
// lanes: 64, 128 or 256; order bit 0: every launch runs its workgroups last to first; bit 1: the lanes of a workgroup run last to
// first in the steps without a barrier. 0, or -2 for a bad argument.
int hh_hillslopes(dh_map* const* maps, uint32_t nm, int variant, uint32_t lanes, int launch_order, uint32_t threshold, uint32_t cap, void* out, uint32_t* nsegments,
                  uint32_t* entry, uint32_t* hillslope, uint32_t* straight, uint32_t* diagonal, double* hand, uint32_t* rounds_out) {
  if (nm == 0 || threshold == 0 || !lanes_ok(lanes)) return -2;
  const Members pl = plan_members(maps, nm, cap, CAP_CELLS);
  const uint64_t words = pl.words;
  const uint32_t rounds = hill_rounds(hill_bound(threshold, pl.largest));
  if (rounds_out) *rounds_out = rounds;
  StreamPlanes p;
  poison({&p.T, &p.R, &p.P, &p.AR, &p.D, &p.O, &p.H, &p.RE, &p.B, &p.SG}, words);
  std::vector<double> h64(words, -12345.0);
  std::vector<HillAcc> acc = poisoned_records<HillAcc>(pl.nrec);
  const int desc = launch_order & 1, ldesc = (launch_order >> 1) & 1;
  HillSetH last{nullptr, nullptr, nullptr};
  uint32_t *e = nullptr, *hl = nullptr;
  if (!with_shape<TILE_SHAPES>(variant, [&](auto s) {
        using S = decltype(s);
        run_hills<S::TX, S::TY, S::SLOTS>(pl.tab, lanes, desc, ldesc, threshold, rounds, p, h64, acc, nsegments, entry != nullptr, hillslope != nullptr, hand != nullptr,
                                          last, e, hl);
      })) return -2;
  cut_records<HillRec>(pl, nsegments, cap, out, sizeof(HillRec), [&](size_t j, HillRec& rec) { hill_finish(acc[j], rec); });
  copy_plane(entry, e, words);
  copy_plane(hillslope, hl, words);
  copy_plane(straight, last.S, words);
  copy_plane(diagonal, last.G, words);
  copy_plane(hand, h64.data(), words);
  return 0;
}

}  // extern "C"
