// catchments_host -- TEST-ONLY host build of soilmachine_amd/csrc/soil_catch.h (the bodies of k_catch_mark, k_catch_init,
// k_catch_fold and k_catch_hist, and catch_area) and of hill_jump_group of soil_hills.h, behind the drainage chain of
// tests/drainage_host/drainage_host.cpp, which this file includes.
//
// The same headers the kernels are made of, compiled by g++ (-ffp-contract=off) and run as tests/drainage_host runs them: the lanes of
// a workgroup one after the other, the workgroups of a launch one after the other, both first to last or last to first -- legal
// orders of the device's (the lanes of k_catch_fold and k_catch_hist, which have barriers, always first to last). The maps, the lane
// groups and the tile variants are those of the drainage host build. tests/catchments_host_lib.py builds and binds this file; the
// product never loads it.
#include "../drainage_host/drainage_host.cpp"
#include "../../soilmachine_amd/csrc/soil_catch.h"

struct CatchSetH { uint32_t *J, *S, *G; };
struct CatchHostOut {   // what a run leaves: where the planes ended up
  const uint32_t *gauge, *straight, *diagonal;
};

// The call as the library queues it: the mark plane (3) filled and the list scattered into it for every member, the drainage chain
// with its statistics through the bare table and without its area step, init, `rounds` jumps between the sets (4, 5, 6) and
// (7, 8, 9), the fold on the set the last jump wrote -- the gauge plane goes to the other set's J -- and, with bins, the histogram.
template <int TX, int TY, int SLOTS>
static void run_catch(const std::vector<LakeMember>& tab, uint32_t lanes, int descending, int lanes_descending, uint32_t rounds, const uint32_t* list, uint32_t n,
                      std::vector<std::vector<uint32_t>>& plane, std::vector<double>& drop, std::vector<CatchAcc>& acc, uint32_t* hist, uint32_t nbins, double bin_height,
                      bool want_gauge, bool want_drop, CatchHostOut& res) {
  static CatchTable<SLOTS> table;                    // (the "LDS")
  static CatchHistTable<SLOTS> htable;
  std::vector<LakeMember> bare(tab);
  for (LakeMember& m : bare) m.cap = 0u;
  uint32_t* const M = plane[3].data();
  std::fill(plane[3].begin(), plane[3].end(), CATCH_NONE);
  for (size_t k = 0; k < tab.size(); k++) {
    const uint32_t nb = (n + lanes - 1) / lanes;
    for (uint32_t b = 0; b < nb; b++)
      for (uint32_t l = 0; l < lanes; l++) {
        DrainHostLane one{lanes, nth(l, lanes, lanes_descending)};
        catch_mark_group(bare[k], one, nth(b, nb, descending), list, n, M);
      }
  }
  Planes p;
  p.T.swap(plane[0]); p.B.swap(plane[1]); p.R.swap(plane[2]);
  std::vector<BasinAcc> none(1);
  std::vector<uint32_t> nbasins(tab.size(), 0u);
  run_drainage<TX, TY, SLOTS>(bare, lanes, descending, lanes_descending, false, p, none, nbasins.data());
  p.T.swap(plane[0]); p.B.swap(plane[1]); p.R.swap(plane[2]);
  uint32_t* const T = plane[0].data(); uint32_t* const R = plane[2].data();
  const CatchSetH set[2] = {{plane[4].data(), plane[5].data(), plane[6].data()}, {plane[7].data(), plane[8].data(), plane[9].data()}};
  auto each_lane = [&](auto&& body) {
    for (size_t k = 0; k < tab.size(); k++) {
      const uint32_t nb = (uint32_t)(((uint64_t)tab[k].dimx * tab[k].dimy + lanes - 1) / lanes);
      for (uint32_t b = 0; b < nb; b++)
        for (uint32_t l = 0; l < lanes; l++) {
          DrainHostLane one{lanes, nth(l, lanes, lanes_descending)};
          body(k, one, nth(b, nb, descending), nb);
        }
    }
  };
  each_lane([&](size_t k, DrainHostLane& one, uint32_t b, uint32_t nb) { catch_init_group(tab[k], one, b, nb, R, M, set[0].J, set[0].S, set[0].G, acc.data()); });
  for (uint32_t r = 0; r < rounds; r++) {
    const CatchSetH &from = set[r & 1u], &to = set[(r + 1u) & 1u];
    each_lane([&](size_t k, DrainHostLane& one, uint32_t b, uint32_t) { hill_jump_group(bare[k], one, b, from.J, from.S, from.G, to.J, to.S, to.G); });
  }
  const CatchSetH last = set[rounds & 1u], spare = set[(rounds + 1u) & 1u];
  DrainHostGroup g{lanes};
  for (size_t k = 0; k < tab.size(); k++) {
    const LakeMember& m = tab[k];
    const uint32_t per = lake_stats_cells(SLOTS, lanes);
    const uint32_t nb = (uint32_t)(((uint64_t)m.dimx * m.dimy + per - 1) / per);
    for (uint32_t b = 0; b < nb; b++)
      catch_fold_group<SLOTS>(m, g, nth(b, nb, descending), table, T, R, M, last.J, last.S, last.G, acc.data(), want_gauge ? spare.J : nullptr, want_drop ? drop.data() : nullptr);
    if (nbins)
      for (uint32_t b = 0; b < nb; b++) catch_hist_group<SLOTS>(m, g, nth(b, nb, descending), htable, M, last.J, hist, nbins, bin_height);
  }
  res.gauge = spare.J; res.straight = last.S; res.diagonal = last.G;
}

extern "C" {

// The catchments of maps[0..nm) in one go, as smx_ensemble_catchments runs it (nm == 1: smx_catchments). cells: the n gauges, one
// list for every map (the caller has checked it: inside every map, no cell twice); out: nm * n records, map i's from record i * n,
// the first struct_size bytes of each; hist (with nbins > 0): nm * n * nbins words; the planes of all maps one after the other
// (NULL = skip); rounds (NULL = skip): the rounds of hill_jump that ran. variant: a tile shape of dh_variant; lanes: 64, 128 or 256;
// order bit 0: every launch runs its workgroups last to first; bit 1: the lanes of a workgroup run last to first in the steps without
// a barrier. 0, or -2 for a bad argument.
int ch_catchments(dh_map* const* maps, uint32_t nm, int variant, uint32_t lanes, int launch_order, const uint32_t* cells, uint32_t n, void* out, uint64_t struct_size,
                  uint32_t* hist, uint32_t nbins, double bin_height, uint32_t* gauge, uint32_t* straight, uint32_t* diagonal, double* drop, uint32_t* rounds_out) {
  if (nm == 0 || !cells || n == 0 || !out || !lanes_ok(lanes) || nbins > CATCH_MAX_BINS || (nbins && (!hist || !(bin_height > 0.0)))) return -2;
  const Members pl = plan_members(maps, nm, n, CAP_CELLS);
  for (const LakeMember& m : pl.tab)
    if (m.cap != n) return -2;
  const uint64_t words = pl.words;
  const uint32_t rounds = hill_rounds(pl.largest - 1u);
  if (rounds_out) *rounds_out = rounds;
  std::vector<std::vector<uint32_t>> plane(10);
  for (auto& v : plane) poison({&v}, words);
  std::vector<double> dr(words);
  memset(dr.data(), 0xAB, words * 8);
  std::vector<CatchAcc> acc = poisoned_records<CatchAcc>(pl.nrec);
  std::vector<uint32_t> table((size_t)pl.nrec * nbins + 1u, 0u);
  const int desc = launch_order & 1, ldesc = (launch_order >> 1) & 1;
  CatchHostOut res{};
  if (!with_shape<TILE_SHAPES>(variant, [&](auto s) {
        using S = decltype(s);
        run_catch<S::TX, S::TY, S::SLOTS>(pl.tab, lanes, desc, ldesc, rounds, cells, n, plane, dr, acc, table.data(), nbins, bin_height, gauge != nullptr, drop != nullptr, res);
      })) return -2;
  std::vector<CatchRec> recs(n);
  std::vector<uint32_t> work(2 * (size_t)n);
  for (uint32_t i = 0; i < nm; i++) {
    for (uint32_t r = 0; r < n; r++) catch_finish(acc[(size_t)pl.tab[i].rec0 + r], recs[r]);
    catch_area(recs.data(), n, work.data(), work.data() + n);
    for (uint32_t r = 0; r < n; r++) memcpy(static_cast<char*>(out) + ((size_t)i * n + r) * struct_size, &recs[r], std::min<size_t>(struct_size, sizeof(CatchRec)));
  }
  if (nbins) memcpy(hist, table.data(), (size_t)pl.nrec * nbins * 4);
  copy_plane(gauge, res.gauge, words);
  copy_plane(straight, res.straight, words);
  copy_plane(diagonal, res.diagonal, words);
  copy_plane(drop, (const double*)dr.data(), words);
  return 0;
}

}  // extern "C"
