// prox_host -- TEST-ONLY host build of soilmachine_amd/csrc/soil_prox.h (the bodies of k_prox_mark, k_prox_columns, k_prox_envelope,
// k_prox_query and k_prox_hist) behind the census's labelling of soil_lakes.h, which WATER mode runs first.
//
// The same headers the kernels are made of, compiled by g++ (-ffp-contract=off) and run as tests/drainage_host runs them: the lanes of
// a workgroup one after the other, the workgroups of a launch one after the other, both first to last or last to first -- legal
// orders of the device's (the lanes of k_prox_columns, k_prox_query and k_prox_hist, which have barriers, always first to last). The
// maps, the lane groups and the tile variants are those of the drainage host build, which this file includes for them.
// tests/proximity_host_lib.py builds and binds this file; the product never loads it.
#include "../drainage_host/drainage_host.cpp"
#include "../../soilmachine_amd/csrc/soil_prox.h"

// The call as the library queues it. LIST: the mark plane (0) filled and the list scattered into it for every member. WATER: the
// labelling through the bare table, the scan of the root marks into plane 1, the roots turned into ranks. Then the columns into
// plane 2, the envelopes of `bands` bands of columns into planes 3 and 4 with their depths in plane 1, the query into planes 5 (nearest), 6 (dist2) and 7 (group)
// where they are wanted, and with bins the histogram.
template <int TX, int TY, int SLOTS>
static void run_prox(const std::vector<LakeMember>& tab, uint32_t lanes, int descending, int lanes_descending, const uint32_t* list, uint32_t n,
                     std::vector<std::vector<uint32_t>>& plane, std::vector<ProxAcc>& acc, uint32_t* counts, uint32_t* hist, uint32_t nbins, uint32_t bin_width,
                     bool want_nearest, bool want_dist2, bool want_group, uint32_t bands) {
  static uint32_t lab[TX * TY];                      // (the "LDS")
  static ProxColumn column;
  static ProxTable<SLOTS> table;
  static ProxHistTable<SLOTS> htable;
  DrainHostGroup g{lanes};
  std::vector<LakeMember> bare(tab);
  for (LakeMember& m : bare) m.cap = 0u;
  uint32_t* const M = plane[0].data(); uint32_t* const BD = plane[1].data(); uint32_t* const P = plane[2].data();
  uint32_t* const S = plane[3].data(); uint32_t* const T = plane[4].data();
  if (list) {
    std::fill(plane[0].begin(), plane[0].end(), PROX_NONE);
  } else {
    for (const LakeMember& m : bare) {
      const uint32_t nt = lake_tiles(m, TX, TY);
      for (uint32_t b = 0; b < nt; b++) lake_tile_group<TX, TY>(m, g, nth(b, nt, descending), nt, lab, M, (LakeAcc*)nullptr);
    }
    for (const LakeMember& m : bare) {
      const uint32_t nt = lake_tiles(m, TX, TY);
      for (uint32_t b = 0; b < nt; b++) lake_merge_group<TX, TY>(m, g, nth(b, nt, descending), M);
    }
    for (const LakeMember& m : bare) {
      const uint32_t nb = (uint32_t)(((uint64_t)m.dimx * m.dimy + lanes - 1) / lanes);
      for (uint32_t b = 0; b < nb; b++) lake_flatten_group(m, g, nth(b, nb, descending), M);
    }
    uint32_t run = 0;
    for (size_t i = 0; i < plane[0].size(); i++) { BD[i] = run; run += lake_mark(M, i); }
  }
  // the bodies without a barrier: every lane by itself, in the order asked for
  auto each_lane = [&](auto&& blocks, auto&& body) {
    for (size_t k = 0; k < tab.size(); k++) {
      const uint32_t nb = blocks(tab[k]);
      for (uint32_t b = 0; b < nb; b++)
        for (uint32_t l = 0; l < lanes; l++) {
          DrainHostLane one{lanes, nth(l, lanes, lanes_descending)};
          body(k, one, nth(b, nb, descending), nb);
        }
    }
  };
  each_lane([&](const LakeMember& m) { return prox_mark_blocks(m, list != nullptr, n, lanes); },
            [&](size_t k, DrainHostLane& one, uint32_t b, uint32_t nb) { prox_mark_group(tab[k], one, b, nb, list, n, M, BD, acc.data(), counts + k); });
  for (const LakeMember& m : tab)
    for (uint32_t x = 0; x < (uint32_t)m.dimx; x++) prox_columns_group(m, g, nth(x, (uint32_t)m.dimx, descending), column, M, P);
  each_lane([&](const LakeMember& m) { return (uint32_t)(((uint64_t)m.dimy * prox_bands(m, bands) + lanes - 1) / lanes); },
            [&](size_t k, DrainHostLane& one, uint32_t b, uint32_t) { prox_envelope_group(tab[k], one, b, bands, P, S, T, BD); });
  for (const LakeMember& m : tab) {
    const uint32_t per = lake_stats_cells(SLOTS, lanes);
    const uint32_t nb = (uint32_t)(((uint64_t)m.dimx * m.dimy + per - 1) / per);
    uint32_t* const d2 = want_dist2 || nbins ? plane[6].data() : nullptr;
    uint32_t* const gr = want_group || nbins ? plane[7].data() : nullptr;
    for (uint32_t b = 0; b < nb; b++)
      prox_query_group<SLOTS>(m, g, nth(b, nb, descending), bands, table, M, P, S, T, BD, acc.data(), want_nearest ? plane[5].data() : nullptr, d2, gr);
    if (nbins && m.cap)
      for (uint32_t b = 0; b < nb; b++) prox_hist_group<SLOTS>(m, g, nth(b, nb, descending), htable, d2, gr, hist, nbins, bin_width);
  }
}

extern "C" {

uint32_t ph_bands() { return PROX_BANDS; }

// Proximity of maps[0..nm) in one go, as smx_ensemble_proximity runs it (nm == 1: smx_proximity). cells: the n listed cells, one
// list for every map (the caller has checked it: inside every map, no cell twice), or NULL with n == 0 for the wet cells; out:
// nm * cap records, map i's from record i * cap, the first struct_size bytes of each; nrecords: one count per map; hist (with
// nbins > 0): nm * cap * nbins words, poisoned by the caller where it wants to see what is written; the planes of all maps one
// after the other (NULL = skip). variant: a tile shape of dh_variant; lanes: 64, 128 or 256; order bit 0: every launch runs its
// workgroups last to first; bit 1: the lanes of a workgroup run last to first in the steps without a barrier; bands: the bands of
// columns the envelopes are built in (at least 1; the library's is PROX_BANDS, ph_bands()). 0, or -2 for a bad argument.
int ph_proximity(dh_map* const* maps, uint32_t nm, int variant, uint32_t lanes, int launch_order, const uint32_t* cells, uint32_t n, void* out, uint64_t struct_size,
                 uint32_t cap, uint32_t* nrecords, uint32_t* hist, uint32_t nbins, uint32_t bin_width, uint32_t* nearest, uint32_t* group, uint32_t* dist2, uint32_t bands) {
  if (nm == 0 || bands == 0 || !nrecords || !lanes_ok(lanes) || (cells == nullptr) != (n == 0) || (cells && cap < n) || (!out && cap) || nbins > PROX_MAX_BINS ||
      (nbins && (!hist || !bin_width)) || struct_size == 0)
    return -2;
  for (uint32_t i = 0; i < nm; i++)
    if ((uint32_t)maps[i]->dimx > PROX_MAX_SIDE || (uint32_t)maps[i]->dimy > PROX_MAX_SIDE) return -2;
  const Members pl = plan_members(maps, nm, cells ? n : cap, cells ? CAP_CELLS : CAP_BLOCKS);
  const uint64_t words = pl.words;
  std::vector<std::vector<uint32_t>> plane(8);
  for (auto& v : plane) poison({&v}, words);
  std::vector<ProxAcc> acc = poisoned_records<ProxAcc>(pl.nrec);
  std::vector<uint32_t> table((size_t)pl.nrec * nbins + 1u, 0u), counts(nm, 0xDEADBEEFu);
  const int desc = launch_order & 1, ldesc = (launch_order >> 1) & 1;
  if (!with_shape<TILE_SHAPES>(variant, [&](auto s) {
        using S = decltype(s);
        run_prox<S::TX, S::TY, S::SLOTS>(pl.tab, lanes, desc, ldesc, cells, n, plane, acc, counts.data(), table.data(), nbins, bin_width, nearest != nullptr, dist2 != nullptr,
                                         group != nullptr, bands);
      })) return -2;
  for (uint32_t i = 0; i < nm; i++) {
    nrecords[i] = cells ? n : counts[i];
    const uint32_t w = std::min({nrecords[i], pl.tab[i].cap, cap});
    if (nbins && w) memcpy(hist + (size_t)i * cap * nbins, table.data() + (size_t)pl.tab[i].rec0 * nbins, (size_t)w * nbins * 4);
  }
  cut_records<ProxRec>(pl, nrecords, cap, out, (size_t)struct_size, [&](size_t j, ProxRec& rec) { prox_finish(acc[j], rec); });
  copy_plane(nearest, (const uint32_t*)plane[5].data(), words);
  copy_plane(dist2, (const uint32_t*)plane[6].data(), words);
  copy_plane(group, (const uint32_t*)plane[7].data(), words);
  return 0;
}

}  // extern "C"
