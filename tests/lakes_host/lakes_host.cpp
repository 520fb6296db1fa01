// lakes_host -- TEST-ONLY host build of soilmachine_amd/csrc/soil_lakes.h (the bodies of k_lake_tiles, k_lake_merge, k_lake_flatten
// and k_lake_stats).
//
// The same header the kernels are made of, compiled by g++ (-ffp-contract=off) and run with the lanes of a workgroup looped one
// after the other and the workgroups of a launch one after the other (in ascending or descending order): one legal order of the
// device's. A map is the top records of a snapshot's columns; several maps share the two planes as the members of an ensemble do.
// tests/analysis_host_lib.py builds and binds this file; the product never loads it.
#include "../analysis_host/analysis_host.h"

using lh_map = ah_map;

struct LakeHostGroup {   // a workgroup whose lanes the caller runs one after the other
  uint32_t n;
  uint32_t lanes() const { return n; }
  uint32_t lo() const { return 0u; }
  uint32_t hi() const { return n; }
  void barrier() const {}
};

template <int TX, int TY, int SLOTS>
static void run_census(const std::vector<LakeMember>& tab, uint32_t lanes, int descending, std::vector<uint32_t>& A, std::vector<uint32_t>& B,
                       std::vector<LakeAcc>& acc, uint32_t* nlakes) {
  static uint32_t lab[TX * TY];          // (the "LDS")
  static LakeTable<SLOTS> table;
  LakeHostGroup g{lanes};
  for (const LakeMember& m : tab) {
    const uint32_t nt = lake_tiles(m, TX, TY);
    for (uint32_t b = 0; b < nt; b++) lake_tile_group<TX, TY>(m, g, nth(b, nt, descending), nt, lab, A.data(), acc.data());
  }
  for (const LakeMember& m : tab) {
    const uint32_t nt = lake_tiles(m, TX, TY);
    for (uint32_t b = 0; b < nt; b++) lake_merge_group<TX, TY>(m, g, nth(b, nt, descending), A.data());
  }
  for (const LakeMember& m : tab) {
    const uint32_t nb = (uint32_t)(((uint64_t)m.dimx * m.dimy + lanes - 1) / lanes);
    for (uint32_t b = 0; b < nb; b++) lake_flatten_group(m, g, nth(b, nb, descending), A.data());
  }
  uint32_t run = 0;
  for (size_t i = 0; i < A.size(); i++) { B[i] = run; run += lake_mark(A.data(), i); }
  for (size_t k = 0; k < tab.size(); k++) {
    const LakeMember& m = tab[k];
    const uint32_t per = lake_stats_cells(SLOTS, lanes);
    const uint32_t nb = (uint32_t)(((uint64_t)m.dimx * m.dimy + per - 1) / per);
    for (uint32_t b = 0; b < nb; b++) lake_stats_group<SLOTS>(m, g, nth(b, nb, descending), table, A.data(), B.data(), acc.data(), nlakes + k);
  }
}

extern "C" {

lh_map* lh_create(int dimx, int dimy, const uint32_t* count, const uint32_t* type, const double* size, const double* floor) {
  return ah_create(dimx, dimy, count, type, size, floor);
}
void lh_destroy(lh_map* m) { delete m; }

int lh_variants() { return (int)std::size(TILE_SHAPES); }
// (tile columns, tile rows, slots of the statistics table) of a variant
int lh_variant(int v, int* tx, int* ty, int* slots) {
  const Shape* s = shape_at(TILE_SHAPES, v);
  if (!s) return -2;
  *tx = s->tx; *ty = s->ty; *slots = s->slots;
  return 0;
}

// The census of maps[0..nm) in one go, as smx_ensemble_lakes runs it (nm == 1: smx_lakes). out: nm * cap records of 64 bytes, map i's
// from record i * cap; nlakes: one count per map; plane: the label plane of all maps, one after the other (NULL = skip).
// lanes: 64, 128 or 256; descending != 0: every launch runs its workgroups last to first. 0, or -2 for a bad argument.
int lh_census(lh_map* const* maps, uint32_t nm, int variant, uint32_t lanes, int descending, uint32_t cap, void* out, uint32_t* nlakes, uint32_t* plane) {
  if (nm == 0 || !lanes_ok(lanes)) return -2;
  const Members pl = plan_members(maps, nm, cap, CAP_BLOCKS);
  std::vector<uint32_t> A, B;
  poison({&A, &B}, pl.words);
  std::vector<LakeAcc> acc = poisoned_records<LakeAcc>(pl.nrec);
  if (!with_shape<TILE_SHAPES>(variant, [&](auto s) {
        using S = decltype(s);
        run_census<S::TX, S::TY, S::SLOTS>(pl.tab, lanes, descending, A, B, acc, nlakes);
      })) return -2;
  cut_records<LakeRec>(pl, nlakes, cap, out, sizeof(LakeRec), [&](size_t j, LakeRec& rec) { lake_finish(acc[j], rec); });
  copy_plane(plane, A.data(), pl.words);
  return 0;
}

}  // extern "C"
