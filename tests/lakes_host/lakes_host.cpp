// lakes_host -- TEST-ONLY host build of soilmachine_amd/csrc/soil_lakes.h (the bodies of k_lake_tiles, k_lake_merge, k_lake_flatten
// and k_lake_stats).
//
// The same header the kernels are made of, compiled by g++ (-ffp-contract=off) and run with the lanes of a workgroup looped one
// after the other and the workgroups of a launch one after the other (in ascending or descending order): one legal order of the
// device's. A map is the top records of a snapshot's columns; several maps share the two planes as the members of an ensemble do.
// tests/lakes_host_lib.py builds and binds this file; the product never loads it.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#define SMX_D inline
#define SMX_HOSTSIM 1
#include "../../soilmachine_amd/csrc/soil_core.h"
#include "../../soilmachine_amd/csrc/soil_lakes.h"

using namespace smx;

struct lh_map {
  int dimx, dimy;
  std::vector<Sec> cells;
};

struct LakeHostGroup {   // a workgroup whose lanes the caller runs one after the other
  uint32_t n;
  uint32_t lanes() const { return n; }
  uint32_t lo() const { return 0u; }
  uint32_t hi() const { return n; }
  void barrier() const {}
};

// block b of nb in launch order
static inline uint32_t nth(uint32_t b, uint32_t nb, int descending) { return descending ? nb - 1u - b : b; }

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

// columns bottom -> top in cell order (the snapshot layout): a map keeps each column's top record
lh_map* lh_create(int dimx, int dimy, const uint32_t* count, const uint32_t* type, const double* size, const double* floor) {
  lh_map* m = new lh_map();
  m->dimx = dimx; m->dimy = dimy;
  const size_t n = (size_t)dimx * dimy;
  m->cells.resize(n);
  size_t off = 0;
  for (size_t i = 0; i < n; i++) {
    Sec c; c.size = c.floor = c.sat = 0; c.type = EMPTY; c.prev = NIL;
    if (count[i]) { const size_t t = off + count[i] - 1; c.size = size[t]; c.floor = floor[t]; c.type = type[t]; }
    off += count[i];
    m->cells[i] = c;
  }
  return m;
}
void lh_destroy(lh_map* m) { delete m; }

int lh_variants() { return 4; }
// (tile columns, tile rows, slots of the statistics table) of a variant
int lh_variant(int v, int* tx, int* ty, int* slots) {
  static const int t[4][3] = {{16, 64, 512}, {8, 8, 256}, {5, 7, 320}, {32, 4, 1024}};
  if (v < 0 || v >= 4) return -2;
  *tx = t[v][0]; *ty = t[v][1]; *slots = t[v][2];
  return 0;
}

// The census of maps[0..nm) in one go, as smx_ensemble_lakes runs it (nm == 1: smx_lakes). out: nm * cap records of 64 bytes, map i's
// from record i * cap; nlakes: one count per map; plane: the label plane of all maps, one after the other (NULL = skip).
// lanes: 64, 128 or 256; descending != 0: every launch runs its workgroups last to first. 0, or -2 for a bad argument.
int lh_census(lh_map* const* maps, uint32_t nm, int variant, uint32_t lanes, int descending, uint32_t cap, void* out, uint32_t* nlakes, uint32_t* plane) {
  if (nm == 0 || !(lanes == 64 || lanes == 128 || lanes == 256)) return -2;
  std::vector<LakeMember> tab(nm);
  uint64_t words = 0, nrec = 0;
  for (uint32_t i = 0; i < nm; i++) {
    LakeMember& m = tab[i];
    m.cells = maps[i]->cells.data(); m.dimx = maps[i]->dimx; m.dimy = maps[i]->dimy; m.pad = 0;
    m.off = (uint32_t)words; m.rec0 = (uint32_t)nrec;
    const uint64_t most = (uint64_t)((m.dimx + 1) / 2) * (uint64_t)((m.dimy + 1) / 2);
    m.cap = (uint32_t)(cap < most ? cap : most);
    words += (uint64_t)m.dimx * m.dimy; nrec += m.cap;
  }
  std::vector<uint32_t> A(words, 0xDEADBEEFu), B(words, 0xDEADBEEFu);   // (as the device's planes: whatever the last call left)
  std::vector<LakeAcc> acc(nrec ? nrec : 1);
  memset(acc.data(), 0xAB, acc.size() * sizeof(LakeAcc));
  switch (variant) {
    case 0: run_census<16, 64, 512>(tab, lanes, descending, A, B, acc, nlakes); break;   // the kernels' own shape
    case 1: run_census<8, 8, 256>(tab, lanes, descending, A, B, acc, nlakes); break;
    case 2: run_census<5, 7, 320>(tab, lanes, descending, A, B, acc, nlakes); break;     // a tile no dimension is a multiple of
    case 3: run_census<32, 4, 1024>(tab, lanes, descending, A, B, acc, nlakes); break;
    default: return -2;
  }
  for (uint32_t i = 0; i < nm; i++) {
    const uint32_t w = nlakes[i] < tab[i].cap ? nlakes[i] : tab[i].cap;
    for (uint32_t r = 0; r < w; r++) {
      LakeRec rec;
      lake_finish(acc[tab[i].rec0 + r], rec);
      memcpy(static_cast<char*>(out) + ((size_t)i * cap + r) * sizeof(LakeRec), &rec, sizeof(rec));
    }
  }
  if (plane) memcpy(plane, A.data(), words * 4);
  return 0;
}

}  // extern "C"
