// strata_host -- TEST-ONLY host build of soilmachine_amd/csrc/soil_strata.h (the bodies of k_strata_totals, k_strata_thickness,
// k_core_count and k_core_scatter).
//
// The same header the kernels are made of, compiled by g++ (-ffp-contract=off) and run with the lanes of a workgroup looped one
// after the other and the workgroups of a launch one after the other: one legal order of the device's. A map is built from a
// snapshot's columns: the top section inline in the cell record, the buried ones in a pool whose order the caller may scramble, so
// that nothing leans on the import's layout. The drivers below are the library's in small: results land in scratch, the verdict is
// taken, and only then are the caller's outputs written. tests/strata_host_lib.py builds and binds this file; the product never loads it.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#define SMX_D inline
#define SMX_HOSTSIM 1
#include "../../soilmachine_amd/csrc/soil_core.h"
#include "../../soilmachine_amd/csrc/soil_strata.h"

using namespace smx;

struct sh_map {
  int dimx, dimy;
  std::vector<Sec> cells, pool;
};

struct StrataHostGroup {   // a workgroup whose lanes the caller runs one after the other
  uint32_t n;
  uint32_t lanes() const { return n; }
  uint32_t lo() const { return 0u; }
  uint32_t hi() const { return n; }
  void barrier() const {}
};

static StrataMap host_map(const sh_map* h) {
  StrataMap m;
  m.cells = h->cells.data(); m.pool = h->pool.data(); m.cap = h->pool.size(); m.ncells = h->cells.size(); m.rec0 = 0u; m.index = 0u;
  return m;
}
static bool shape_ok(uint32_t lanes, uint32_t nblocks) { return (lanes == 64u || lanes == 128u || lanes == 256u) && nblocks >= 1u; }

extern "C" {

int sh_rec_bytes() { return (int)sizeof(StrataRec); }

// columns bottom -> top in cell order (the snapshot layout). scramble != 0: the buried sections take pool indices in the order of a
// stride permutation instead of the import's; `slack` unused records are appended to the pool.
sh_map* sh_create(int dimx, int dimy, const uint32_t* count, const uint32_t* type, const double* size, const double* floor, const double* sat, int scramble,
                  uint32_t slack) {
  sh_map* m = new sh_map();
  m->dimx = dimx; m->dimy = dimy;
  const size_t n = (size_t)dimx * dimy;
  size_t buried = 0;
  for (size_t i = 0; i < n; i++) buried += count[i] ? count[i] - 1u : 0u;
  std::vector<uint32_t> where(buried);
  size_t stride = 1;
  if (scramble && buried > 2) { stride = buried / 2 + 1; auto gcd = [](size_t a, size_t b) { while (b) { const size_t t = a % b; a = b; b = t; } return a; }; while (gcd(stride, buried) != 1) stride++; }
  for (size_t j = 0; j < buried; j++) where[j] = (uint32_t)((j * stride + (scramble ? 3 : 0)) % (buried ? buried : 1));
  m->cells.resize(n);
  m->pool.resize(buried + slack);
  for (Sec& p : m->pool) { p.size = p.floor = p.sat = 0; p.type = EMPTY; p.prev = NIL; }
  size_t off = 0, j = 0;
  for (size_t i = 0; i < n; i++) {
    Sec c; c.size = c.floor = c.sat = 0; c.type = EMPTY; c.prev = NIL;
    uint32_t below = NIL;
    for (uint32_t k = 0; k < count[i]; k++, off++) {
      Sec s; s.size = size[off]; s.floor = floor[off]; s.sat = sat[off]; s.type = type[off]; s.prev = below;
      if (k + 1u == count[i]) c = s;
      else { below = where[j++]; m->pool[below] = s; }
    }
    m->cells[i] = c;
  }
  return m;
}
void sh_destroy(sh_map* m) { delete m; }
uint64_t sh_pool_size(const sh_map* m) { return m->pool.size(); }
// the `prev` word of a cell's top record (pool == 0) or of a pool record: read, and written where set != 0 (to corrupt a chain)
uint32_t sh_prev(sh_map* m, int pool, uint64_t at, int set, uint32_t value) {
  Sec& s = pool ? m->pool[at] : m->cells[at];
  const uint32_t old = s.prev;
  if (set) s.prev = value;
  return old;
}

// smx_ensemble_soil_totals over maps[0..nm) (nm == 1: smx_soil_totals): nm * ntypes records of 48 bytes, one count of other sections
// per map. start (NULL = zeros): the records the fold begins from, where the device's begin from zero -- a test forces a wrap
// through it. 0; -5 with info = {member, lowest bad cell} and nothing written; -2 for a bad argument.
int sh_totals(sh_map* const* maps, uint32_t nm, uint32_t lanes, uint32_t nblocks, uint32_t ntypes, void* out, uint64_t* other, const void* start, uint64_t* info) {
  if (nm == 0 || !shape_ok(lanes, nblocks) || ntypes < 1u || ntypes > (uint32_t)STRATA_MAX_TYPES) return -2;
  std::vector<StrataRec> acc((size_t)nm * ntypes);
  if (start) memcpy(acc.data(), start, acc.size() * sizeof(StrataRec)); else memset(acc.data(), 0, acc.size() * sizeof(StrataRec));
  std::vector<uint64_t> oth(nm, 0ull), bad(nm, 0ull);
  static StrataTable table;   // (the "LDS")
  StrataHostGroup g{lanes};
  for (uint32_t i = 0; i < nm; i++) {
    StrataMap m = host_map(maps[i]);
    m.rec0 = i * ntypes; m.index = i;
    for (uint32_t b = 0; b < nblocks; b++) {
      if ((uint64_t)b * lanes >= m.ncells) continue;
      memset(&table, 0xAB, sizeof(table));   // (whatever the last workgroup left)
      strata_totals_group(m, g, b, nblocks, ntypes, table, acc.data(), oth.data(), bad.data());
    }
  }
  for (uint32_t i = 0; i < nm; i++)
    if (bad[i]) { info[0] = i; info[1] = strata_bad_cell(bad[i]); return -5; }
  memcpy(out, acc.data(), acc.size() * sizeof(StrataRec));
  if (other) memcpy(other, oth.data(), nm * 8);
  return 0;
}

// smx_soil_thickness: each output may be NULL. 0; -5 with *bad_cell and nothing written; -2.
int sh_thickness(sh_map* h, uint32_t lanes, uint32_t nblocks, const uint32_t* types, int32_t ntypes, double* thickness, double* cover, uint32_t* sections,
                 uint64_t* bad_cell) {
  if (!shape_ok(lanes, nblocks) || ntypes < 1 || ntypes > STRATA_MAX_LIST) return -2;
  StrataTypes ty{};
  ty.n = (uint32_t)ntypes;
  for (int32_t a = 0; a < ntypes; a++) {
    ty.t[a] = types[a];
    for (int32_t b = 0; b < a; b++) if (types[a] == types[b]) return -2;
  }
  const StrataMap m = host_map(h);
  const size_t vals = (size_t)ntypes * m.ncells;
  std::vector<double> th(thickness ? vals : 0, 777.0), cv(cover ? vals : 0, 777.0);
  std::vector<uint32_t> ns(sections ? vals : 0, 777u);
  uint64_t bad = 0ull;
  StrataHostGroup g{lanes};
  for (uint32_t b = 0; b < nblocks; b++)
    strata_thickness_group(m, g, b, nblocks, ty, thickness ? th.data() : nullptr, cover ? cv.data() : nullptr, sections ? ns.data() : nullptr, &bad);
  if (bad) { *bad_cell = strata_bad_cell(bad); return -5; }
  if (thickness) memcpy(thickness, th.data(), vals * 8);
  if (cover) memcpy(cover, cv.data(), vals * 8);
  if (sections) memcpy(sections, ns.data(), vals * 4);
  return 0;
}

// smx_cores. 0; 1 where *total > cap (count and *total written, the section arrays untouched); -5 with *bad_cell and nothing written; -2.
int sh_cores(sh_map* h, uint32_t lanes, uint32_t nblocks, const uint32_t* cells, uint32_t n, uint32_t* count, uint64_t cap, uint64_t* total, uint32_t* type,
             double* size, double* floor, double* sat, uint64_t* bad_cell) {
  if (!shape_ok(lanes, nblocks)) return -2;
  if (n == 0) { *total = 0; return 0; }
  const StrataMap m = host_map(h);
  for (uint32_t i = 0; i < n; i++) if (cells[i] >= m.ncells) { *bad_cell = i; return -2; }
  std::vector<uint32_t> cnt(n, 0xDEADBEEFu);
  std::vector<uint64_t> base(n);
  uint64_t bad = 0ull;
  StrataHostGroup g{lanes};
  for (uint32_t b = 0; b < nblocks; b++) core_count_group(m, g, b, nblocks, cells, n, cnt.data(), &bad);
  uint64_t run = 0;
  for (uint32_t i = 0; i < n; i++) { base[i] = run; run += core_widen(cnt.data(), i); }   // the exclusive scan
  if (bad) { *bad_cell = strata_bad_cell(bad); return -5; }
  *total = run;
  memcpy(count, cnt.data(), (size_t)n * 4);
  if (run > cap) return 1;
  std::vector<uint32_t> ty(run);
  std::vector<double> sz(run), fl(run), st(run);
  for (uint32_t b = 0; b < nblocks; b++) core_scatter_group(m, g, b, nblocks, cells, n, cnt.data(), base.data(), run, ty.data(), sz.data(), fl.data(), st.data());
  if (run) { memcpy(type, ty.data(), run * 4); memcpy(size, sz.data(), run * 8); memcpy(floor, fl.data(), run * 8); memcpy(sat, st.data(), run * 8); }
  return 0;
}

}  // extern "C"
