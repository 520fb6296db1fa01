// budget_host -- TEST-ONLY host build of soilmachine_amd/csrc/soil_budget.h (the bodies of k_budget_fold and k_budget_where) behind
// the drainage chain of tests/drainage_host on the base.
//
// The same headers the kernels are made of, compiled by g++ (-ffp-contract=off) and run with the lanes of a workgroup looped one
// after the other and the workgroups of a launch one after the other, in ascending or descending order. A map holds FULL columns, laid
// out as tests/strata_host lays them out: the top section inline in the cell record, the buried ones in a pool whose order the
// caller may scramble. bh_budget is smx_budget / smx_ensemble_budget in small: results land in scratch, the verdict is taken, and
// only then are the caller's outputs written. tests/budget_host_lib.py builds and binds this file; the product never loads it.
#include "../drainage_host/drainage_host.cpp"
#include "../../soilmachine_amd/csrc/soil_budget.h"

struct bh_map : ah_map {   // (the drainage chain reads the cell records: the columns' tops)
  std::vector<Sec> pool;
};

// the fold's tile shapes beside the chain's (TILE_SHAPES of the same variant): (tile columns, tile rows, slots of the basin table).
// Shape 0 is the kernel's own, shape 2 a tile no dimension is a multiple of, with more slots than cells.
static constexpr Shape FOLD_SHAPES[4] = {{16, 16, 256, 0}, {8, 8, 64, 0}, {5, 7, 40, 0}, {32, 4, 128, 0}};

template <int TX, int TY, int SLOTS>
static void run_budget(const BudgetBase& b, const std::vector<BudgetMap>& maps, uint32_t lanes, int descending, int lanes_descending, const uint32_t* T,
                       BudgetAcc* acc, BudgetSoilRec* soils, uint64_t* bad, const BudgetPlanes& pl) {
  static BudgetBasinTable<SLOTS> bt;   // (the "LDS")
  static BudgetSoilTable st;
  const uint32_t nt = budget_tiles(b.dimx, b.dimy, TX, TY);
  const uint32_t nb = (uint32_t)(((uint64_t)b.dimx * b.dimy + lanes - 1) / lanes);
  // every stretch between two barriers with the lanes one by one, in the order asked for
  auto each_lane = [&](auto&& body) {
    for (uint32_t l = 0; l < lanes; l++) {
      DrainHostLane one{lanes, nth(l, lanes, lanes_descending)};
      body(one);
    }
  };
  for (size_t i = 0; i < maps.size(); i++) {
    const BudgetMap& m = maps[nth((uint32_t)i, (uint32_t)maps.size(), descending)];
    for (uint32_t t = 0; t < nt; t++) {
      const uint32_t tile = nth(t, nt, descending);
      memset(&bt, 0xAB, sizeof(bt)); memset(&st, 0xAB, sizeof(st));   // (whatever the last workgroup left)
      each_lane([&](DrainHostLane& one) { budget_fold_clear(one, bt, st); });
      each_lane([&](DrainHostLane& one) { budget_fold_cells<TX, TY>(b, m, one, tile, bt, st, T, bad, pl); });
      each_lane([&](DrainHostLane& one) { budget_fold_flush(b, m, one, bt, st, acc, soils); });
    }
  }
  if (!b.bcap) return;
  for (const BudgetMap& m : maps)
    for (uint32_t k = 0; k < nb; k++)
      each_lane([&](DrainHostLane& one) { budget_where_group(b, m, one, nth(k, nb, descending), T, acc); });
}

extern "C" {

int bh_rec_bytes(int soil) { return soil ? (int)sizeof(BudgetSoilRec) : (int)sizeof(BudgetBasinRec); }

// columns bottom -> top in cell order (the snapshot layout). scramble != 0: the buried sections take pool indices in the order of a
// stride permutation instead of the import's; `slack` unused records are appended to the pool.
bh_map* bh_create(int dimx, int dimy, const uint32_t* count, const uint32_t* type, const double* size, const double* floor, const double* sat, int scramble,
                  uint32_t slack) {
  bh_map* m = new bh_map();
  m->dimx = dimx; m->dimy = dimy;
  const size_t n = (size_t)dimx * dimy;
  size_t buried = 0;
  for (size_t i = 0; i < n; i++) buried += count[i] ? count[i] - 1u : 0u;
  std::vector<uint32_t> where(buried);
  size_t stride = 1;
  auto gcd = [](size_t a, size_t b) { while (b) { const size_t t = a % b; a = b; b = t; } return a; };
  if (scramble && buried > 2) { stride = buried / 2 + 1; while (gcd(stride, buried) != 1) stride++; }
  for (size_t j = 0; j < buried; j++) where[j] = (uint32_t)((j * stride + (scramble ? 3 : 0)) % buried);
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
void bh_destroy(bh_map* m) { delete m; }
uint64_t bh_pool_size(const bh_map* m) { return m->pool.size(); }
// the `prev` word of a cell's top record (pool == 0) or of a pool record: read, and written where set != 0 (to corrupt a chain)
uint32_t bh_prev(bh_map* m, int pool, uint64_t at, int set, uint32_t value) {
  Sec& s = pool ? m->pool[at] : m->cells[at];
  const uint32_t old = s.prev;
  if (set) s.prev = value;
  return old;
}

int bh_variants() { return (int)std::size(FOLD_SHAPES); }
// (tile columns, tile rows, slots of the basin table) of the fold of a variant
int bh_variant(int v, int* tx, int* ty, int* slots) {
  const Shape* s = shape_at(FOLD_SHAPES, v);
  if (!s) return -2;
  *tx = s->tx; *ty = s->ty; *slots = s->slots;
  return 0;
}

// The budget of maps[0..nm) against `base` in one go, as smx_ensemble_budget runs it (nm == 1: smx_budget). out: nm * cap records, map
// i's from record i * cap, each cut to struct_size; *nbasins: the base's count; soils (NULL = skip): nm * ntypes records cut to
// soil_struct_size; the planes (NULL = skip): nm == 1 only. lanes: 64, 128 or 256; order bit 0: every launch runs its workgroups (and
// the fold its members) last to first; bit 1: the lanes of a workgroup run last to first. 0; -5 with info = {0 for the base or
// 1 + member, the lowest bad cell} and nothing written; -2 for a bad argument.
int bh_budget(bh_map* base, bh_map* const* maps, uint32_t nm, int variant, uint32_t lanes, int order, uint32_t cap, void* out, uint64_t struct_size,
              uint32_t* nbasins, void* soils, uint64_t soil_struct_size, uint32_t ntypes, double* dground, double* dheight, int64_t* dsolid, int64_t* dwater,
              uint64_t* info) {
  if (!base || !lanes_ok(lanes) || struct_size == 0 || (!out && cap)) return -2;
  if (nm == 0) return 0;
  if (!nbasins) return -2;
  if (soils && (soil_struct_size == 0 || ntypes < 1u || ntypes > (uint32_t)BUDGET_MAX_TYPES)) return -2;
  const bool planes = dground || dheight || dsolid || dwater;
  if (planes && nm != 1) return -2;
  for (uint32_t i = 0; i < nm; i++)
    if (!maps[i] || maps[i] == base || maps[i]->dimx != base->dimx || maps[i]->dimy != base->dimy) return -2;
  ah_map* const chain[1] = {base};
  const Members pl = plan_members(chain, 1, cap, CAP_CELLS);
  const uint64_t words = pl.words;
  const uint32_t bcap = pl.tab[0].cap, nt = soils ? ntypes : 0u;
  Planes p;
  poison({&p.T, &p.B, &p.R}, words);
  std::vector<BasinAcc> basin = poisoned_records<BasinAcc>(bcap);
  const int desc = order & 1, ldesc = (order >> 1) & 1;
  uint32_t n = 0xDEADBEEFu;
  std::vector<BudgetAcc> acc((size_t)nm * bcap + 1);              // (the device's begin as zeros: a memset)
  std::vector<BudgetSoilRec> soil((size_t)nm * nt + 1);
  memset(acc.data(), 0, acc.size() * sizeof(BudgetAcc)); memset(soil.data(), 0, soil.size() * sizeof(BudgetSoilRec));
  std::vector<uint64_t> bad(1 + (size_t)nm, 0ull);
  std::vector<double> dg(dground ? words : 0, 777.0), dh(dheight ? words : 0, 777.0);
  std::vector<int64_t> ds(dsolid ? words : 0, 777), dw(dwater ? words : 0, 777);
  const BudgetPlanes bp{dground ? dg.data() : nullptr, dheight ? dh.data() : nullptr, dsolid ? ds.data() : nullptr, dwater ? dw.data() : nullptr};
  std::vector<BudgetMap> tab(nm);
  for (uint32_t i = 0; i < nm; i++) tab[i] = BudgetMap{maps[i]->cells.data(), maps[i]->pool.data(), (uint64_t)maps[i]->pool.size(), i * bcap, i * nt, i, 0u};
  const BudgetBase bb{base->cells.data(), base->pool.data(), (uint64_t)base->pool.size(), base->dimx, base->dimy, bcap, nt};
  const bool fold = bcap || nt || planes;   // (a counting call: the chain alone)
  if (!with_shape<TILE_SHAPES>(variant, [&](auto s) {
        using S = decltype(s);
        run_drainage<S::TX, S::TY, S::SLOTS>(pl.tab, lanes, desc, ldesc, false, p, basin, &n);
      })) return -2;
  if (fold && !with_shape<FOLD_SHAPES>(variant, [&](auto s) {
        using S = decltype(s);
        run_budget<S::TX, S::TY, S::SLOTS>(bb, tab, lanes, desc, ldesc, p.T.data(), acc.data(), soil.data(), bad.data(), bp);
      })) return -2;
  for (size_t i = 0; i < bad.size(); i++)
    if (bad[i]) { if (info) { info[0] = i; info[1] = strata_bad_cell(bad[i]); } return -5; }
  *nbasins = n;
  const uint32_t w = std::min({n, bcap, cap});
  for (size_t i = 0; i < nm; i++) {
    for (uint32_t r = 0; r < w; r++) {
      BudgetBasinRec rec;
      budget_finish(basin[r], acc[i * bcap + r], rec);
      memcpy(static_cast<char*>(out) + (i * cap + r) * struct_size, &rec, std::min<size_t>(struct_size, sizeof(rec)));
    }
    for (uint32_t t = 0; t < nt; t++)
      memcpy(static_cast<char*>(soils) + (i * nt + t) * soil_struct_size, &soil[i * nt + t], std::min<size_t>(soil_struct_size, sizeof(BudgetSoilRec)));
  }
  copy_plane(dground, dg.data(), words); copy_plane(dheight, dh.data(), words);
  copy_plane(dsolid, ds.data(), words); copy_plane(dwater, dw.data(), words);
  return 0;
}

}  // extern "C"
