// soil_drain.h -- drainage (smx_drainage / smx_ensemble_drainage): every dry cell's receiver, the basin every cell drains into, one
// record per basin and the contributing area. The bodies of k_drain_recv, k_drain_resolve, k_drain_stats, k_drain_pending and
// k_drain_area. Nothing here writes a map.
//
// h(c) is Layermap::height: floor + size of the top record in one f64 addition, 0.0 for an empty column. A WET cell and a LAKE are
// those of soil_lakes.h. A wet cell has no receiver. A dry cell's RECEIVER is the in-map cell n among its eight neighbours with
// h(n) < h(c) and the smallest (h(n), n) -- plain f64 `<`, then the smaller cell index: -0 and +0 tie, a NaN is never lower and never
// has a lower neighbour. A dry cell without one is a SINK. A path strictly descends in h, so it ends at a sink or at the first wet
// cell it meets; the TERMINAL of a cell is that sink, or the smallest cell of that lake (a wet cell's: its own lake's). A BASIN is
// the set of cells of one terminal, its identity first_cell the terminal's index, its rank its place in ascending first_cell.
// area(c) = 1 + the areas of the cells whose receiver is c, as u32.
//
// All members of one call share u32 planes, member i at words [off_i, off_i + dimx_i*dimy_i); indices in them are PLANE indices:
//   T   first the lake forest of soil_lakes.h (its tile, merge and flatten kernels run on it: a wet cell holds its lake's root, a dry
//       cell LAKE_DRY); recv makes it the downstream pointer (the receiver; the cell itself for a sink; a wet cell keeps its root);
//       resolve makes it the terminal; stats makes it the basin's rank: the label plane.
//   R   the receiver, DRAIN_NONE for a sink and for a wet cell. Written by recv, read-only afterwards.
//   B   the exclusive prefix sum of the terminal marks (T[g] == g) over the whole plane: the caller's business, as in the census.
//   P   donors still to report to the cell (area only).      AR   the area (area only).
// The steps, each one launch for all members (blockIdx.y = member):
//   recv     a TX x TY tile of heights with a halo of one is loaded into LDS (a cell outside the map is a NaN there: never lower);
//            each dry cell picks its receiver from the tile. The same workgroups set the member's records to the fold's identities.
//   resolve  T[g] = the terminal of g's path, by chasing T with agent-scope atomics (other workgroups store into the chain meanwhile).
//   stats    as k_lake_stats: the rank B[T[g]] - B[off] replaces T[g]; the cell's figures are combined per basin in an LDS table,
//            then ONE set of atomics per basin and workgroup goes to the record. Integer adds and order-free extremes only.
//   pending  P[g] = the number of neighbours whose receiver is g, counted from R without atomics: DRAIN_LEAF for a dry cell with no
//            donor, DRAIN_WET for a wet cell. AR[g] = 1.
//   area     a lane that owns a LEAF walks downstream: it adds its cell's area to the receiver and decrements the receiver's P; only
//            the lane that takes P from 1 to 0 -- every donor has reported -- reads the receiver's area and carries on from there.
//            No lane ever waits for another, and u32 adds make the result independent of the order.
// The file compiles for the device and, under SMX_D / SMX_HOSTSIM, for the host (tests/drainage_host), as soil_lakes.h does.
#pragma once
#include "soil_lakes.h"

#ifdef SMX_HOSTSIM
#define SMX_DRAIN_DEC_RELEASE(p) smx::lake_hs_add((p), 0xFFFFFFFFu)
#define SMX_DRAIN_ACQUIRE() (void)0
#else
// the decrement releases the area add in front of it; the one lane that goes on acquires the other donors' adds
#define SMX_DRAIN_DEC_RELEASE(p) __hip_atomic_fetch_sub((p), 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT)
#define SMX_DRAIN_ACQUIRE() __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent")
#endif

namespace smx {

constexpr uint32_t DRAIN_NONE = 0xFFFFFFFFu;   // R: no receiver
constexpr uint32_t DRAIN_LEAF = 0xFFFFFFFFu;   // P: a dry cell nobody drains into (nobody ever decrements it)
constexpr uint32_t DRAIN_WET = 0x80000000u;    // P: where a wet cell starts; at most eight decrements: it never reads 1, 0 or DRAIN_LEAF
constexpr uint32_t DRAIN_F_LAKE = 1u, DRAIN_F_BORDER = 2u;

struct BasinAcc {     // a record while it is folded (48 bytes, as smx_basin): the extremes as ordered images, the box as four words
  uint32_t first_cell, cells, wet_cells, flags;
  uint64_t hmin, hmax;
  uint32_t x0, y0, x1, y1;
};
struct BasinRec {     // == smx_basin (include/soilmx.h)
  uint32_t first_cell, cells, wet_cells, flags;
  double height_min, height_max;
  uint16_t x0, y0, x1, y1;
  uint32_t reserved[2];
};
static_assert(sizeof(BasinAcc) == 48 && sizeof(BasinRec) == 48, "basin record layouts");

SMX_HD void drain_finish(const BasinAcc& a, BasinRec& r) {
  r.first_cell = a.first_cell; r.cells = a.cells; r.wet_cells = a.wet_cells; r.flags = a.flags;
  r.height_min = lake_unkey(a.hmin); r.height_max = lake_unkey(a.hmax);
  r.x0 = (uint16_t)a.x0; r.y0 = (uint16_t)a.y0; r.x1 = (uint16_t)a.x1; r.y1 = (uint16_t)a.y1;
  r.reserved[0] = r.reserved[1] = 0u;
}
SMX_D double drain_height(const Sec& s) { return s.type == EMPTY ? 0.0 : s.floor + s.size; }

// ---- recv: workgroup `tile` of member m; hs: (TX + 2) * (TY + 2) doubles of LDS. (m.cap: basin records kept for the member) ----
template <int TX, int TY, class G>
SMX_D void drain_recv_group(const LakeMember& m, G& g, uint32_t tile, uint32_t ntiles, double* hs, uint32_t* T, uint32_t* R, BasinAcc* acc) {
  constexpr int HY = TY + 2, HN = (TX + 2) * HY;
  const uint32_t nl = g.lanes();
  const int nty = (m.dimy + TY - 1) / TY;
  const int x0 = (int)(tile / (uint32_t)nty) * TX, y0 = (int)(tile % (uint32_t)nty) * TY;
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    for (uint32_t i = l; i < (uint32_t)HN; i += nl) {   // (y runs fastest: adjacent lanes, adjacent records)
      const int x = x0 - 1 + (int)(i / HY), y = y0 - 1 + (int)(i % HY);
      const bool in = x >= 0 && y >= 0 && x < m.dimx && y < m.dimy;
      hs[i] = in ? drain_height(m.cells[(size_t)x * m.dimy + y]) : __builtin_nan("");
    }
    for (uint64_t r = (uint64_t)tile * nl + l; r < m.cap; r += (uint64_t)ntiles * nl) {
      BasinAcc z;
      z.first_cell = 0u; z.cells = 0u; z.wet_cells = 0u; z.flags = 0u; z.hmin = ~0ull; z.hmax = 0ull;
      z.x0 = 0xFFFFFFFFu; z.y0 = 0xFFFFFFFFu; z.x1 = 0u; z.y1 = 0u;
      acc[m.rec0 + r] = z;
    }
  }
  g.barrier();
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    for (uint32_t i = l; i < (uint32_t)(TX * TY); i += nl) {
      const int lx = (int)(i / TY), ly = (int)(i % TY);
      const int x = x0 + lx, y = y0 + ly;
      if (x >= m.dimx || y >= m.dimy) continue;
      const uint32_t c = (uint32_t)x * (uint32_t)m.dimy + (uint32_t)y;
      const size_t a = (size_t)m.off + c;
      if (T[a] != LAKE_DRY) { R[a] = DRAIN_NONE; continue; }   // (wet: T[a] stays the lake's root, set by the launches before)
      const double* p = hs + (lx + 1) * HY + (ly + 1);
      double best = *p;   // (h(c): a neighbour must be lower; a NaN here or there compares false)
      uint32_t recv = DRAIN_NONE;
      for (int dx = -1; dx <= 1; dx++)       // (ascending cell index: of equal heights the first one stays)
        for (int dy = -1; dy <= 1; dy++) {
          if (dx == 0 && dy == 0) continue;
          const double hn = p[dx * HY + dy];
          if (hn < best) { best = hn; recv = c + (uint32_t)(dx * m.dimy + dy); }   // (unsigned: a cell index may pass 2^31)
        }
      R[a] = recv == DRAIN_NONE ? DRAIN_NONE : m.off + recv;
      T[a] = recv == DRAIN_NONE ? (uint32_t)a : m.off + recv;
    }
  }
}

// ---- resolve: workgroup `block` takes g.lanes() cells ----
template <class G>
SMX_D void drain_resolve_group(const LakeMember& m, G& g, uint32_t block, uint32_t* T) {
  const uint32_t nl = g.lanes();
  const uint64_t n = (uint64_t)m.dimx * (uint64_t)m.dimy;
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    const uint64_t c = (uint64_t)block * nl + l;
    if (c >= n) continue;
    const uint32_t a = m.off + (uint32_t)c;
    uint32_t p = SMX_LAKE_LD(T + a, SMX_LAKE_AGENT);
    if (p == a) continue;   // a sink, or a lake's root
    // Every value T[q] ever holds is q itself (a terminal), q's receiver, q's lake root, or -- stored by this loop in another lane --
    // the terminal of q's path: always a cell further down q's path. A path strictly descends in h over the dry cells and then takes
    // one step to a root, so it is finite and has no cycle: p moves down it with every turn and reaches the terminal.
    for (;;) {
      const uint32_t q = SMX_LAKE_LD(T + p, SMX_LAKE_AGENT);
      if (q == p) break;
      p = q;
    }
    SMX_LAKE_ST(T + a, p, SMX_LAKE_AGENT);
  }
}

// ---- stats: workgroup `block` takes (SLOTS / lanes) * lanes cells; the LDS table has a slot for every one of them ----
template <int SLOTS>
struct BasinTable {
  uint64_t hmin[SLOTS], hmax[SLOTS];
  uint32_t key[SLOTS], cells[SLOTS], wet[SLOTS], x0[SLOTS], y0[SLOTS], x1[SLOTS], y1[SLOTS], flags[SLOTS];
};

template <int SLOTS, class G>
SMX_D void drain_stats_group(const LakeMember& m, G& g, uint32_t block, BasinTable<SLOTS>& t, uint32_t* T, const uint32_t* B, BasinAcc* acc, uint32_t* nbasins) {
  const uint32_t nl = g.lanes(), items = (uint32_t)SLOTS / nl;
  const uint64_t n = (uint64_t)m.dimx * (uint64_t)m.dimy, c0 = (uint64_t)block * items * nl;
  for (uint32_t l = g.lo(); l < g.hi(); l++)
    for (uint32_t s = l; s < (uint32_t)SLOTS; s += nl) {
      t.key[s] = LAKE_DRY; t.cells[s] = 0u; t.wet[s] = 0u; t.hmin[s] = ~0ull; t.hmax[s] = 0ull;
      t.x0[s] = 0xFFFFFFFFu; t.y0[s] = 0xFFFFFFFFu; t.x1[s] = 0u; t.y1[s] = 0u; t.flags[s] = 0u;
    }
  g.barrier();
  const uint32_t before = B[m.off];   // terminals of the members in front of this one
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    for (uint32_t it = 0; it < items; it++) {
      const uint64_t c = c0 + (uint64_t)it * nl + l;
      if (c >= n) break;
      const size_t a = (size_t)m.off + (size_t)c;
      const uint32_t term = T[a];   // (resolved by the launch before; this kernel rewrites T[a] only, and only this lane reads it)
      if (c == n - 1) *nbasins = B[a] + (term == (uint32_t)a ? 1u : 0u) - before;
      const uint32_t rank = B[term] - before;
      T[a] = rank;
      if (rank >= m.cap) continue;
      const Sec top = m.cells[c];
      const bool wet = top.type == AIR;
      const uint32_t x = (uint32_t)(c / (uint64_t)m.dimy), y = (uint32_t)(c % (uint64_t)m.dimy);
      const bool border = x == 0u || y == 0u || x == (uint32_t)m.dimx - 1u || y == (uint32_t)m.dimy - 1u;
      uint32_t f = 0u;
      if (term == (uint32_t)a) {   // the terminal itself: a sink (dry) or a lake's first cell (wet)
        acc[m.rec0 + rank].first_cell = (uint32_t)c;   // (its only writer)
        if (wet) f |= DRAIN_F_LAKE;
      }
      if (border && (wet || term == (uint32_t)a)) f |= DRAIN_F_BORDER;   // (a wet cell of the basin is a cell of its lake)
      uint32_t s = (rank * 2654435761u) % (uint32_t)SLOTS;
      for (;;) {   // (at most SLOTS keys are ever inserted: a free or matching slot exists)
        const uint32_t k = SMX_LAKE_CAS(t.key + s, LAKE_DRY, rank, SMX_LAKE_WG);
        if (k == LAKE_DRY || k == rank) break;
        s = s + 1u == (uint32_t)SLOTS ? 0u : s + 1u;
      }
      SMX_LAKE_ADD(t.cells + s, 1u, SMX_LAKE_WG);
      if (wet) SMX_LAKE_ADD(t.wet + s, 1u, SMX_LAKE_WG);
      const uint64_t kh = lake_key(drain_height(top));
      SMX_LAKE_MIN(t.hmin + s, kh, SMX_LAKE_WG); SMX_LAKE_MAX(t.hmax + s, kh, SMX_LAKE_WG);
      SMX_LAKE_MIN(t.x0 + s, x, SMX_LAKE_WG); SMX_LAKE_MAX(t.x1 + s, x, SMX_LAKE_WG);
      SMX_LAKE_MIN(t.y0 + s, y, SMX_LAKE_WG); SMX_LAKE_MAX(t.y1 + s, y, SMX_LAKE_WG);
      if (f) SMX_LAKE_OR(t.flags + s, f, SMX_LAKE_WG);
    }
  }
  g.barrier();
  for (uint32_t l = g.lo(); l < g.hi(); l++)
    for (uint32_t s = l; s < (uint32_t)SLOTS; s += nl) {
      if (t.key[s] == LAKE_DRY) continue;
      BasinAcc& r = acc[m.rec0 + t.key[s]];
      SMX_LAKE_ADD(&r.cells, t.cells[s], SMX_LAKE_AGENT);
      if (t.wet[s]) SMX_LAKE_ADD(&r.wet_cells, t.wet[s], SMX_LAKE_AGENT);
      SMX_LAKE_MIN(&r.hmin, t.hmin[s], SMX_LAKE_AGENT); SMX_LAKE_MAX(&r.hmax, t.hmax[s], SMX_LAKE_AGENT);
      SMX_LAKE_MIN(&r.x0, t.x0[s], SMX_LAKE_AGENT); SMX_LAKE_MAX(&r.x1, t.x1[s], SMX_LAKE_AGENT);
      SMX_LAKE_MIN(&r.y0, t.y0[s], SMX_LAKE_AGENT); SMX_LAKE_MAX(&r.y1, t.y1[s], SMX_LAKE_AGENT);
      if (t.flags[s]) SMX_LAKE_OR(&r.flags, t.flags[s], SMX_LAKE_AGENT);
    }
}

// ---- pending: workgroup `block` takes g.lanes() cells (R is read-only here) ----
template <class G>
SMX_D void drain_pending_group(const LakeMember& m, G& g, uint32_t block, const uint32_t* R, uint32_t* P, uint32_t* AR) {
  const uint32_t nl = g.lanes();
  const uint64_t n = (uint64_t)m.dimx * (uint64_t)m.dimy;
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    const uint64_t c = (uint64_t)block * nl + l;
    if (c >= n) continue;
    const uint32_t a = m.off + (uint32_t)c;
    const int x = (int)(c / (uint64_t)m.dimy), y = (int)(c % (uint64_t)m.dimy);
    uint32_t donors = 0u;
    for (int dx = -1; dx <= 1; dx++)
      for (int dy = -1; dy <= 1; dy++) {
        const int u = x + dx, v = y + dy;
        if ((dx == 0 && dy == 0) || u < 0 || v < 0 || u >= m.dimx || v >= m.dimy) continue;
        if (R[(size_t)m.off + (size_t)u * m.dimy + v] == a) donors++;
      }
    const bool wet = m.cells[c].type == AIR;
    // a wet cell starts at DRAIN_WET: no decrement ever takes it from 1 to 0, so every walk ends at the first wet cell it reaches,
    // and its word never becomes DRAIN_LEAF, so its own lane never starts a walk
    P[a] = wet ? DRAIN_WET : (donors ? donors : DRAIN_LEAF);
    AR[a] = 1u;
  }
}

// ---- area: workgroup `block` takes g.lanes() cells; every access to P and AR is an agent-scope atomic (other workgroups walk through
//      the same words, and a plain load may be served from a cache that never sees their writes) ----
template <class G>
SMX_D void drain_area_group(const LakeMember& m, G& g, uint32_t block, const uint32_t* R, uint32_t* P, uint32_t* AR) {
  const uint32_t nl = g.lanes();
  const uint64_t n = (uint64_t)m.dimx * (uint64_t)m.dimy;
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    const uint64_t c = (uint64_t)block * nl + l;
    if (c >= n) continue;
    uint32_t cur = m.off + (uint32_t)c;
    if (SMX_LAKE_LD(P + cur, SMX_LAKE_AGENT) != DRAIN_LEAF) continue;   // (a leaf's P never changes: no cell drains into it; a wet cell's stays within 8 of DRAIN_WET)
    uint32_t area = 1u;                                                  // (... and nobody adds to its area)
    // Every turn moves cur to its receiver, one step down a path that strictly descends in h: the walk ends at a sink, at a wet
    // cell, or earlier, where another donor is still to report. It never waits: the lane whose decrement is the last one goes on.
    for (;;) {
      const uint32_t r = R[cur];
      if (r == DRAIN_NONE) break;                        // cur is a sink: its area is complete
      SMX_LAKE_ADD(AR + r, area, SMX_LAKE_AGENT);
      if (SMX_DRAIN_DEC_RELEASE(P + r) != 1u) break;     // a donor of r is still to come (or r is wet)
      SMX_DRAIN_ACQUIRE();                               // every donor's add happened before its decrement: r's area is complete
      area = SMX_LAKE_LD(AR + r, SMX_LAKE_AGENT);
      cur = r;
    }
  }
}

}  // namespace smx
