// soil_lakes.h -- the lake census (smx_lakes / smx_ensemble_lakes): connected-component labelling of the wet cells and one record
// per lake. The bodies of k_lake_tiles, k_lake_merge, k_lake_flatten and k_lake_stats. Nothing here writes a map.
//
// A WET cell is a non-empty column whose top section is Air (cells[c].type == AIR; an empty column has type EMPTY). A LAKE is a
// maximal set of wet cells connected through the EIGHT neighbours WaterParticle::cascade levels water over (water.h:155-164); cells
// do not connect across the map border. A lake's identity is its smallest cell index x*dimy+y (first_cell); lakes are listed in
// ascending first_cell and lake k of that order has rank k.
//
// All members of one call share two u32 planes, member i at words [off_i, off_i + dimx_i*dimy_i):
//   A   the union-find forest: A[g] = a wet cell of the same lake with an index <= g (g itself: a root), LAKE_DRY for a dry cell.
//       Indices are PLANE indices (off_i + cell), so that "g is a root" is A[g] == g for every member at once.
//   B   the exclusive prefix sum of the root marks (A[g] == g) over the whole plane: B[root] - B[off_i] is the lake's rank.
// The steps, each one launch for all members (blockIdx.y = member):
//   tiles    a TX x TY tile of cells is labelled in LDS (union-find with atomicMin towards the smaller index over the four forward
//            neighbours (1,-1) (1,0) (1,1) (0,1), which name every neighbour pair once), flattened, and written to A as the plane
//            index of the tile-local root. The order of cells inside a tile is the order of their cell indices, so the local root is
//            the smallest cell of its piece. The same workgroups set the member's records to the fold's identities.
//   merge    the forward pairs that cross a tile edge or corner are united on A. Every hook goes from a root to a smaller index, so
//            labels only decrease, every loop ends, a tree's root is its smallest cell, and no workgroup ever waits for another.
//            Every access to A in this kernel is an agent-scope atomic: another workgroup may be writing the word, and a plain load
//            may be served from a cache that never sees that write.
//   flatten  A[g] = root(g) for every wet cell (the same atomics: a chain may run through words that other workgroups flatten).
//   scan     B = exclusive sum of (A[g] == g): the caller's business (rocPRIM on the device, a loop in tests/lakes_host).
//   stats    per wet cell the rank B[A[g]] - B[off]; A[g] becomes that rank (the label plane); the cell's figures are combined per
//            lake in an LDS table first, then ONE set of atomics per lake and workgroup goes to the record. Integer adds, and
//            min / max on an order-preserving integer image of the f64 bits: nothing depends on the order of the contributions.
// The file compiles for the device and, under SMX_D / SMX_HOSTSIM, for the host (tests/lakes_host runs the same bodies with the lanes
// of a workgroup looped), with the group object of soil_observe.h: lanes(), lo(), hi(), barrier().
#pragma once
#include "soil_core.h"

namespace smx {
#ifdef SMX_HOSTSIM
// (one lane after the other: a read-modify-write is a read and a write)
template <class T> inline T lake_hs_add(T* p, T v) { const T o = *p; *p = (T)(o + v); return o; }
template <class T> inline T lake_hs_min(T* p, T v) { const T o = *p; if (v < o) *p = v; return o; }
template <class T> inline T lake_hs_max(T* p, T v) { const T o = *p; if (v > o) *p = v; return o; }
template <class T> inline T lake_hs_or(T* p, T v) { const T o = *p; *p = (T)(o | v); return o; }
template <class T> inline T lake_hs_cas(T* p, T e, T d) { const T o = *p; if (o == e) *p = d; return o; }
}  // namespace smx
#define SMX_LAKE_WG 0
#define SMX_LAKE_AGENT 0
#define SMX_LAKE_LD(p, scope) (*(p))
#define SMX_LAKE_ST(p, v, scope) (void)(*(p) = (v))
#define SMX_LAKE_ADD(p, v, scope) smx::lake_hs_add((p), (v))
#define SMX_LAKE_MIN(p, v, scope) smx::lake_hs_min((p), (v))
#define SMX_LAKE_MAX(p, v, scope) smx::lake_hs_max((p), (v))
#define SMX_LAKE_OR(p, v, scope) smx::lake_hs_or((p), (v))
#define SMX_LAKE_CAS(p, e, d, scope) smx::lake_hs_cas((p), (e), (d))
namespace smx {
#else
template <int SCOPE, class T> SMX_D T lake_dev_cas(T* p, T e, T d) {
  __hip_atomic_compare_exchange_strong(p, &e, d, __ATOMIC_RELAXED, __ATOMIC_RELAXED, SCOPE);
  return e;
}
}  // namespace smx
#define SMX_LAKE_WG __HIP_MEMORY_SCOPE_WORKGROUP
#define SMX_LAKE_AGENT __HIP_MEMORY_SCOPE_AGENT
#define SMX_LAKE_LD(p, scope) __hip_atomic_load((p), __ATOMIC_RELAXED, scope)
#define SMX_LAKE_ST(p, v, scope) __hip_atomic_store((p), (v), __ATOMIC_RELAXED, scope)
#define SMX_LAKE_ADD(p, v, scope) __hip_atomic_fetch_add((p), (v), __ATOMIC_RELAXED, scope)
#define SMX_LAKE_MIN(p, v, scope) __hip_atomic_fetch_min((p), (v), __ATOMIC_RELAXED, scope)
#define SMX_LAKE_MAX(p, v, scope) __hip_atomic_fetch_max((p), (v), __ATOMIC_RELAXED, scope)
#define SMX_LAKE_OR(p, v, scope) __hip_atomic_fetch_or((p), (v), __ATOMIC_RELAXED, scope)
#define SMX_LAKE_CAS(p, e, d, scope) smx::lake_dev_cas<scope>((p), (e), (d))
namespace smx {
#endif

constexpr uint32_t LAKE_DRY = 0xFFFFFFFFu;   // A / the label plane: a dry cell; also the LDS table's free key
constexpr uint32_t LAKE_F_BORDER = 1u, LAKE_F_VOLUME = 2u;

struct LakeMember {   // one map of the call; 32 bytes
  const Sec* cells;
  int32_t dimx, dimy;
  uint32_t off;       // its first word in A and B
  uint32_t cap;       // records kept for it: lakes of rank < cap
  uint32_t rec0;      // its first record in the table
  uint32_t pad;
};
struct LakeAcc {      // a record while it is folded (64 bytes, as smx_lake): the extremes as ordered images, the box as four words
  uint32_t first_cell, cells;
  uint64_t volume_q40, lmin, lmax, dmax;
  uint32_t x0, y0, x1, y1, flags, pad;
};
struct LakeRec {      // == smx_lake (include/soilmx.h)
  uint32_t first_cell, cells;
  uint64_t volume_q40;
  double level_min, level_max, depth_max;
  uint16_t x0, y0, x1, y1;
  uint32_t flags;
  uint32_t reserved[3];
};
static_assert(sizeof(LakeMember) == 32 && sizeof(LakeAcc) == 64 && sizeof(LakeRec) == 64, "lake record layouts");

// the order-preserving image of an f64: a < b as doubles (and -0 < +0) <=> key(a) < key(b) as u64
SMX_HD uint64_t lake_key(double v) {
  uint64_t b;
  __builtin_memcpy(&b, &v, 8);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
SMX_HD double lake_unkey(uint64_t k) {
  const uint64_t b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
  double v;
  __builtin_memcpy(&v, &b, 8);
  return v;
}
// floor(size * 2^40) of one wet cell; a size that is not finite, is negative or is >= 2^24 contributes 0 and raises LAKE_F_VOLUME
SMX_HD uint64_t lake_q40(double size, uint32_t& flags) {
  if (!(size >= 0.0) || !(size < 16777216.0)) { flags |= LAKE_F_VOLUME; return 0ull; }
  return (uint64_t)floor(size * 1099511627776.0);
}
SMX_HD void lake_finish(const LakeAcc& a, LakeRec& r) {
  r.first_cell = a.first_cell; r.cells = a.cells; r.volume_q40 = a.volume_q40;
  r.level_min = lake_unkey(a.lmin); r.level_max = lake_unkey(a.lmax); r.depth_max = lake_unkey(a.dmax);
  r.x0 = (uint16_t)a.x0; r.y0 = (uint16_t)a.y0; r.x1 = (uint16_t)a.x1; r.y1 = (uint16_t)a.y1;
  r.flags = a.flags; r.reserved[0] = r.reserved[1] = r.reserved[2] = 0u;
}
SMX_HD uint32_t lake_tiles(const LakeMember& m, int tx, int ty) {
  return (uint32_t)((m.dimx + tx - 1) / tx) * (uint32_t)((m.dimy + ty - 1) / ty);
}

// ---- union-find towards the smaller index (L: the LDS tile or the plane A) ----
template <int SCOPE>
SMX_D uint32_t lake_find(uint32_t* L, uint32_t a) {
  for (;;) {
    const uint32_t p = SMX_LAKE_LD(L + a, SCOPE);
    if (p == a) return a;
    a = p;   // (p < a: the chain ends)
  }
}
template <int SCOPE>
SMX_D void lake_union(uint32_t* L, uint32_t a, uint32_t b) {
  for (;;) {
    a = lake_find<SCOPE>(L, a);
    b = lake_find<SCOPE>(L, b);
    if (a == b) return;
    if (a < b) { const uint32_t t = a; a = b; b = t; }
    const uint32_t old = SMX_LAKE_MIN(L + a, b, SCOPE);
    if (old == a) return;   // a was a root and now hangs under b
    a = old;                // somebody hooked a first (old < a); whatever the word holds now, old's tree and b's are still to be united
  }
}

// ---- tiles: workgroup `tile` of member m labels its TX x TY cells in `lab` (LDS, TX*TY words) ----
template <int TX, int TY, class G>
SMX_D void lake_tile_group(const LakeMember& m, G& g, uint32_t tile, uint32_t ntiles, uint32_t* lab, uint32_t* A, LakeAcc* acc) {
  const uint32_t nl = g.lanes();
  const int nty = (m.dimy + TY - 1) / TY;
  const int x0 = (int)(tile / (uint32_t)nty) * TX, y0 = (int)(tile % (uint32_t)nty) * TY;
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    for (uint32_t i = l; i < (uint32_t)(TX * TY); i += nl) {   // (adjacent lanes, adjacent cells: y runs fastest in both orders)
      const int x = x0 + (int)(i / TY), y = y0 + (int)(i % TY);
      const bool wet = x < m.dimx && y < m.dimy && m.cells[(size_t)x * m.dimy + y].type == AIR;
      lab[i] = wet ? i : LAKE_DRY;
    }
    // the member's records: the identities of the fold
    for (uint64_t r = (uint64_t)tile * nl + l; r < m.cap; r += (uint64_t)ntiles * nl) {
      LakeAcc z;
      z.first_cell = 0u; z.cells = 0u; z.volume_q40 = 0ull; z.lmin = ~0ull; z.lmax = 0ull; z.dmax = 0ull;
      z.x0 = 0xFFFFFFFFu; z.y0 = 0xFFFFFFFFu; z.x1 = 0u; z.y1 = 0u; z.flags = 0u; z.pad = 0u;
      acc[m.rec0 + r] = z;
    }
  }
  g.barrier();
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    for (uint32_t i = l; i < (uint32_t)(TX * TY); i += nl) {
      if (SMX_LAKE_LD(lab + i, SMX_LAKE_WG) == LAKE_DRY) continue;
      const int lx = (int)(i / TY), ly = (int)(i % TY);
      if (ly + 1 < TY && SMX_LAKE_LD(lab + i + 1, SMX_LAKE_WG) != LAKE_DRY) lake_union<SMX_LAKE_WG>(lab, i, i + 1u);
      if (lx + 1 >= TX) continue;
      for (int dy = -1; dy <= 1; dy++) {
        if (ly + dy < 0 || ly + dy >= TY) continue;
        const uint32_t j = (uint32_t)((int)i + TY + dy);
        if (SMX_LAKE_LD(lab + j, SMX_LAKE_WG) != LAKE_DRY) lake_union<SMX_LAKE_WG>(lab, i, j);
      }
    }
  }
  g.barrier();
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    for (uint32_t i = l; i < (uint32_t)(TX * TY); i += nl) {
      const int x = x0 + (int)(i / TY), y = y0 + (int)(i % TY);
      if (x >= m.dimx || y >= m.dimy) continue;
      uint32_t v = LAKE_DRY;
      if (SMX_LAKE_LD(lab + i, SMX_LAKE_WG) != LAKE_DRY) {
        const uint32_t r = lake_find<SMX_LAKE_WG>(lab, i);   // (nobody hooks any more: a root stays a root)
        v = m.off + (uint32_t)(x0 + (int)(r / TY)) * (uint32_t)m.dimy + (uint32_t)(y0 + (int)(r % TY));
      }
      A[(size_t)m.off + (size_t)x * m.dimy + y] = v;
    }
  }
}

// ---- merge: the forward pairs of tile `tile` that leave it ----
SMX_D void lake_merge_pair(const LakeMember& m, uint32_t* A, uint32_t a, int x, int y) {
  if (x < 0 || y < 0 || x >= m.dimx || y >= m.dimy) return;
  const uint32_t b = m.off + (uint32_t)x * (uint32_t)m.dimy + (uint32_t)y;
  if (SMX_LAKE_LD(A + b, SMX_LAKE_AGENT) == LAKE_DRY) return;
  lake_union<SMX_LAKE_AGENT>(A, a, b);
}
template <int TX, int TY, class G>
SMX_D void lake_merge_group(const LakeMember& m, G& g, uint32_t tile, uint32_t* A) {
  const uint32_t nl = g.lanes();
  const int nty = (m.dimy + TY - 1) / TY;
  const int x0 = (int)(tile / (uint32_t)nty) * TX, y0 = (int)(tile % (uint32_t)nty) * TY;
  // the tile's last column (TY cells: towards x+1, and its last cell towards y+1), the rest of its last row (towards y+1 and
  // (x+1, y+1)), the rest of its first row (towards (x+1, y-1))
  const uint32_t n1 = (uint32_t)TY, n2 = (uint32_t)(TX - 1);
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    for (uint32_t i = l; i < n1 + 2u * n2; i += nl) {
      const int kind = i < n1 ? 0 : (i < n1 + n2 ? 1 : 2);
      const int lx = kind == 0 ? TX - 1 : (int)(i - n1 - (kind == 2 ? n2 : 0u));
      const int ly = kind == 0 ? (int)i : (kind == 1 ? TY - 1 : 0);
      const int x = x0 + lx, y = y0 + ly;
      if (x >= m.dimx || y >= m.dimy) continue;
      const uint32_t a = m.off + (uint32_t)x * (uint32_t)m.dimy + (uint32_t)y;
      if (SMX_LAKE_LD(A + a, SMX_LAKE_AGENT) == LAKE_DRY) continue;
      if (kind == 0) {
        lake_merge_pair(m, A, a, x + 1, y - 1); lake_merge_pair(m, A, a, x + 1, y); lake_merge_pair(m, A, a, x + 1, y + 1);
        if (ly == TY - 1) lake_merge_pair(m, A, a, x, y + 1);
      } else if (kind == 1) {
        lake_merge_pair(m, A, a, x, y + 1); lake_merge_pair(m, A, a, x + 1, y + 1);
      } else {
        lake_merge_pair(m, A, a, x + 1, y - 1);
      }
    }
  }
}

// ---- flatten: workgroup `block` takes g.lanes() cells ----
template <class G>
SMX_D void lake_flatten_group(const LakeMember& m, G& g, uint32_t block, uint32_t* A) {
  const uint32_t nl = g.lanes();
  const uint64_t n = (uint64_t)m.dimx * (uint64_t)m.dimy;
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    const uint64_t c = (uint64_t)block * nl + l;
    if (c >= n) continue;
    const uint32_t a = m.off + (uint32_t)c;
    const uint32_t p = SMX_LAKE_LD(A + a, SMX_LAKE_AGENT);
    if (p == LAKE_DRY || p == a) continue;
    SMX_LAKE_ST(A + a, lake_find<SMX_LAKE_AGENT>(A, p), SMX_LAKE_AGENT);
  }
}

// the root mark the scan sums (the caller's iterator on the device, its loop on the host)
SMX_HD uint32_t lake_mark(const uint32_t* A, size_t g) { return A[g] == (uint32_t)g ? 1u : 0u; }

// ---- stats: workgroup `block` takes (SLOTS / lanes) * lanes cells; the LDS table has a slot for every one of them ----
template <int SLOTS>
struct LakeTable {
  uint64_t vol[SLOTS], lmin[SLOTS], lmax[SLOTS], dmax[SLOTS];
  uint32_t key[SLOTS], cells[SLOTS], x0[SLOTS], y0[SLOTS], x1[SLOTS], y1[SLOTS], flags[SLOTS];
};
SMX_HD uint32_t lake_stats_cells(uint32_t slots, uint32_t lanes) { return (slots / lanes) * lanes; }

template <int SLOTS, class G>
SMX_D void lake_stats_group(const LakeMember& m, G& g, uint32_t block, LakeTable<SLOTS>& t, uint32_t* A, const uint32_t* B, LakeAcc* acc, uint32_t* nlakes) {
  const uint32_t nl = g.lanes(), items = (uint32_t)SLOTS / nl;
  const uint64_t n = (uint64_t)m.dimx * (uint64_t)m.dimy, c0 = (uint64_t)block * items * nl;
  for (uint32_t l = g.lo(); l < g.hi(); l++)
    for (uint32_t s = l; s < (uint32_t)SLOTS; s += nl) {
      t.key[s] = LAKE_DRY; t.cells[s] = 0u; t.vol[s] = 0ull; t.lmin[s] = ~0ull; t.lmax[s] = 0ull; t.dmax[s] = 0ull;
      t.x0[s] = 0xFFFFFFFFu; t.y0[s] = 0xFFFFFFFFu; t.x1[s] = 0u; t.y1[s] = 0u; t.flags[s] = 0u;
    }
  g.barrier();
  const uint32_t before = B[m.off];   // roots of the members in front of this one
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    for (uint32_t it = 0; it < items; it++) {
      const uint64_t c = c0 + (uint64_t)it * nl + l;
      if (c >= n) break;
      const size_t a = (size_t)m.off + (size_t)c;
      const uint32_t root = A[a];   // (flattened by the launch before; this kernel rewrites A[a] only, and only this lane reads it)
      if (c == n - 1) *nlakes = B[a] + (root == (uint32_t)a ? 1u : 0u) - before;
      if (root == LAKE_DRY) continue;
      const uint32_t rank = B[root] - before;
      A[a] = rank;
      if (rank >= m.cap) continue;
      if (root == (uint32_t)a) acc[m.rec0 + rank].first_cell = (uint32_t)c;   // (its only writer)
      const uint32_t x = (uint32_t)(c / (uint64_t)m.dimy), y = (uint32_t)(c % (uint64_t)m.dimy);
      const double size = m.cells[c].size, fl = m.cells[c].floor;
      uint32_t f = (x == 0u || y == 0u || x == (uint32_t)m.dimx - 1u || y == (uint32_t)m.dimy - 1u) ? LAKE_F_BORDER : 0u;
      const uint64_t q = lake_q40(size, f);
      uint32_t s = (rank * 2654435761u) % (uint32_t)SLOTS;
      for (;;) {   // (at most SLOTS keys are ever inserted: a free or matching slot exists)
        const uint32_t k = SMX_LAKE_CAS(t.key + s, LAKE_DRY, rank, SMX_LAKE_WG);
        if (k == LAKE_DRY || k == rank) break;
        s = s + 1u == (uint32_t)SLOTS ? 0u : s + 1u;
      }
      SMX_LAKE_ADD(t.cells + s, 1u, SMX_LAKE_WG);
      if (q) { const uint64_t o = SMX_LAKE_ADD(t.vol + s, q, SMX_LAKE_WG); if (o + q < o) f |= LAKE_F_VOLUME; }
      const uint64_t kl = lake_key(fl + size), kd = lake_key(size);
      SMX_LAKE_MIN(t.lmin + s, kl, SMX_LAKE_WG); SMX_LAKE_MAX(t.lmax + s, kl, SMX_LAKE_WG); SMX_LAKE_MAX(t.dmax + s, kd, SMX_LAKE_WG);
      SMX_LAKE_MIN(t.x0 + s, x, SMX_LAKE_WG); SMX_LAKE_MAX(t.x1 + s, x, SMX_LAKE_WG);
      SMX_LAKE_MIN(t.y0 + s, y, SMX_LAKE_WG); SMX_LAKE_MAX(t.y1 + s, y, SMX_LAKE_WG);
      if (f) SMX_LAKE_OR(t.flags + s, f, SMX_LAKE_WG);
    }
  }
  g.barrier();
  for (uint32_t l = g.lo(); l < g.hi(); l++)
    for (uint32_t s = l; s < (uint32_t)SLOTS; s += nl) {
      if (t.key[s] == LAKE_DRY) continue;
      LakeAcc& r = acc[m.rec0 + t.key[s]];
      uint32_t f = t.flags[s];
      SMX_LAKE_ADD(&r.cells, t.cells[s], SMX_LAKE_AGENT);
      if (t.vol[s]) { const uint64_t v = t.vol[s], o = SMX_LAKE_ADD(&r.volume_q40, v, SMX_LAKE_AGENT); if (o + v < o) f |= LAKE_F_VOLUME; }
      SMX_LAKE_MIN(&r.lmin, t.lmin[s], SMX_LAKE_AGENT); SMX_LAKE_MAX(&r.lmax, t.lmax[s], SMX_LAKE_AGENT); SMX_LAKE_MAX(&r.dmax, t.dmax[s], SMX_LAKE_AGENT);
      SMX_LAKE_MIN(&r.x0, t.x0[s], SMX_LAKE_AGENT); SMX_LAKE_MAX(&r.x1, t.x1[s], SMX_LAKE_AGENT);
      SMX_LAKE_MIN(&r.y0, t.y0[s], SMX_LAKE_AGENT); SMX_LAKE_MAX(&r.y1, t.y1[s], SMX_LAKE_AGENT);
      if (f) SMX_LAKE_OR(&r.flags, f, SMX_LAKE_AGENT);
    }
}

}  // namespace smx
