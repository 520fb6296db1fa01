// soil_spill.h -- spill analysis (smx_spill / smx_ensemble_spill): every basin's pour point, its fill level, its storage and the
// filled surface. The bodies of k_spill_init, k_spill_pass, k_spill_list, k_spill_point, k_spill_relax and k_spill_store. Nothing
// here writes a map.
//
// Cells, h(c), wet cells, lakes, basins, first_cell and the rank are those of soil_drain.h. Heights are ordered by K = lake_key: a
// total order on bit patterns (-0 below +0, a positive NaN above +inf); max and min of heights mean "by K", and a height in a result
// is a copied double. A PASS of basin a is a pair (c, n): c in a, n an in-map cell among c's eight neighbours in another basin, its
// height w = max(h(c), h(n)); a cell c of a on the map border also has the off-map pass (c, SPILL_NONE) with w = h(c). The POUR
// POINT of a basin is its pass with the smallest (K(w), c, n). The FILL LEVEL L(a) = min over the passes of max(w, L(basin(n))), w
// itself for an off-map pass: the minimax height over basin-to-basin routes to the edge of the map. filled(c) = max(h(c),
// L(basin(c))). storage_q40 sums floor((pour_height - h(c)) * 2^40) over the basin's cells with K(h(c)) < K(pour_height),
// fill_storage_q40 the same against the fill level; a difference that is not finite, is negative or is >= 2^24 contributes 0 and
// raises the flag, a wrapped sum raises it too.
//
// The planes are the drainage chain's (all members of a call share them, indices are PLANE indices), run through k_drain_stats
// first, so that T holds every cell's basin rank and B the prefix sum of the terminal marks; plus Q (u32) and H (f64):
//   H   h(c), written by the first pass launch; the store step makes it filled(c) where the plane is asked for.
//   R   the drainage's receiver is not needed here: the first pass launch makes it the BOUNDARY mark, 1 for a cell with a pass.
//   B   after the first pass launch has found the terminals with it: the exclusive prefix sum of the boundary marks (the caller's scan).
//   Q   the boundary cells in ascending order: member i's are Q[B[off_i] .. ), as many as B and R say.
// The basins' table (SpillAcc, one record per basin of every member, member i's from rec0_i; m.cap is the member's NUMBER of basins
// here, known to the host after the drainage chain) is folded as the drainage's records are.
// The steps, each one launch for all members (blockIdx.y = member):
//   init     the table's records become the identities of the fold.
//   pass     PHASE 0 and PHASE 1, two launches. A TX x TY tile of heights and ranks with a halo of one goes into LDS; each cell
//            finds its lowest pass (K(w), n) -- c is its own; the passes are combined per basin in an LDS table, then ONE atomic
//            per basin and workgroup goes to the record. The key (K(w), c, n) is wider than 64 bits: phase 0 takes the minimum of
//            K(w), phase 1 that of (c << 32 | n) among the cells whose lowest pass attains it. Phase 0 also writes H and the
//            boundary marks and lets each terminal cell write its basin's first_cell and lake bit.
//   list     Q[B[g]] = g for every boundary cell g.
//   point    one lane per basin: to_basin = first_cell of the basin of the pour point's n.
//   relax    ONE SWEEP: every boundary cell lowers its basin's level with fetch_min(max(w, L[basin(n)])) over its passes, in place:
//            the update is monotone, so whatever the order the levels end at the same fixed point, never below it on the way. A
//            basin a sweep lowers is counted once (its stamp holds the last sweep that did). The host launches sweeps until one
//            counts nothing. A workgroup strides over the member's list: the count is read on the device.
//   store    per cell the two storage terms, combined per basin in an LDS table as in k_drain_stats, and filled(c).
// No lane waits for another, nothing spins. The file compiles for the device and, under SMX_D / SMX_HOSTSIM, for the host
// (tests/spill_host), as soil_drain.h does.
#pragma once
#include "soil_drain.h"

namespace smx {

constexpr uint32_t SPILL_NONE = 0xFFFFFFFFu;   // pour_to / to_basin: off the map; in the LDS tile of ranks: a cell outside the map
constexpr uint32_t SPILL_F_LAKE = 1u, SPILL_F_OFFMAP = 2u, SPILL_F_NESTED = 4u, SPILL_F_STORAGE = 8u, SPILL_F_FILL_STORAGE = 16u;
constexpr uint32_t SPILL_BATCH = 8u;           // G: relax sweeps the host launches between two looks at the change counts

struct SpillAcc {     // a basin while it is folded (64 bytes): heights as ordered images
  uint32_t first_cell, stamp;       // stamp: the last sweep (counted from 1) that lowered `level`
  uint64_t kw, cn;                  // the pour point: K(w) and (c << 32 | n)
  uint64_t level;                   // K(L)
  uint64_t storage, fill_storage;
  uint32_t cells_below, flags, to_basin, pad;
};
struct SpillRec {     // == smx_spill_record (include/soilmx.h)
  uint32_t first_cell, pour_cell, pour_to, to_basin, flags, cells_below;
  double pour_height, fill_height;
  uint64_t storage_q40, fill_storage_q40;
  uint32_t reserved[2];
};
static_assert(sizeof(SpillAcc) == 64 && sizeof(SpillRec) == 64, "spill record layouts");

SMX_HD void spill_finish(const SpillAcc& a, SpillRec& r) {
  r.first_cell = a.first_cell; r.pour_cell = (uint32_t)(a.cn >> 32); r.pour_to = (uint32_t)a.cn; r.to_basin = a.to_basin;
  r.flags = a.flags | (r.pour_to == SPILL_NONE ? SPILL_F_OFFMAP : 0u) | (a.level > a.kw ? SPILL_F_NESTED : 0u);
  r.cells_below = a.cells_below;
  r.pour_height = lake_unkey(a.kw); r.fill_height = lake_unkey(a.level);
  r.storage_q40 = a.storage; r.fill_storage_q40 = a.fill_storage;
  r.reserved[0] = r.reserved[1] = 0u;
}
// floor(d * 2^40) of one cell below a level; a difference that is not finite, is negative or is >= 2^24 contributes 0 and raises `bit`
SMX_HD uint64_t spill_q40(double d, uint32_t& flags, uint32_t bit) {
  if (!(d >= 0.0) || !(d < 16777216.0)) { flags |= bit; return 0ull; }
  return (uint64_t)floor(d * 1099511627776.0);
}
// the boundary cells of member m: where its list starts in Q and how many there are
SMX_D void spill_list_span(const LakeMember& m, const uint32_t* B, const uint32_t* R, uint32_t& first, uint32_t& count) {
  const size_t last = (size_t)m.off + (size_t)m.dimx * (size_t)m.dimy - 1u;
  first = B[m.off];
  count = B[last] + R[last] - first;
}

// ---- init: workgroup `block` takes g.lanes() records of member m ----
template <class G>
SMX_D void spill_init_group(const LakeMember& m, G& g, uint32_t block, SpillAcc* acc) {
  const uint32_t nl = g.lanes();
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    const uint64_t r = (uint64_t)block * nl + l;
    if (r >= m.cap) continue;
    SpillAcc z;
    z.first_cell = 0u; z.stamp = 0u; z.kw = ~0ull; z.cn = ~0ull; z.level = ~0ull; z.storage = 0ull; z.fill_storage = 0ull;
    z.cells_below = 0u; z.flags = 0u; z.to_basin = SPILL_NONE; z.pad = 0u;
    acc[m.rec0 + r] = z;
  }
}

// ---- pass: workgroup `tile` of member m; hs, ls: (TX + 2) * (TY + 2) doubles / words of LDS; the table has a slot per cell ----
template <int PS>
struct SpillPassTable {
  uint64_t v[PS];
  uint32_t key[PS];
};

template <int TX, int TY, int PS, int PHASE, class G>
SMX_D void spill_pass_group(const LakeMember& m, G& g, uint32_t tile, double* hs, uint32_t* ls, SpillPassTable<PS>& t, const uint32_t* T, const uint32_t* B,
                            uint32_t* R, double* H, SpillAcc* acc) {
  static_assert(PS >= TX * TY, "a slot for every cell of the tile");
  constexpr int HY = TY + 2, HN = (TX + 2) * HY;
  const uint32_t nl = g.lanes();
  const int nty = (m.dimy + TY - 1) / TY;
  const int x0 = (int)(tile / (uint32_t)nty) * TX, y0 = (int)(tile % (uint32_t)nty) * TY;
  const uint64_t n = (uint64_t)m.dimx * (uint64_t)m.dimy;
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    for (uint32_t i = l; i < (uint32_t)HN; i += nl) {   // (y runs fastest: adjacent lanes, adjacent words)
      const int x = x0 - 1 + (int)(i / HY), y = y0 - 1 + (int)(i % HY);
      const bool in = x >= 0 && y >= 0 && x < m.dimx && y < m.dimy;
      const size_t c = in ? (size_t)x * m.dimy + y : 0u;
      hs[i] = !in ? 0.0 : (PHASE == 0 ? drain_height(m.cells[c]) : H[(size_t)m.off + c]);
      ls[i] = in ? T[(size_t)m.off + c] : SPILL_NONE;
    }
    for (uint32_t s = l; s < (uint32_t)PS; s += nl) { t.key[s] = LAKE_DRY; t.v[s] = ~0ull; }
  }
  g.barrier();
  const uint32_t before = PHASE == 0 ? B[m.off] : 0u;   // terminals of the members in front of this one
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    for (uint32_t i = l; i < (uint32_t)(TX * TY); i += nl) {
      const int lx = (int)(i / TY), ly = (int)(i % TY);
      const int x = x0 + lx, y = y0 + ly;
      if (x >= m.dimx || y >= m.dimy) continue;
      const uint32_t c = (uint32_t)x * (uint32_t)m.dimy + (uint32_t)y;
      const size_t a = (size_t)m.off + c;
      const double* p = hs + (lx + 1) * HY + (ly + 1);
      const uint32_t* q = ls + (lx + 1) * HY + (ly + 1);
      const uint32_t mine = *q;
      const uint64_t kc = lake_key(*p);
      // the cell's lowest pass (K(w), n): neighbours in ascending cell index, so of equal heights the first one stays
      uint64_t best = 0ull;
      uint32_t bn = SPILL_NONE;
      bool any = false;
      for (int dx = -1; dx <= 1; dx++)
        for (int dy = -1; dy <= 1; dy++) {
          const uint32_t lab = q[dx * HY + dy];
          if (lab == SPILL_NONE || lab == mine) continue;   // (off the map, the cell itself or a cell of its own basin)
          const uint64_t kn = lake_key(p[dx * HY + dy]), kw = kn > kc ? kn : kc;
          if (!any || kw < best) { best = kw; bn = c + (uint32_t)(dx * m.dimy + dy); any = true; }   // (unsigned: a cell index may pass 2^31)
        }
      const bool border = x == 0 || y == 0 || x == m.dimx - 1 || y == m.dimy - 1;
      if (border && (!any || kc < best)) { best = kc; bn = SPILL_NONE; any = true; }   // (at an equal height an in-map neighbour stays)
      if (PHASE == 0) {
        H[a] = *p;
        R[a] = any ? 1u : 0u;
        // the terminal of the basin: where the prefix sum of the terminal marks steps
        const bool term = (uint64_t)c + 1u == n ? B[a] - before + 1u == m.cap : B[a + 1] != B[a];
        if (term) {   // (its only writer)
          acc[m.rec0 + mine].first_cell = c;
          acc[m.rec0 + mine].flags = m.cells[c].type == AIR ? SPILL_F_LAKE : 0u;
        }
      }
      if (!any) continue;
      uint64_t v = best;
      if (PHASE == 1) {
        if (best != acc[m.rec0 + mine].kw) continue;   // (complete: the launch before)
        v = ((uint64_t)c << 32) | (uint64_t)bn;
      }
      uint32_t s = (mine * 2654435761u) % (uint32_t)PS;
      for (;;) {   // (at most TX * TY keys are ever inserted: a free or matching slot exists)
        const uint32_t k = SMX_LAKE_CAS(t.key + s, LAKE_DRY, mine, SMX_LAKE_WG);
        if (k == LAKE_DRY || k == mine) break;
        s = s + 1u == (uint32_t)PS ? 0u : s + 1u;
      }
      SMX_LAKE_MIN(t.v + s, v, SMX_LAKE_WG);
    }
  }
  g.barrier();
  for (uint32_t l = g.lo(); l < g.hi(); l++)
    for (uint32_t s = l; s < (uint32_t)PS; s += nl) {
      if (t.key[s] == LAKE_DRY) continue;
      SpillAcc& r = acc[m.rec0 + t.key[s]];
      SMX_LAKE_MIN(PHASE == 0 ? &r.kw : &r.cn, t.v[s], SMX_LAKE_AGENT);
    }
}

// ---- list: workgroup `block` takes g.lanes() cells ----
template <class G>
SMX_D void spill_list_group(const LakeMember& m, G& g, uint32_t block, const uint32_t* B, const uint32_t* R, uint32_t* Q) {
  const uint32_t nl = g.lanes();
  const uint64_t n = (uint64_t)m.dimx * (uint64_t)m.dimy;
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    const uint64_t c = (uint64_t)block * nl + l;
    if (c >= n) continue;
    const size_t a = (size_t)m.off + (size_t)c;
    if (R[a]) Q[B[a]] = (uint32_t)a;   // (B[a] < the number of cells of the call: Q has a word for each)
  }
}

// ---- point: workgroup `block` takes g.lanes() basins ----
template <class G>
SMX_D void spill_point_group(const LakeMember& m, G& g, uint32_t block, const uint32_t* T, SpillAcc* acc) {
  const uint32_t nl = g.lanes();
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    const uint64_t r = (uint64_t)block * nl + l;
    if (r >= m.cap) continue;
    const uint32_t to = (uint32_t)acc[m.rec0 + r].cn;   // (a basin without a pass does not exist; its identity reads "off the map")
    acc[m.rec0 + r].to_basin = to == SPILL_NONE ? SPILL_NONE : acc[m.rec0 + T[(size_t)m.off + to]].first_cell;
  }
}

// ---- relax: sweep `sweep` (counted from 1); workgroup `block` of `nblocks` strides over the member's boundary cells. Every access
//      to a level is an agent-scope atomic: other workgroups lower it meanwhile, and any value it ever held is a valid bound. ----
template <class G>
SMX_D void spill_relax_group(const LakeMember& m, G& g, uint32_t block, uint32_t nblocks, uint32_t sweep, const uint32_t* T, const uint32_t* B, const uint32_t* R,
                             const uint32_t* Q, const double* H, SpillAcc* acc, uint32_t* changed) {
  const uint32_t nl = g.lanes();
  uint32_t first, count;
  spill_list_span(m, B, R, first, count);
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    for (uint64_t i = (uint64_t)block * nl + l; i < count; i += (uint64_t)nblocks * nl) {
      const uint32_t a = Q[(size_t)first + (size_t)i], c = a - m.off;
      const int x = (int)(c / (uint32_t)m.dimy), y = (int)(c % (uint32_t)m.dimy);
      const uint32_t mine = T[a];
      const uint64_t kc = lake_key(H[a]);
      SpillAcc& r = acc[m.rec0 + mine];
      // every pass of this cell is at least as high as the cell: once the level is down to h(c) the cell has nothing to add, ever
      if (!(kc < SMX_LAKE_LD(&r.level, SMX_LAKE_AGENT))) continue;
      uint64_t cand = 0ull;
      bool any = false;
      for (int dx = -1; dx <= 1; dx++)
        for (int dy = -1; dy <= 1; dy++) {
          const int u = x + dx, v = y + dy;
          if ((dx == 0 && dy == 0) || u < 0 || v < 0 || u >= m.dimx || v >= m.dimy) continue;
          const size_t b = (size_t)m.off + (size_t)u * m.dimy + v;
          const uint32_t lab = T[b];
          if (lab == mine) continue;
          const uint64_t kn = lake_key(H[b]), kw = kn > kc ? kn : kc;
          const uint64_t lv = SMX_LAKE_LD(&acc[m.rec0 + lab].level, SMX_LAKE_AGENT), k = lv > kw ? lv : kw;
          if (!any || k < cand) { cand = k; any = true; }
        }
      if ((x == 0 || y == 0 || x == m.dimx - 1 || y == m.dimy - 1) && (!any || kc < cand)) { cand = kc; any = true; }
      if (!any) continue;   // (not a boundary cell: the list holds none)
      if (!(cand < SMX_LAKE_LD(&r.level, SMX_LAKE_AGENT))) continue;
      if (!(cand < SMX_LAKE_MIN(&r.level, cand, SMX_LAKE_AGENT))) continue;   // (somebody else got as low first)
      if (SMX_LAKE_MAX(&r.stamp, sweep, SMX_LAKE_AGENT) < sweep) SMX_LAKE_ADD(changed, 1u, SMX_LAKE_AGENT);   // the basin's first lowering of this sweep
    }
  }
}

// ---- store: workgroup `block` takes (SLOTS / lanes) * lanes cells; the LDS table has a slot for every one of them ----
template <int SLOTS>
struct SpillStoreTable {
  uint64_t storage[SLOTS], fill[SLOTS];
  uint32_t key[SLOTS], below[SLOTS], flags[SLOTS];
};

template <int SLOTS, class G>
SMX_D void spill_store_group(const LakeMember& m, G& g, uint32_t block, SpillStoreTable<SLOTS>& t, const uint32_t* T, double* H, SpillAcc* acc, bool filled) {
  const uint32_t nl = g.lanes(), items = (uint32_t)SLOTS / nl;
  const uint64_t n = (uint64_t)m.dimx * (uint64_t)m.dimy, c0 = (uint64_t)block * items * nl;
  for (uint32_t l = g.lo(); l < g.hi(); l++)
    for (uint32_t s = l; s < (uint32_t)SLOTS; s += nl) { t.key[s] = LAKE_DRY; t.storage[s] = 0ull; t.fill[s] = 0ull; t.below[s] = 0u; t.flags[s] = 0u; }
  g.barrier();
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    for (uint32_t it = 0; it < items; it++) {
      const uint64_t c = c0 + (uint64_t)it * nl + l;
      if (c >= n) break;
      const size_t a = (size_t)m.off + (size_t)c;
      const uint32_t mine = T[a];
      const double h = H[a];   // (only this lane reads or writes H[a] in this launch)
      const uint64_t kh = lake_key(h), kp = acc[m.rec0 + mine].kw, kl = acc[m.rec0 + mine].level;   // (both final: the launches before)
      if (!(kh < kl)) continue;   // (kl >= kp: a cell at or above the fill level is at or above the pour height)
      uint32_t f = 0u;
      const double lv = lake_unkey(kl);
      const uint64_t q2 = spill_q40(lv - h, f, SPILL_F_FILL_STORAGE);
      const bool below = kh < kp;
      const uint64_t q1 = below ? spill_q40(lake_unkey(kp) - h, f, SPILL_F_STORAGE) : 0ull;
      if (filled) H[a] = lv;
      uint32_t s = (mine * 2654435761u) % (uint32_t)SLOTS;
      for (;;) {   // (at most SLOTS keys are ever inserted: a free or matching slot exists)
        const uint32_t k = SMX_LAKE_CAS(t.key + s, LAKE_DRY, mine, SMX_LAKE_WG);
        if (k == LAKE_DRY || k == mine) break;
        s = s + 1u == (uint32_t)SLOTS ? 0u : s + 1u;
      }
      if (below) SMX_LAKE_ADD(t.below + s, 1u, SMX_LAKE_WG);
      if (q1) { const uint64_t o = SMX_LAKE_ADD(t.storage + s, q1, SMX_LAKE_WG); if (o + q1 < o) f |= SPILL_F_STORAGE; }
      if (q2) { const uint64_t o = SMX_LAKE_ADD(t.fill + s, q2, SMX_LAKE_WG); if (o + q2 < o) f |= SPILL_F_FILL_STORAGE; }
      if (f) SMX_LAKE_OR(t.flags + s, f, SMX_LAKE_WG);
    }
  }
  g.barrier();
  for (uint32_t l = g.lo(); l < g.hi(); l++)
    for (uint32_t s = l; s < (uint32_t)SLOTS; s += nl) {
      if (t.key[s] == LAKE_DRY) continue;
      SpillAcc& r = acc[m.rec0 + t.key[s]];
      uint32_t f = t.flags[s];
      if (t.below[s]) SMX_LAKE_ADD(&r.cells_below, t.below[s], SMX_LAKE_AGENT);
      if (t.storage[s]) { const uint64_t v = t.storage[s], o = SMX_LAKE_ADD(&r.storage, v, SMX_LAKE_AGENT); if (o + v < o) f |= SPILL_F_STORAGE; }
      if (t.fill[s]) { const uint64_t v = t.fill[s], o = SMX_LAKE_ADD(&r.fill_storage, v, SMX_LAKE_AGENT); if (o + v < o) f |= SPILL_F_FILL_STORAGE; }
      if (f) SMX_LAKE_OR(&r.flags, f, SMX_LAKE_AGENT);
    }
}

}  // namespace smx
