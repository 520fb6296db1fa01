// soil_through.h -- through-drainage (smx_through / smx_ensemble_through): one cycle-free outflow per basin, the forest of basins it
// makes, what drains THROUGH every basin and every cell once the pits and lakes are full. The bodies of k_through_init,
// k_through_count, k_through_hops, k_through_exit, k_through_link, k_through_accumulate, k_through_outlet, k_through_plane and
// k_through_area. Nothing here writes a map.
//
// Cells, h, K, wet cells, basins, first_cell, the rank, the passes (c, n), w and the fill level L(a) are those of soil_drain.h and
// soil_spill.h. A pass (c, n) of basin a is TIGHT when K(max(w, L(basin(n)))) == K(L(a)), the off-map pass when K(w) == K(L(a)):
// the first pass of a minimax route is tight, so every basin has one. hops(a) = 1 where a has a tight off-map pass, else 1 + the
// smallest hops over the targets of its tight in-map passes. The EXIT of a is the tight pass with the smallest (c, n) among those
// whose target has hops(a) - 1, off the map counting as 0: down(a) = basin(exit_to). hops strictly falls along down: the basins
// form a forest whose roots exit off the map. (Following the POUR POINTS instead loops wherever two basins share their lowest pass.)
// through_cells(a) = cells(a) + the through_cells of the basins whose down is a; upstream_basins(a) the number of basins above a;
// outlet(a) the root below a. through_area(c) = 1 + the through_area of c's donors + the through_cells of the basins whose exit_to
// is c: inside a basin the paths are the drainage's own, a basin's total arrives at its terminal and re-appears at the entry cell
// of the next basin.
//
// The planes are the spill chain's: T the rank, B the prefix sum of the boundary marks, Q the boundary cells, H h(c); M takes the
// boundary marks (soil_spill.h calls it R), so that R stays the drainage's receivers for the area walk. P and AR are the drainage's.
// The basins' tables: SpillAcc (first_cell, the lake bit, the pour point, K(L)) and ThroughAcc, one record each per basin of every
// member. The steps behind the spill chain's sweeps, each one launch for all members (blockIdx.y = member):
//   init        the ThroughAcc records become the identities.
//   count       cells(a): every cell adds 1 to its basin, combined per workgroup in an LDS table as in k_drain_stats.
//   hops        ONE SWEEP over Q: a cell above its basin's level leaves at once; for each tight pass fetch_min(hops[a],
//               hops[basin(n)] + 1), 1 off the map; a target that has no count yet is skipped. Monotone and in place, as k_spill_relax.
//   exit        one pass over Q: the smallest (c << 32 | n) per basin among the tight passes whose target has hops - 1.
//   link        PHASE 0, one lane per basin: down, the exit's height and the flags; through_cells = cells; 1 added to down's pending
//               word. PHASE 1: a basin nobody reported to gets the LEAF mark (its word is final only behind phase 0's launch).
//   accumulate  the never-waiting walk of k_drain_area over the basins: the lane owning a leaf adds through_cells and
//               upstream_basins + 1 to down and release-decrements down's pending word; only the lane whose decrement is the last
//               acquires and carries on. Before it leaves a completed basin it adds the basin's through_cells to AR[exit_to].
//   outlet      each basin walks down for hops - 1 steps.      plane   outlets(c) = the outlet's rank, from T.
//   area        k_drain_area's walk over the injected AR. A leaf CELL starts from its own AR, not from 1: an entry cell is as often
//               as not a cell nobody drains into, and what was injected there must travel on.
// No lane waits for another, nothing spins. The file compiles for the device and, under SMX_D / SMX_HOSTSIM, for the host
// (tests/through_host), as soil_spill.h does.
#pragma once
#include "soil_spill.h"

namespace smx {

constexpr uint32_t THROUGH_NONE = 0xFFFFFFFFu;   // exit_to / down: off the map; hops: no count yet
constexpr uint32_t THROUGH_LEAF = 0xFFFFFFFFu;   // pend: a basin no basin exits into (nobody ever decrements it)
constexpr uint32_t THROUGH_F_LAKE = 1u, THROUGH_F_OFFMAP = 2u, THROUGH_F_NOT_POUR = 4u, THROUGH_F_WET_ENTRY = 8u;

struct ThroughAcc {   // a basin while the forest is built (64 bytes)
  uint64_t cn;                       // the exit: (c << 32 | n)
  uint64_t kw;                       // K(w) of the exit
  uint32_t hops, down, down_first;   // down: the RANK of basin(exit_to); down_first: its first_cell
  uint32_t pend;                     // upstream neighbours still to report, THROUGH_LEAF
  uint32_t cells, through_cells, upstream;
  uint32_t outlet, outlet_first, outlet_cell;   // outlet: the root's RANK
  uint32_t flags, pad;
};
struct ThroughRec {   // == smx_through_record (include/soilmx.h)
  uint32_t first_cell, exit_cell, exit_to, down;
  uint32_t outlet, outlet_cell, hops, flags;
  uint32_t cells, through_cells, upstream_basins, reserved;
  double exit_height, fill_height;
};
static_assert(sizeof(ThroughAcc) == 64 && sizeof(ThroughRec) == 64, "through record layouts");

SMX_HD void through_finish(const SpillAcc& s, const ThroughAcc& a, ThroughRec& r) {
  r.first_cell = s.first_cell; r.exit_cell = (uint32_t)(a.cn >> 32); r.exit_to = (uint32_t)a.cn; r.down = a.down_first;
  r.outlet = a.outlet_first; r.outlet_cell = a.outlet_cell; r.hops = a.hops; r.flags = a.flags;
  r.cells = a.cells; r.through_cells = a.through_cells; r.upstream_basins = a.upstream; r.reserved = 0u;
  r.exit_height = lake_unkey(a.kw); r.fill_height = lake_unkey(s.level);
}

// ---- init: workgroup `block` takes g.lanes() records of member m ----
template <class G>
SMX_D void through_init_group(const LakeMember& m, G& g, uint32_t block, ThroughAcc* acc) {
  const uint32_t nl = g.lanes();
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    const uint64_t r = (uint64_t)block * nl + l;
    if (r >= m.cap) continue;
    ThroughAcc z;
    z.cn = ~0ull; z.kw = 0ull; z.hops = THROUGH_NONE; z.down = THROUGH_NONE; z.down_first = THROUGH_NONE; z.pend = 0u;
    z.cells = 0u; z.through_cells = 0u; z.upstream = 0u; z.outlet = THROUGH_NONE; z.outlet_first = THROUGH_NONE; z.outlet_cell = THROUGH_NONE;
    z.flags = 0u; z.pad = 0u;
    acc[m.rec0 + r] = z;
  }
}

// ---- count: workgroup `block` takes (SLOTS / lanes) * lanes cells; the LDS table has a slot for every one of them ----
template <int SLOTS>
struct ThroughCountTable {
  uint32_t key[SLOTS], cells[SLOTS];
};

template <int SLOTS, class G>
SMX_D void through_count_group(const LakeMember& m, G& g, uint32_t block, ThroughCountTable<SLOTS>& t, const uint32_t* T, ThroughAcc* acc) {
  const uint32_t nl = g.lanes(), items = (uint32_t)SLOTS / nl;
  const uint64_t n = (uint64_t)m.dimx * (uint64_t)m.dimy, c0 = (uint64_t)block * items * nl;
  for (uint32_t l = g.lo(); l < g.hi(); l++)
    for (uint32_t s = l; s < (uint32_t)SLOTS; s += nl) { t.key[s] = LAKE_DRY; t.cells[s] = 0u; }
  g.barrier();
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    for (uint32_t it = 0; it < items; it++) {
      const uint64_t c = c0 + (uint64_t)it * nl + l;
      if (c >= n) break;
      const uint32_t mine = T[(size_t)m.off + (size_t)c];
      uint32_t s = (mine * 2654435761u) % (uint32_t)SLOTS;
      for (;;) {   // (at most SLOTS keys are ever inserted: a free or matching slot exists)
        const uint32_t k = SMX_LAKE_CAS(t.key + s, LAKE_DRY, mine, SMX_LAKE_WG);
        if (k == LAKE_DRY || k == mine) break;
        s = s + 1u == (uint32_t)SLOTS ? 0u : s + 1u;
      }
      SMX_LAKE_ADD(t.cells + s, 1u, SMX_LAKE_WG);
    }
  }
  g.barrier();
  for (uint32_t l = g.lo(); l < g.hi(); l++)
    for (uint32_t s = l; s < (uint32_t)SLOTS; s += nl) {
      if (t.key[s] == LAKE_DRY) continue;
      SMX_LAKE_ADD(&acc[m.rec0 + t.key[s]].cells, t.cells[s], SMX_LAKE_AGENT);
    }
}

// ---- hops: one sweep; workgroup `block` of `nblocks` strides over the member's boundary cells (M: the boundary marks). The levels
//      are final (the launches before); every access to a hop count is an agent-scope atomic: other workgroups lower it meanwhile,
//      and any value it ever held is the length of a tight route. ----
template <class G>
SMX_D void through_hops_group(const LakeMember& m, G& g, uint32_t block, uint32_t nblocks, const uint32_t* T, const uint32_t* B, const uint32_t* M,
                              const uint32_t* Q, const double* H, const SpillAcc* sacc, ThroughAcc* acc, uint32_t* changed) {
  const uint32_t nl = g.lanes();
  uint32_t first, count;
  spill_list_span(m, B, M, first, count);
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    for (uint64_t i = (uint64_t)block * nl + l; i < count; i += (uint64_t)nblocks * nl) {
      const uint32_t a = Q[(size_t)first + (size_t)i], c = a - m.off;
      const int x = (int)(c / (uint32_t)m.dimy), y = (int)(c % (uint32_t)m.dimy);
      const uint32_t mine = T[a];
      const uint64_t kc = lake_key(H[a]), lv = sacc[m.rec0 + mine].level;
      if (kc > lv) continue;   // every pass of this cell is at least as high as the cell: none is tight
      uint32_t* mh = &acc[m.rec0 + mine].hops;
      const uint32_t had = SMX_LAKE_LD(mh, SMX_LAKE_AGENT);
      uint32_t best = had;
      if (kc == lv && (x == 0 || y == 0 || x == m.dimx - 1 || y == m.dimy - 1)) best = 1u;   // the tight off-map pass
      for (int dx = -1; dx <= 1 && best > 1u; dx++)
        for (int dy = -1; dy <= 1; dy++) {
          const int u = x + dx, v = y + dy;
          if ((dx == 0 && dy == 0) || u < 0 || v < 0 || u >= m.dimx || v >= m.dimy) continue;
          const size_t b = (size_t)m.off + (size_t)u * m.dimy + v;
          const uint32_t lab = T[b];
          if (lab == mine) continue;
          const uint64_t kn = lake_key(H[b]), kw = kn > kc ? kn : kc, ln = sacc[m.rec0 + lab].level;
          if ((ln > kw ? ln : kw) != lv) continue;   // not tight
          const uint32_t th = SMX_LAKE_LD(&acc[m.rec0 + lab].hops, SMX_LAKE_AGENT);
          if (th != THROUGH_NONE && th + 1u < best) best = th + 1u;
        }
      if (!(best < had)) continue;
      if (!(best < SMX_LAKE_MIN(mh, best, SMX_LAKE_AGENT))) continue;   // (somebody else got as low first)
      if (SMX_LAKE_LD(changed, SMX_LAKE_AGENT) == 0u) SMX_LAKE_ADD(changed, 1u, SMX_LAKE_AGENT);   // (zero or not is all the host asks)
    }
  }
}

// ---- exit: one pass over the boundary cells; the hop counts are final ----
template <class G>
SMX_D void through_exit_group(const LakeMember& m, G& g, uint32_t block, uint32_t nblocks, const uint32_t* T, const uint32_t* B, const uint32_t* M,
                              const uint32_t* Q, const double* H, const SpillAcc* sacc, ThroughAcc* acc) {
  const uint32_t nl = g.lanes();
  uint32_t first, count;
  spill_list_span(m, B, M, first, count);
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    for (uint64_t i = (uint64_t)block * nl + l; i < count; i += (uint64_t)nblocks * nl) {
      const uint32_t a = Q[(size_t)first + (size_t)i], c = a - m.off;
      const int x = (int)(c / (uint32_t)m.dimy), y = (int)(c % (uint32_t)m.dimy);
      const uint32_t mine = T[a];
      const uint64_t kc = lake_key(H[a]), lv = sacc[m.rec0 + mine].level;
      if (kc > lv) continue;
      ThroughAcc& r = acc[m.rec0 + mine];
      const uint32_t want = r.hops - 1u;   // (a basin without a count does not exist behind the sweeps)
      uint64_t best = ~0ull;               // the cell's own smallest qualifying (c, n): n ascends, the off-map side is the largest
      for (int dx = -1; dx <= 1 && best == ~0ull && want != 0u; dx++)
        for (int dy = -1; dy <= 1; dy++) {
          const int u = x + dx, v = y + dy;
          if ((dx == 0 && dy == 0) || u < 0 || v < 0 || u >= m.dimx || v >= m.dimy) continue;
          const size_t b = (size_t)m.off + (size_t)u * m.dimy + v;
          const uint32_t lab = T[b];
          if (lab == mine) continue;
          const uint64_t kn = lake_key(H[b]), kw = kn > kc ? kn : kc, ln = sacc[m.rec0 + lab].level;
          if ((ln > kw ? ln : kw) != lv || acc[m.rec0 + lab].hops != want) continue;
          best = ((uint64_t)c << 32) | (uint64_t)(b - m.off);
          break;
        }
      if (want == 0u && kc == lv && (x == 0 || y == 0 || x == m.dimx - 1 || y == m.dimy - 1)) best = ((uint64_t)c << 32) | (uint64_t)THROUGH_NONE;
      if (best == ~0ull) continue;
      if (!(best < SMX_LAKE_LD(&r.cn, SMX_LAKE_AGENT))) continue;   // only an improving lane issues the atomic
      SMX_LAKE_MIN(&r.cn, best, SMX_LAKE_AGENT);
    }
  }
}

// ---- link: workgroup `block` takes g.lanes() basins. PHASE 0 resolves and counts, PHASE 1 marks the leaves ----
template <int PHASE, class G>
SMX_D void through_link_group(const LakeMember& m, G& g, uint32_t block, const uint32_t* T, const double* H, const SpillAcc* sacc, ThroughAcc* acc) {
  const uint32_t nl = g.lanes();
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    const uint64_t k = (uint64_t)block * nl + l;
    if (k >= m.cap) continue;
    ThroughAcc& r = acc[m.rec0 + k];
    if (PHASE == 1) {   // (pend is complete: the launch before; only this lane touches it here)
      if (r.pend == 0u) r.pend = THROUGH_LEAF;
      continue;
    }
    const SpillAcc& s = sacc[m.rec0 + k];
    r.through_cells = r.cells;
    if (r.cn == ~0ull) continue;   // (cannot happen: every basin has a tight pass towards hops - 1; no cell index is read from the identity)
    const uint32_t c = (uint32_t)(r.cn >> 32), to = (uint32_t)r.cn;
    const uint64_t kc = lake_key(H[(size_t)m.off + c]);
    uint32_t f = s.flags & SPILL_F_LAKE ? THROUGH_F_LAKE : 0u;
    if (r.cn != s.cn) f |= THROUGH_F_NOT_POUR;
    if (to == THROUGH_NONE) {
      r.kw = kc; r.flags = f | THROUGH_F_OFFMAP;   // (down and down_first stay THROUGH_NONE)
      continue;
    }
    const uint64_t kn = lake_key(H[(size_t)m.off + to]);
    const uint32_t d = T[(size_t)m.off + to];
    r.kw = kn > kc ? kn : kc;
    r.down = d; r.down_first = sacc[m.rec0 + d].first_cell;
    r.flags = f | (m.cells[to].type == AIR ? THROUGH_F_WET_ENTRY : 0u);
    SMX_LAKE_ADD(&acc[m.rec0 + d].pend, 1u, SMX_LAKE_AGENT);
  }
}

// ---- accumulate: workgroup `block` takes g.lanes() basins; every access to a pending word, to a sum another lane adds to and to AR
//      is an agent-scope atomic. AR null: records only, nothing is injected. ----
template <class G>
SMX_D void through_accumulate_group(const LakeMember& m, G& g, uint32_t block, ThroughAcc* acc, uint32_t* AR) {
  const uint32_t nl = g.lanes();
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    const uint64_t k = (uint64_t)block * nl + l;
    if (k >= m.cap) continue;
    uint32_t cur = (uint32_t)k;
    if (SMX_LAKE_LD(&acc[m.rec0 + cur].pend, SMX_LAKE_AGENT) != THROUGH_LEAF) continue;   // (a leaf's word never changes)
    uint32_t tc = acc[m.rec0 + cur].cells, ub = 0u;                                       // (... and nobody adds to its sums)
    // Every turn moves cur to down(cur), one step down a chain along which hops strictly falls: the walk ends at a root or earlier,
    // where another upstream basin is still to report. It never waits: the lane whose decrement is the last one goes on.
    for (;;) {
      const ThroughAcc& r = acc[m.rec0 + cur];
      const uint32_t to = (uint32_t)r.cn, d = r.down;   // (written by the launches before)
      if (d == THROUGH_NONE) break;                     // a root: it exits off the map
      if (AR) SMX_LAKE_ADD(AR + m.off + to, tc, SMX_LAKE_AGENT);   // cur is complete: its total re-appears at the entry cell
      ThroughAcc& n = acc[m.rec0 + d];
      SMX_LAKE_ADD(&n.through_cells, tc, SMX_LAKE_AGENT);
      SMX_LAKE_ADD(&n.upstream, ub + 1u, SMX_LAKE_AGENT);
      if (SMX_DRAIN_DEC_RELEASE(&n.pend) != 1u) break;   // an upstream basin of d is still to come
      SMX_DRAIN_ACQUIRE();                               // every one's adds happened before its decrement: d's sums are complete
      tc = SMX_LAKE_LD(&n.through_cells, SMX_LAKE_AGENT);
      ub = SMX_LAKE_LD(&n.upstream, SMX_LAKE_AGENT);
      cur = d;
    }
  }
}

// ---- outlet: workgroup `block` takes g.lanes() basins; each walks down for hops - 1 steps ----
template <class G>
SMX_D void through_outlet_group(const LakeMember& m, G& g, uint32_t block, const SpillAcc* sacc, ThroughAcc* acc) {
  const uint32_t nl = g.lanes();
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    const uint64_t k = (uint64_t)block * nl + l;
    if (k >= m.cap) continue;
    uint32_t cur = (uint32_t)k;
    for (uint32_t i = acc[m.rec0 + k].hops; i > 1u; i--) {   // (hops and down: the launches before; this launch writes the outlet words only)
      const uint32_t d = acc[m.rec0 + cur].down;
      if (d == THROUGH_NONE) break;                           // (cannot happen: hops(down) = hops - 1)
      cur = d;
    }
    ThroughAcc& r = acc[m.rec0 + k];
    r.outlet = cur; r.outlet_first = sacc[m.rec0 + cur].first_cell; r.outlet_cell = (uint32_t)(acc[m.rec0 + cur].cn >> 32);
  }
}

// ---- plane: workgroup `block` takes g.lanes() cells: O[a] = the rank of the outlet of the cell's basin ----
template <class G>
SMX_D void through_plane_group(const LakeMember& m, G& g, uint32_t block, const uint32_t* T, const ThroughAcc* acc, uint32_t* O) {
  const uint32_t nl = g.lanes();
  const uint64_t n = (uint64_t)m.dimx * (uint64_t)m.dimy;
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    const uint64_t c = (uint64_t)block * nl + l;
    if (c >= n) continue;
    const size_t a = (size_t)m.off + (size_t)c;
    O[a] = acc[m.rec0 + T[a]].outlet;
  }
}

// ---- area: drain_area_group over the injected AR; a leaf starts from what its own word holds ----
template <class G>
SMX_D void through_area_group(const LakeMember& m, G& g, uint32_t block, const uint32_t* R, uint32_t* P, uint32_t* AR) {
  const uint32_t nl = g.lanes();
  const uint64_t n = (uint64_t)m.dimx * (uint64_t)m.dimy;
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    const uint64_t c = (uint64_t)block * nl + l;
    if (c >= n) continue;
    uint32_t cur = m.off + (uint32_t)c;
    if (SMX_LAKE_LD(P + cur, SMX_LAKE_AGENT) != DRAIN_LEAF) continue;   // (a leaf's P never changes)
    uint32_t area = SMX_LAKE_LD(AR + cur, SMX_LAKE_AGENT);              // 1 + what the launches before injected; nobody adds to it here
    for (;;) {   // (the walk of drain_area_group)
      const uint32_t r = R[cur];
      if (r == DRAIN_NONE) break;
      SMX_LAKE_ADD(AR + r, area, SMX_LAKE_AGENT);
      if (SMX_DRAIN_DEC_RELEASE(P + r) != 1u) break;
      SMX_DRAIN_ACQUIRE();
      area = SMX_LAKE_LD(AR + r, SMX_LAKE_AGENT);
      cur = r;
    }
  }
}

}  // namespace smx
