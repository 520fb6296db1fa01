// soil_hills.h -- the hillslopes (smx_hillslopes / smx_ensemble_hillslopes): where every dry cell enters the channel network, how far
// it is from there and how high it stands above it (HAND), and one record per segment of the lateral land that drains into it. The
// bodies of k_hill_init, k_hill_jump and k_hill_fold. Nothing here writes a map.
//
// Cells, h(c), wet cells, receivers and sinks are those of soil_drain.h; channel cells, segments and their ranks those of
// soil_streams.h with the same threshold. For a dry cell c the ENTRY e(c) is the first cell on c, R(c), R(R(c)), ... (c included) that
// is a channel cell, a sink or a wet cell; straight(c) / diagonal(c) count the steps to it, hand(c) = h(c) - h(e(c)) in one f64
// subtraction (+0.0 where e(c) == c), hillslope(c) the rank of the segment e(c) lies on, HILL_NONE where e(c) is no channel cell. A wet
// cell has no entry: HILL_NONE twice, no steps, hand +0.0. Every dry cell before the entry is off the channels, so its area is below
// threshold, and the area is at least the number of cells upstream: a path has at most min(threshold, cells) - 1 steps.
//
// The planes are read as the streams chain left them with the segments plane complete (k_stream_segments with_plane): SG the
// segment's rank per channel cell, D the channel donors, B the scan of the start marks, R the receivers. Two sets of three u32 planes
// (J the jump pointer, a plane index; S, G the straight and diagonal steps to it) are written in turns:
//   init   J[c] = c for an entry -- a channel cell, a wet cell or a sink -- with no step; else J[c] = R[c] with that one step in S or
//          G. One lane per cell, its own words only, so J may take R's plane. The same workgroups set the member's records to the
//          fold's identities.
//   jump   one round of pointer doubling from one set to the other: with j = J[c], a settled j (J[j] == j) is copied, else
//          J' = J[j], S' = S[c] + S[j], G' = G[c] + G[j]. A round reads one set and writes the other: the three values of a cell
//          always belong together, no atomics, no waiting, and nothing depends on which workgroup runs first. After k rounds a cell
//          points min(2^k, its path's length) steps down: the caller queues the smallest k with 2^k >= the path bound.
//   fold   each cell reads its settled (e, s, g), writes the planes asked for and, where it is a dry off-channel cell whose entry lies
//          on a segment of rank < cap, folds its figures per rank in an LDS table; then ONE set of atomics per segment and workgroup
//          goes to the record. Integer adds and order-free extremes only: nothing depends on the order of the contributions.
// The file compiles for the device and, under SMX_D / SMX_HOSTSIM, for the host (tests/hillslopes_host), as soil_streams.h does.
#pragma once
#include "soil_streams.h"

namespace smx {

constexpr uint32_t HILL_NONE = 0xFFFFFFFFu;   // entry, hillslope: a wet cell; hillslope: the entry is no channel cell; farthest_cell: no cell
constexpr uint32_t HILL_F_HAND = 1u;          // hand_sum_q40 unreliable

struct HillAcc {      // a record while it is folded (64 bytes, as smx_hillslope): steps_max and farthest_cell as one ordered word
  uint32_t first_cell, cells;
  uint64_t far;       // (steps << 32) | (0xFFFFFFFF - cell): its maximum is the largest steps and, among those, the smallest cell
  uint64_t straight_sum, diagonal_sum;
  uint64_t hmax;      // the ordered image of hand_max
  uint64_t hand_sum_q40;
  uint32_t bank_cells, head_cells, flags, pad;
};
struct HillRec {      // == smx_hillslope (include/soilmx.h)
  uint32_t first_cell, cells, steps_max, farthest_cell;
  uint64_t straight_sum, diagonal_sum;
  double hand_max;
  uint64_t hand_sum_q40;
  uint32_t bank_cells, head_cells, flags, reserved;
};
static_assert(sizeof(HillAcc) == 64 && sizeof(HillRec) == 64, "hillslope record layouts");

SMX_HD void hill_finish(const HillAcc& a, HillRec& r) {
  r.first_cell = a.first_cell; r.cells = a.cells;
  r.steps_max = (uint32_t)(a.far >> 32); r.farthest_cell = 0xFFFFFFFFu - (uint32_t)a.far;   // (far == 0 without a cell: 0 steps, HILL_NONE)
  r.straight_sum = a.straight_sum; r.diagonal_sum = a.diagonal_sum;
  r.hand_max = a.cells ? lake_unkey(a.hmax) : 0.0;
  r.hand_sum_q40 = a.hand_sum_q40;
  r.bank_cells = a.bank_cells; r.head_cells = a.head_cells; r.flags = a.flags; r.reserved = 0u;
}
// rounds of hill_jump for paths of at most `bound` steps: the smallest k with 2^k >= bound, 0 for a bound of 0 or 1
SMX_HD uint32_t hill_rounds(uint64_t bound) {
  uint32_t k = 0u;
  while (((uint64_t)1 << k) < bound) k++;
  return k;
}
// the path bound of a call: min(threshold, the cells of its largest map) - 1
SMX_HD uint64_t hill_bound(uint32_t threshold, uint64_t cells) { return (threshold < cells ? (uint64_t)threshold : cells) - 1u; }

// ---- init: workgroup `block` of `nblocks` takes g.lanes() cells; J is R's plane, read and written by the cell's own lane only ----
template <class G>
SMX_D void hill_init_group(const LakeMember& m, G& g, uint32_t block, uint32_t nblocks, const uint32_t* SG, uint32_t* J, uint32_t* S, uint32_t* Gd, HillAcc* acc) {
  const uint32_t nl = g.lanes(), dimy = (uint32_t)m.dimy;
  const uint64_t n = (uint64_t)m.dimx * (uint64_t)m.dimy;
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    for (uint64_t r = (uint64_t)block * nl + l; r < m.cap; r += (uint64_t)nblocks * nl) {   // the member's records: the identities of the fold
      HillAcc z;
      z.first_cell = 0u; z.cells = 0u; z.far = 0ull; z.straight_sum = 0ull; z.diagonal_sum = 0ull; z.hmax = 0ull; z.hand_sum_q40 = 0ull;
      z.bank_cells = 0u; z.head_cells = 0u; z.flags = 0u; z.pad = 0u;
      acc[m.rec0 + r] = z;
    }
    const uint64_t c = (uint64_t)block * nl + l;
    if (c >= n) continue;
    const uint32_t a = m.off + (uint32_t)c;
    const uint32_t r = J[a];   // (the receiver: DRAIN_NONE for a sink and for a wet cell)
    if (SG[a] != STREAM_OFF || r == DRAIN_NONE) { J[a] = a; S[a] = 0u; Gd[a] = 0u; continue; }
    const uint32_t cc = (uint32_t)c, rc = r - m.off;
    const uint32_t diag = cc / dimy != rc / dimy && cc % dimy != rc % dimy ? 1u : 0u;
    S[a] = 1u - diag; Gd[a] = diag;   // (J[a] stays the receiver)
  }
}

// ---- jump: workgroup `block` takes g.lanes() cells; reads set 0, writes set 1 ----
template <class G>
SMX_D void hill_jump_group(const LakeMember& m, G& g, uint32_t block, const uint32_t* J0, const uint32_t* S0, const uint32_t* G0, uint32_t* J1, uint32_t* S1,
                           uint32_t* G1) {
  const uint32_t nl = g.lanes();
  const uint64_t n = (uint64_t)m.dimx * (uint64_t)m.dimy;
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    const uint64_t c = (uint64_t)block * nl + l;
    if (c >= n) continue;
    const uint32_t a = m.off + (uint32_t)c;
    const uint32_t j = J0[a], jj = J0[j];   // (every pointer is a plane index of the cell's own member)
    uint32_t s = S0[a], d = G0[a];
    if (jj != j) { s += S0[j]; d += G0[j]; }
    J1[a] = jj; S1[a] = s; G1[a] = d;       // (jj == j where j is settled: a copy)
  }
}

// ---- fold: workgroup `block` takes (SLOTS / lanes) * lanes cells; the LDS table has a slot for every one of them ----
template <int SLOTS>
struct HillTable {
  uint64_t far[SLOTS], ssum[SLOTS], dsum[SLOTS], hmax[SLOTS], q40[SLOTS];
  uint32_t key[SLOTS], cells[SLOTS], bank[SLOTS], head[SLOTS], flags[SLOTS];
};

// (J, S, Gd: the settled set; entry / hillslope / hand: the planes to write, null = not asked for; m.cap: records kept for the member)
template <int SLOTS, class G>
SMX_D void hill_fold_group(const LakeMember& m, G& g, uint32_t block, HillTable<SLOTS>& t, const uint32_t* J, const uint32_t* S, const uint32_t* Gd,
                           const uint32_t* SG, const uint32_t* D, const uint32_t* B, HillAcc* acc, uint32_t* nsegments, uint32_t* entry, uint32_t* hillslope,
                           double* hand) {
  const uint32_t nl = g.lanes(), items = (uint32_t)SLOTS / nl;
  const uint64_t n = (uint64_t)m.dimx * (uint64_t)m.dimy, c0 = (uint64_t)block * items * nl;
  for (uint32_t l = g.lo(); l < g.hi(); l++)
    for (uint32_t s = l; s < (uint32_t)SLOTS; s += nl) {
      t.key[s] = HILL_NONE; t.cells[s] = 0u; t.far[s] = 0ull; t.ssum[s] = 0ull; t.dsum[s] = 0ull; t.hmax[s] = 0ull; t.q40[s] = 0ull;
      t.bank[s] = 0u; t.head[s] = 0u; t.flags[s] = 0u;
    }
  g.barrier();
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    for (uint32_t it = 0; it < items; it++) {
      const uint64_t c = c0 + (uint64_t)it * nl + l;
      if (c >= n) break;
      const size_t a = (size_t)m.off + (size_t)c;
      if (c == n - 1) *nsegments = B[a] + stream_mark(D, a) - B[m.off];
      const Sec top = m.cells[c];
      const bool wet = top.type == AIR;
      const uint32_t e = J[a];
      const uint32_t rank = wet ? HILL_NONE : SG[e];   // (STREAM_OFF == HILL_NONE where the entry is a sink or a wet cell)
      double hd = 0.0;
      if (!wet && e != (uint32_t)a) hd = drain_height(top) - drain_height(m.cells[e - m.off]);
      if (entry) entry[a] = wet ? HILL_NONE : e - m.off;
      if (hillslope) hillslope[a] = rank;
      if (hand) hand[a] = hd;
      if (stream_mark(D, a) && SG[a] < m.cap) acc[m.rec0 + SG[a]].first_cell = (uint32_t)c;   // (its only writer)
      if (wet || e == (uint32_t)a || rank >= m.cap) continue;   // (HILL_NONE is never below cap)
      const uint32_t sc = S[a], dc = Gd[a];
      uint32_t f = 0u, lf = 0u;
      const uint64_t q = lake_q40(hd, lf);
      if (lf) f |= HILL_F_HAND;
      uint32_t s = (rank * 2654435761u) % (uint32_t)SLOTS;
      for (;;) {   // (at most SLOTS keys are ever inserted: a free or matching slot exists)
        const uint32_t k = SMX_LAKE_CAS(t.key + s, HILL_NONE, rank, SMX_LAKE_WG);
        if (k == HILL_NONE || k == rank) break;
        s = s + 1u == (uint32_t)SLOTS ? 0u : s + 1u;
      }
      SMX_LAKE_ADD(t.cells + s, 1u, SMX_LAKE_WG);
      SMX_LAKE_MAX(t.far + s, ((uint64_t)(sc + dc) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)c), SMX_LAKE_WG);
      if (sc) SMX_LAKE_ADD(t.ssum + s, (uint64_t)sc, SMX_LAKE_WG);
      if (dc) SMX_LAKE_ADD(t.dsum + s, (uint64_t)dc, SMX_LAKE_WG);
      SMX_LAKE_MAX(t.hmax + s, lake_key(hd), SMX_LAKE_WG);
      if (q) { const uint64_t o = SMX_LAKE_ADD(t.q40 + s, q, SMX_LAKE_WG); if (o + q < o) f |= HILL_F_HAND; }
      if (sc + dc == 1u) SMX_LAKE_ADD(t.bank + s, 1u, SMX_LAKE_WG);
      if (stream_mark(D, e)) SMX_LAKE_ADD(t.head + s, 1u, SMX_LAKE_WG);
      if (f) SMX_LAKE_OR(t.flags + s, f, SMX_LAKE_WG);
    }
  }
  g.barrier();
  for (uint32_t l = g.lo(); l < g.hi(); l++)
    for (uint32_t s = l; s < (uint32_t)SLOTS; s += nl) {
      if (t.key[s] == HILL_NONE) continue;
      HillAcc& r = acc[m.rec0 + t.key[s]];
      uint32_t f = t.flags[s];
      SMX_LAKE_ADD(&r.cells, t.cells[s], SMX_LAKE_AGENT);
      SMX_LAKE_MAX(&r.far, t.far[s], SMX_LAKE_AGENT);
      if (t.ssum[s]) SMX_LAKE_ADD(&r.straight_sum, t.ssum[s], SMX_LAKE_AGENT);
      if (t.dsum[s]) SMX_LAKE_ADD(&r.diagonal_sum, t.dsum[s], SMX_LAKE_AGENT);
      SMX_LAKE_MAX(&r.hmax, t.hmax[s], SMX_LAKE_AGENT);
      if (t.q40[s]) { const uint64_t v = t.q40[s], o = SMX_LAKE_ADD(&r.hand_sum_q40, v, SMX_LAKE_AGENT); if (o + v < o) f |= HILL_F_HAND; }
      if (t.bank[s]) SMX_LAKE_ADD(&r.bank_cells, t.bank[s], SMX_LAKE_AGENT);
      if (t.head[s]) SMX_LAKE_ADD(&r.head_cells, t.head[s], SMX_LAKE_AGENT);
      if (f) SMX_LAKE_OR(&r.flags, f, SMX_LAKE_AGENT);
    }
}

}  // namespace smx
