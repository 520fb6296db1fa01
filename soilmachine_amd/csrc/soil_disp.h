// soil_disp.h -- dispersed flow (smx_dispersal / smx_ensemble_dispersal): the multiple-flow-direction contributing area in fixed
// point, the donors and receivers of every cell, and per basin of smx_drainage what arrives at its terminal and what leaks over its
// divides. The bodies of k_disp_pending, k_disp_flow, k_disp_fold and k_disp_peak. Nothing here writes a map.
//
// Cells, h(c), wet cells, receivers R(c), sinks, basins and their ranks are those of soil_drain.h. ONE = 2^24. The LOWER neighbours of
// a dry cell c are the in-map cells n among its eight neighbours with h(n) < h(c) (plain f64 `<`: a NaN is never lower and never has
// a lower neighbour); a dry cell with one is a GIVER, sinks and wet cells give nothing, and R(c) is always one of c's lower
// neighbours. For a lower neighbour n of c: s = (h(c) - h(n)) * k, k = 1.0 for a straight step and 0x3FE6A09E667F3BCD for a diagonal
// one; w(n) = 1.0 * s * s ... (`exponent` factors, left to right; exponent 0..16); W = 0.0 + w(n) + ... in ascending cell index;
// f(n) = (u32)((w(n) / W) * 16777216.0), truncated, where W > 0 and W is finite, else every f(n) = 0 (the products overflowed, or all
// underflowed). The f(n) sum to at most ONE. A(c), a u64, is ONE plus what c is given; a giver hands share(n) = (A(c) * f(n)) >> 24
// (a 128-bit product) to every lower neighbour and the remainder A(c) - sum of the shares to R(c) on top of its share: nothing is
// lost, and with all f = 0 the cell behaves as in D8. donors(c): the givers among c's neighbours that are higher than c (for a wet
// cell too); receivers(c): the lower neighbours of a giver, 0 for a sink and a wet cell.
//
// The planes are read as the drainage chain left them with its statistics: T the basin's rank per cell, R the receivers. This file
// adds P (the donors still to report), RC (receivers in bits 0..7, donors above them: P counts down to 0), Q (the ready list) and AQ,
// the 64-bit plane of A. Per member eight counter words, `ring`: n[3] and lo[3]. Round j of the flow reads the cells Q[lo[j % 3] ..
// + n[j % 3]), which the launch before it completed; it appends behind them through the atomic n[(j + 1) % 3], one lane writes
// lo[(j + 1) % 3] = lo + n and clears n[(j + 2) % 3], which nobody else touches during round j. A cell enters the list once: as a
// leaf (a giver without donors), or when the decrement that takes its P from 1 to 0 finds it a giver.
//   pending  a TX x TY tile of heights and dry marks with a halo of one in LDS (outside the map: a NaN, never lower, never higher).
//            P = donors, RC, AQ = ONE; the tile's leaves are counted in LDS, ONE atomic per workgroup reserves their room in Q, then
//            they are written. The same workgroups set the member's records to the fold's identities.
//   flow     one listed giver per lane, the grid strides over the round's range. The lane reads A(c), recomputes the fractions from
//            the nine top records, adds the shares with agent-scope u64 atomics (and the basin leakage where the ranks of giver and
//            receiver differ), and decrements every receiver's P with release. Where a decrement takes P from 1 to 0 and the
//            receiver is a giver, that receiver's A is complete: the lane carries on with the first such receiver (behind an
//            acquire) and appends the others to the list; after DISP_CARRY givers in a row it lists the one it holds as well,
//            so that no launch waits for one long walk. It never waits, polls or spins: a walk strictly descends in h and ends
//            where no receiver became ready. A launch that found cells in a member's range sets ITS bit of `busy`, whatever the
//            number of members: the host counts launches, and stops at the first one whose bit stayed clear.
//   fold     per basin the inflow (A over the terminal cells: the sink, or the wet cells), the largest A over the dry cells, the
//            givers and the givers with two receivers or more, in an LDS table; ONE set of atomics per basin and workgroup.
//   peak     the smallest dry cell that holds the basin's largest A; the planes asked for are unpacked from RC (donors over P).
// Integer adds and order-free extremes only: nothing depends on the launch shape or on the order of arrival.
// The file compiles for the device and, under SMX_D / SMX_HOSTSIM, for the host (tests/dispersal_host), as soil_paths.h does.
#pragma once
#include "soil_drain.h"

namespace smx {

constexpr uint64_t DISP_ONE = 1ull << 24;
constexpr uint32_t DISP_MAX_EXPONENT = 16u;
constexpr uint32_t DISP_NONE = 0xFFFFFFFFu;    // no cell; the free key of the fold's table
constexpr uint32_t DISP_RING = 8u;             // counter words per member: n[0..3), lo[3..6), two spare
#ifndef SMX_DISP_BATCH                         // (the three can be set on the compiler's command line: profiles/r22_dispersal.md compares builds)
#define SMX_DISP_BATCH 32
#endif
#ifndef SMX_DISP_FLOW_BLOCKS
#define SMX_DISP_FLOW_BLOCKS 1024
#endif
#ifndef SMX_DISP_CARRY
#define SMX_DISP_CARRY 2
#endif
constexpr uint32_t DISP_CARRY = SMX_DISP_CARRY;               // givers a lane takes in a row before it hands the walk back to the list
static_assert(DISP_CARRY >= 1u, "a listed giver is handled by the launch that reads it");
constexpr uint32_t DISP_BATCH = SMX_DISP_BATCH;               // flow launches the host queues between two looks at `busy`, a bit each
static_assert(DISP_BATCH >= 1u && DISP_BATCH <= 32u, "one bit of the busy word per launch of a batch");
constexpr unsigned DISP_FLOW_BLOCKS = SMX_DISP_FLOW_BLOCKS;   // workgroups of a flow launch at most

struct DispAcc {      // a basin's figures while they are folded (48 bytes)
  uint64_t inflow, leak_in, leak_out, peak;
  uint32_t peak_cell, givers, split_cells, pad;
};
struct DispRec {      // == smx_dispersal_record (include/soilmx.h)
  uint32_t first_cell, cells, flags, peak_cell;
  uint64_t inflow_q24, leak_in_q24, leak_out_q24, peak_q24;
  uint32_t givers, split_cells;
  uint32_t reserved[2];
};
static_assert(sizeof(DispAcc) == 48 && sizeof(DispRec) == 64, "dispersal record layouts");

SMX_HD void disp_finish(const BasinAcc& b, const DispAcc& a, DispRec& r) {
  r.first_cell = b.first_cell; r.cells = b.cells; r.flags = b.flags; r.peak_cell = a.peak_cell;
  r.inflow_q24 = a.inflow; r.leak_in_q24 = a.leak_in; r.leak_out_q24 = a.leak_out; r.peak_q24 = a.peak;
  r.givers = a.givers; r.split_cells = a.split_cells; r.reserved[0] = r.reserved[1] = 0u;
}

// (a * f) >> 24 through the 128-bit product: a < 2^56 and f <= 2^24, so the result fits 64 bits
SMX_D uint64_t disp_share(uint64_t a, uint32_t f) {
#ifdef SMX_HOSTSIM
  return (uint64_t)(((unsigned __int128)a * (unsigned __int128)f) >> 24);
#else
  return (__umul64hi(a, (uint64_t)f) << 40) | ((a * (uint64_t)f) >> 24);
#endif
}
// neighbour d of 0..7 in ascending cell index: (-1,-1) (-1,0) (-1,1) (0,-1) (0,1) (1,-1) (1,0) (1,1)
SMX_D int disp_dx(int d) { return (d < 4 ? d : d + 1) / 3 - 1; }
SMX_D int disp_dy(int d) { return (d < 4 ? d : d + 1) % 3 - 1; }

// The fractions of cell (x, y) of height hc towards its eight neighbours, from the heights hn[d] (a NaN for a cell outside the map):
// f[d], 0 where d is not lower; the return value has bit d set where neighbour d is lower.
SMX_D uint32_t disp_fractions(double hc, const double* hn, uint32_t exponent, uint32_t* f) {
  double w[8], W = 0.0;
  uint32_t lower = 0u;
#pragma unroll
  for (int d = 0; d < 8; d++) {
    w[d] = 0.0;
    if (!(hn[d] < hc)) continue;
    lower |= 1u << d;
    const double s = (hc - hn[d]) * ((disp_dx(d) != 0 && disp_dy(d) != 0) ? 0x1.6a09e667f3bcdp-1 : 1.0);
    double p = 1.0;
    for (uint32_t e = 0; e < exponent; e++) p = p * s;
    w[d] = p;
    W = W + p;
  }
  const bool ok = W > 0.0 && W <= 0x1.fffffffffffffp+1023;
#pragma unroll
  for (int d = 0; d < 8; d++) f[d] = (ok && ((lower >> d) & 1u)) ? (uint32_t)((w[d] / W) * 16777216.0) : 0u;
  return lower;
}

// ---- pending: workgroup `tile` of member m. LDS: hs and ds, (TX + 2) * (TY + 2) doubles and words; sl, TX * TY words; wc, 2 words ----
template <int TX, int TY, class G>
SMX_D void disp_pending_group(const LakeMember& m, G& g, uint32_t tile, uint32_t ntiles, double* hs, uint32_t* ds, uint32_t* sl, uint32_t* wc, uint32_t* P,
                              uint32_t* RC, uint32_t* Q, uint64_t* AQ, DispAcc* acc, uint32_t* ring) {
  constexpr int HY = TY + 2, HN = (TX + 2) * HY;
  const uint32_t nl = g.lanes();
  const int nty = (m.dimy + TY - 1) / TY;
  const int x0 = (int)(tile / (uint32_t)nty) * TX, y0 = (int)(tile % (uint32_t)nty) * TY;
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    if (l == 0u) wc[0] = 0u;
    for (uint32_t i = l; i < (uint32_t)HN; i += nl) {   // (y runs fastest: adjacent lanes, adjacent records)
      const int x = x0 - 1 + (int)(i / HY), y = y0 - 1 + (int)(i % HY);
      const bool in = x >= 0 && y >= 0 && x < m.dimx && y < m.dimy;
      double h = __builtin_nan("");
      uint32_t dry = 0u;
      if (in) { const Sec top = m.cells[(size_t)x * m.dimy + y]; h = drain_height(top); dry = top.type == AIR ? 0u : 1u; }
      hs[i] = h; ds[i] = dry;
    }
    for (uint64_t r = (uint64_t)tile * nl + l; r < m.cap; r += (uint64_t)ntiles * nl) {   // the member's records: the identities of the fold
      DispAcc z;
      z.inflow = 0ull; z.leak_in = 0ull; z.leak_out = 0ull; z.peak = 0ull; z.peak_cell = DISP_NONE; z.givers = 0u; z.split_cells = 0u; z.pad = 0u;
      acc[m.rec0 + r] = z;
    }
  }
  g.barrier();
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    for (uint32_t i = l; i < (uint32_t)(TX * TY); i += nl) {
      const int lx = (int)(i / TY), ly = (int)(i % TY);
      const int x = x0 + lx, y = y0 + ly;
      sl[i] = DISP_NONE;
      if (x >= m.dimx || y >= m.dimy) continue;
      const size_t a = (size_t)m.off + (size_t)x * m.dimy + y;
      const int at = (lx + 1) * HY + (ly + 1);
      const double hc = hs[at];
      uint32_t donors = 0u, lower = 0u;
      for (int dx = -1; dx <= 1; dx++)
        for (int dy = -1; dy <= 1; dy++) {
          if (dx == 0 && dy == 0) continue;
          const double hn = hs[at + dx * HY + dy];
          if (hn < hc) lower++;
          if (hc < hn && ds[at + dx * HY + dy]) donors++;   // (a dry cell above c has c below it: it is a giver)
        }
      const uint32_t receivers = ds[at] ? lower : 0u;
      P[a] = donors; RC[a] = receivers | (donors << 8); AQ[a] = DISP_ONE;
      if (receivers && !donors) sl[i] = SMX_LAKE_ADD(wc, 1u, SMX_LAKE_WG);   // a leaf: its place among the tile's leaves
    }
  }
  g.barrier();
  for (uint32_t l = g.lo(); l < g.hi(); l++)
    if (l == 0u) wc[1] = wc[0] ? SMX_LAKE_ADD(ring, wc[0], SMX_LAKE_AGENT) : 0u;   // ONE atomic reserves the tile's room in the list
  g.barrier();
  for (uint32_t l = g.lo(); l < g.hi(); l++)
    for (uint32_t i = l; i < (uint32_t)(TX * TY); i += nl) {
      if (sl[i] == DISP_NONE) continue;   // (leaves in all: at most the member's cells, the list's length)
      Q[(size_t)m.off + wc[1] + sl[i]] = (uint32_t)(x0 + (int)(i / TY)) * (uint32_t)m.dimy + (uint32_t)(y0 + (int)(i % TY));
    }
}

// ---- flow: what the giver c hands on. Returns a receiver that this hand-over completed (the lane carries on there), DISP_NONE
//      where there is none; further ones go to the list through the tail `app`, behind `base`. ----
SMX_D uint32_t disp_give(const LakeMember& m, uint32_t c, uint32_t exponent, const uint32_t* T, const uint32_t* R, uint32_t* P, const uint32_t* RC, uint32_t* Q,
                         uint64_t* AQ, DispAcc* acc, uint32_t base, uint32_t* app) {
  const uint32_t dimy = (uint32_t)m.dimy;
  const int x = (int)(c / dimy), y = (int)(c % dimy);
  const size_t a = (size_t)m.off + c;
  const double hc = drain_height(m.cells[c]);
  double hn[8];
#pragma unroll
  for (int d = 0; d < 8; d++) {
    const int u = x + disp_dx(d), v = y + disp_dy(d);
    hn[d] = (u >= 0 && v >= 0 && u < m.dimx && v < m.dimy) ? drain_height(m.cells[(size_t)u * dimy + (size_t)v]) : __builtin_nan("");
  }
  uint32_t f[8];
  const uint32_t lower = disp_fractions(hc, hn, exponent, f);
  const uint64_t A = SMX_LAKE_LD(AQ + a, SMX_LAKE_AGENT);   // (complete: every donor added before the decrement that made c ready)
  uint64_t share[8], sum = 0ull;
#pragma unroll
  for (int d = 0; d < 8; d++) { share[d] = disp_share(A, f[d]); sum += share[d]; }
  const uint64_t rem = A - sum;
  const uint32_t rank = T[a], recv = R[a];   // (a giver has a receiver, and it is one of the lower neighbours)
  uint32_t next = DISP_NONE;
#pragma unroll
  for (int d = 0; d < 8; d++) {
    if (!((lower >> d) & 1u)) continue;
    const uint32_t n = c + (uint32_t)(disp_dx(d) * (int)dimy + disp_dy(d));   // (unsigned: a cell index may pass 2^31)
    const uint32_t an = m.off + n;
    const uint64_t amount = share[d] + (an == recv ? rem : 0ull);
    if (amount) {
      SMX_LAKE_ADD(AQ + an, amount, SMX_LAKE_AGENT);
      const uint32_t rn = T[an];
      if (rn != rank) {
        if (rank < m.cap) SMX_LAKE_ADD(&acc[m.rec0 + rank].leak_out, amount, SMX_LAKE_AGENT);
        if (rn < m.cap) SMX_LAKE_ADD(&acc[m.rec0 + rn].leak_in, amount, SMX_LAKE_AGENT);
      }
    }
    if (SMX_DRAIN_DEC_RELEASE(P + an) != 1u) continue;   // a donor of n is still to come
    if (!(RC[an] & 0xFFu)) continue;                     // n is complete, and gives nothing: a sink or a wet cell
    if (next == DISP_NONE) next = n;
    else Q[(size_t)m.off + base + SMX_LAKE_ADD(app, 1u, SMX_LAKE_AGENT)] = n;   // (a cell is listed once: the list has room)
  }
  if (next != DISP_NONE) SMX_DRAIN_ACQUIRE();   // every donor's add happened before its decrement: next's A is complete
  return next;
}

// workgroup `block` of `nblocks` strides over the range of round `round` (ring: the member's counter words; busy: the batch's word,
// bit: this launch's bit in it -- every member with work sets the same bit, so the word counts launches, not members)
template <class G>
SMX_D void disp_flow_group(const LakeMember& m, G& g, uint32_t block, uint32_t nblocks, uint32_t round, uint32_t exponent, const uint32_t* T, const uint32_t* R,
                           uint32_t* P, const uint32_t* RC, uint32_t* Q, uint64_t* AQ, DispAcc* acc, uint32_t* ring, uint32_t* busy, uint32_t bit) {
  const uint32_t nl = g.lanes();
  const uint32_t ra = round % 3u, rb = (round + 1u) % 3u, rc = (round + 2u) % 3u;
  const uint32_t lo = ring[3u + ra], n = ring[ra];   // (settled by the launch before; this launch writes the two other pairs only)
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    if (block == 0u && l == 0u) {
      ring[3u + rb] = lo + n; ring[rc] = 0u;
      if (n) SMX_LAKE_OR(busy, bit, SMX_LAKE_AGENT);
    }
    for (uint64_t i = (uint64_t)block * nl + l; i < n; i += (uint64_t)nblocks * nl) {
      uint32_t c = Q[(size_t)m.off + lo + (size_t)i];
      // Every turn moves c to one of its lower neighbours: the walk strictly descends in h and ends where the hand-over completed
      // no giver. It never waits: a receiver with a donor still to come is taken up by the lane whose decrement is the last one.
      // After DISP_CARRY givers the lane lists the one it holds -- complete, and never listed before -- for the next round: a launch
      // lasts as long as its longest walk, and one long walk would keep every other lane of the launch idle.
      for (uint32_t step = 0; c != DISP_NONE; step++) {
        if (step == DISP_CARRY) { Q[(size_t)m.off + lo + n + SMX_LAKE_ADD(ring + rb, 1u, SMX_LAKE_AGENT)] = c; break; }
        c = disp_give(m, c, exponent, T, R, P, RC, Q, AQ, acc, lo + n, ring + rb);
      }
    }
  }
}

// ---- fold: workgroup `block` takes (SLOTS / lanes) * lanes cells; the LDS table has a slot for every one of them ----
template <int SLOTS>
struct DispTable {
  uint64_t inflow[SLOTS], peak[SLOTS];
  uint32_t key[SLOTS], givers[SLOTS], split[SLOTS];
};
template <int SLOTS, class G>
SMX_D void disp_fold_group(const LakeMember& m, G& g, uint32_t block, DispTable<SLOTS>& t, const uint32_t* T, const uint32_t* R, const uint32_t* RC, const uint64_t* AQ,
                           DispAcc* acc) {
  const uint32_t nl = g.lanes(), items = (uint32_t)SLOTS / nl;
  const uint64_t n = (uint64_t)m.dimx * (uint64_t)m.dimy, c0 = (uint64_t)block * items * nl;
  for (uint32_t l = g.lo(); l < g.hi(); l++)
    for (uint32_t s = l; s < (uint32_t)SLOTS; s += nl) { t.key[s] = DISP_NONE; t.inflow[s] = 0ull; t.peak[s] = 0ull; t.givers[s] = 0u; t.split[s] = 0u; }
  g.barrier();
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    for (uint32_t it = 0; it < items; it++) {
      const uint64_t c = c0 + (uint64_t)it * nl + l;
      if (c >= n) break;
      const size_t a = (size_t)m.off + (size_t)c;
      const uint32_t rank = T[a];
      if (rank >= m.cap) continue;
      const uint64_t A = AQ[a];
      const uint32_t receivers = RC[a] & 0xFFu;
      uint32_t s = (rank * 2654435761u) % (uint32_t)SLOTS;
      for (;;) {   // (at most SLOTS keys are ever inserted: a free or matching slot exists)
        const uint32_t k = SMX_LAKE_CAS(t.key + s, DISP_NONE, rank, SMX_LAKE_WG);
        if (k == DISP_NONE || k == rank) break;
        s = s + 1u == (uint32_t)SLOTS ? 0u : s + 1u;
      }
      if (R[a] == DRAIN_NONE) SMX_LAKE_ADD(t.inflow + s, A, SMX_LAKE_WG);             // a terminal cell: the sink, or a wet cell
      if (m.cells[c].type != AIR) SMX_LAKE_MAX(t.peak + s, A, SMX_LAKE_WG);           // (A >= ONE: a basin with dry land has a peak above 0)
      if (receivers) SMX_LAKE_ADD(t.givers + s, 1u, SMX_LAKE_WG);
      if (receivers >= 2u) SMX_LAKE_ADD(t.split + s, 1u, SMX_LAKE_WG);
    }
  }
  g.barrier();
  for (uint32_t l = g.lo(); l < g.hi(); l++)
    for (uint32_t s = l; s < (uint32_t)SLOTS; s += nl) {
      if (t.key[s] == DISP_NONE) continue;
      DispAcc& r = acc[m.rec0 + t.key[s]];
      if (t.inflow[s]) SMX_LAKE_ADD(&r.inflow, t.inflow[s], SMX_LAKE_AGENT);
      if (t.peak[s]) SMX_LAKE_MAX(&r.peak, t.peak[s], SMX_LAKE_AGENT);
      if (t.givers[s]) SMX_LAKE_ADD(&r.givers, t.givers[s], SMX_LAKE_AGENT);
      if (t.split[s]) SMX_LAKE_ADD(&r.split_cells, t.split[s], SMX_LAKE_AGENT);
    }
}

// ---- peak: workgroup `block` takes g.lanes() cells. RC is read by the cell's own lane and then, where a plane is asked for,
//      unpacked: the donors over P (counted down to 0 by then), the receivers over RC itself. ----
template <class G>
SMX_D void disp_peak_group(const LakeMember& m, G& g, uint32_t block, const uint32_t* T, uint32_t* P, uint32_t* RC, const uint64_t* AQ, DispAcc* acc,
                           uint32_t want_donors, uint32_t want_receivers) {
  const uint32_t nl = g.lanes();
  const uint64_t n = (uint64_t)m.dimx * (uint64_t)m.dimy;
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    const uint64_t c = (uint64_t)block * nl + l;
    if (c >= n) continue;
    const size_t a = (size_t)m.off + (size_t)c;
    const uint32_t rank = T[a], w = RC[a];
    if (rank < m.cap && m.cells[c].type != AIR && AQ[a] == acc[m.rec0 + rank].peak) SMX_LAKE_MIN(&acc[m.rec0 + rank].peak_cell, (uint32_t)c, SMX_LAKE_AGENT);
    if (want_donors) P[a] = w >> 8;
    if (want_receivers) RC[a] = w & 0xFFu;
  }
}

}  // namespace smx
