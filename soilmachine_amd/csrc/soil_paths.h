// soil_paths.h -- the flow paths (smx_flowpaths / smx_ensemble_flowpaths): how far every cell is from where its water ends up and how
// far it falls on the way, the longest path that arrives at every cell, and per basin the main stem -- its longest flow path -- with
// the ordered list of its cells, the profile. The bodies of k_path_init, k_path_fold, k_path_up, k_path_lengths and k_path_stem; the
// pointer doubling between them is k_hill_jump of soil_hills.h, unchanged. Nothing here writes a map.
//
// Cells, h(c), wet cells, receivers, sinks, basins and their ranks are those of soil_drain.h. The TERMINAL t(c) of a dry cell is the
// last cell of c, R(c), R(R(c)), ...: a sink (c itself where c is one) or the first wet cell the path meets; a wet cell is its own.
// straight(c) / diagonal(c) count the steps to it, steps = straight + diagonal, drop(c) = h(c) - h(t(c)) in one f64 subtraction (+0.0
// where t(c) == c). key(c) = (steps(c) << 32) | (0xFFFFFFFF - c); up(c) is the largest key over the cells whose path passes through
// c, c included: up(c) >> 32 is where the longest path that arrives at c started counting, 0xFFFFFFFF - (u32)up(c) the cell it starts
// at (of equally long ones the smallest). far(b) is the largest key of basin b; the MAIN STEM of b is the set of cells with
// up(c) == far(b) -- keys are unique, so it is exactly one path, from the source to its terminal --, stem(c) = steps_max(b) - steps(c)
// the position on it. The PROFILE lists the stems' cells, basin after basin in rank order, each from its source down.
//
// The planes are read as the drainage chain left them with its statistics: T the basin's rank per cell, R the receivers, and P the
// pending donors of k_drain_pending. Two sets of three u32 planes (J the jump pointer, a plane index; S, G the steps to it) are
// written in turns by k_hill_jump. Per-basin words live in planes too, basin r of a member at word off + r:
//   init     J[c] = c for a sink and for a wet cell, with no step; else J[c] = R[c] with that one step in S or G. R stays. FH[..] = 0;
//            the member's records are set to the fold's identities.
//   jump     k_hill_jump, hill_rounds(cells of the largest map - 1) rounds: J becomes the terminal, S and G the steps to it.
//   fold     each cell writes its key into UP, a 64-bit plane, and folds cells, the step sums, the largest drop, the smallest
//            receiverless cell (first_cell) and the largest steps per rank in an LDS table; ONE set of atomics per basin and workgroup
//            goes to the record (ranks below cap) and to FH, the largest steps of EVERY basin. FS[..] = 0xFFFFFFFF.
//   up       a lane that owns a leaf walks downstream as k_drain_area does, on the same pending words: it raises the receiver's UP
//            word to the key it carries (a 64-bit max) and decrements the receiver's P; only the lane that takes P from 1 to 0 reads
//            the receiver's word and carries on. It never waits; it ends at a sink, at a wet cell, or where a donor is still to come.
//   lengths  the wide key far(b) = (FH, 0xFFFFFFFF - FS) is settled in its second half: every cell whose steps attain FH of its
//            basin lowers FS to its index. The same lanes, as ranks, write L[r] = FH[r] + 1 for the member's basins, 0 behind them.
//            The caller scans L into PA: profile_at(r) = PA[off + r] - PA[off].
//   stem     one lane per cell compares up(c) with (FH, FS) of its basin and writes the planes asked for -- stem over T, the
//            terminal over J, the drop over the cell's own UP word, each read by that lane alone before --, scatters c into the
//            profile, and, where c is the source of a basin below cap, completes that record. No walk along a river.
// Integer adds, order-free extremes, copied and once-subtracted doubles only: nothing depends on the order of the contributions.
// The file compiles for the device and, under SMX_D / SMX_HOSTSIM, for the host (tests/flowpaths_host), as soil_hills.h does.
#pragma once
#include "soil_hills.h"

namespace smx {

constexpr uint32_t PATH_NONE = 0xFFFFFFFFu;   // stem: a cell off the stems; the free key of the fold's table
constexpr uint32_t PATH_F_WET = 1u;           // terminal_cell is wet

struct PathAcc {      // a record while it is folded (64 bytes, as smx_flowpath): first_cell as a minimum, drop_max as its ordered image
  uint32_t first_cell, cells, source_cell, terminal_cell, steps_max, diagonal, profile_at, flags;
  uint64_t straight_sum, diagonal_sum;
  double drop_source;
  uint64_t dmax;
};
struct PathRec {      // == smx_flowpath (include/soilmx.h)
  uint32_t first_cell, cells, source_cell, terminal_cell, steps_max, diagonal, profile_at, flags;
  uint64_t straight_sum, diagonal_sum;
  double drop_source, drop_max;
};
static_assert(sizeof(PathAcc) == 64 && sizeof(PathRec) == 64, "flow path record layouts");

SMX_HD void path_finish(const PathAcc& a, PathRec& r) {
  r.first_cell = a.first_cell; r.cells = a.cells; r.source_cell = a.source_cell; r.terminal_cell = a.terminal_cell;
  r.steps_max = a.steps_max; r.diagonal = a.diagonal; r.profile_at = a.profile_at; r.flags = a.flags;
  r.straight_sum = a.straight_sum; r.diagonal_sum = a.diagonal_sum;
  r.drop_source = a.drop_source; r.drop_max = lake_unkey(a.dmax);
}
SMX_HD uint64_t path_key(uint32_t steps, uint32_t c) { return ((uint64_t)steps << 32) | (uint64_t)(0xFFFFFFFFu - c); }
SMX_HD uint64_t path_bits(double v) { uint64_t b; __builtin_memcpy(&b, &v, 8); return b; }

// ---- init: workgroup `block` of `nblocks` takes g.lanes() cells ----
template <class G>
SMX_D void path_init_group(const LakeMember& m, G& g, uint32_t block, uint32_t nblocks, const uint32_t* R, uint32_t* J, uint32_t* S, uint32_t* Gd, uint32_t* FH,
                           PathAcc* acc) {
  const uint32_t nl = g.lanes(), dimy = (uint32_t)m.dimy;
  const uint64_t n = (uint64_t)m.dimx * (uint64_t)m.dimy;
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    for (uint64_t r = (uint64_t)block * nl + l; r < m.cap; r += (uint64_t)nblocks * nl) {   // the member's records: the identities of the fold
      PathAcc z;
      z.first_cell = 0xFFFFFFFFu; z.cells = 0u; z.source_cell = 0u; z.terminal_cell = 0u; z.steps_max = 0u; z.diagonal = 0u; z.profile_at = 0u; z.flags = 0u;
      z.straight_sum = 0ull; z.diagonal_sum = 0ull; z.drop_source = 0.0; z.dmax = 0ull;
      acc[m.rec0 + r] = z;
    }
    const uint64_t c = (uint64_t)block * nl + l;
    if (c >= n) continue;
    const uint32_t a = m.off + (uint32_t)c;
    FH[a] = 0u;
    const uint32_t r = R[a];   // (DRAIN_NONE for a sink and for a wet cell)
    if (r == DRAIN_NONE) { J[a] = a; S[a] = 0u; Gd[a] = 0u; continue; }
    const uint32_t cc = (uint32_t)c, rc = r - m.off;
    const uint32_t diag = cc / dimy != rc / dimy && cc % dimy != rc % dimy ? 1u : 0u;
    J[a] = r; S[a] = 1u - diag; Gd[a] = diag;
  }
}

// ---- fold: workgroup `block` takes (SLOTS / lanes) * lanes cells; the LDS table has a slot for every one of them ----
template <int SLOTS>
struct PathTable {
  uint64_t ssum[SLOTS], dsum[SLOTS], dmax[SLOTS];
  uint32_t key[SLOTS], cells[SLOTS], first[SLOTS], far[SLOTS];
};

// (T: the ranks; J, S, Gd: the settled set; UP: the keys, written here; FH: the largest steps per rank; FS: set to its identity)
template <int SLOTS, class G>
SMX_D void path_fold_group(const LakeMember& m, G& g, uint32_t block, PathTable<SLOTS>& t, const uint32_t* T, const uint32_t* R, const uint32_t* J, const uint32_t* S,
                           const uint32_t* Gd, uint64_t* UP, uint32_t* FH, uint32_t* FS, PathAcc* acc) {
  const uint32_t nl = g.lanes(), items = (uint32_t)SLOTS / nl;
  const uint64_t n = (uint64_t)m.dimx * (uint64_t)m.dimy, c0 = (uint64_t)block * items * nl;
  for (uint32_t l = g.lo(); l < g.hi(); l++)
    for (uint32_t s = l; s < (uint32_t)SLOTS; s += nl) {
      t.key[s] = PATH_NONE; t.cells[s] = 0u; t.first[s] = 0xFFFFFFFFu; t.far[s] = 0u; t.ssum[s] = 0ull; t.dsum[s] = 0ull; t.dmax[s] = 0ull;
    }
  g.barrier();
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    for (uint32_t it = 0; it < items; it++) {
      const uint64_t c = c0 + (uint64_t)it * nl + l;
      if (c >= n) break;
      const size_t a = (size_t)m.off + (size_t)c;
      const uint32_t rank = T[a], sc = S[a], dc = Gd[a], e = J[a];
      UP[a] = path_key(sc + dc, (uint32_t)c);
      FS[a] = 0xFFFFFFFFu;
      double d = 0.0;
      if (e != (uint32_t)a) d = drain_height(m.cells[c]) - drain_height(m.cells[e - m.off]);
      uint32_t s = (rank * 2654435761u) % (uint32_t)SLOTS;
      for (;;) {   // (at most SLOTS keys are ever inserted: a free or matching slot exists)
        const uint32_t k = SMX_LAKE_CAS(t.key + s, PATH_NONE, rank, SMX_LAKE_WG);
        if (k == PATH_NONE || k == rank) break;
        s = s + 1u == (uint32_t)SLOTS ? 0u : s + 1u;
      }
      SMX_LAKE_ADD(t.cells + s, 1u, SMX_LAKE_WG);
      if (R[a] == DRAIN_NONE) SMX_LAKE_MIN(t.first + s, (uint32_t)c, SMX_LAKE_WG);   // (the sink, or a cell of the lake: the smallest is first_cell)
      SMX_LAKE_MAX(t.far + s, sc + dc, SMX_LAKE_WG);
      if (sc) SMX_LAKE_ADD(t.ssum + s, (uint64_t)sc, SMX_LAKE_WG);
      if (dc) SMX_LAKE_ADD(t.dsum + s, (uint64_t)dc, SMX_LAKE_WG);
      SMX_LAKE_MAX(t.dmax + s, lake_key(d), SMX_LAKE_WG);
    }
  }
  g.barrier();
  for (uint32_t l = g.lo(); l < g.hi(); l++)
    for (uint32_t s = l; s < (uint32_t)SLOTS; s += nl) {
      const uint32_t rank = t.key[s];
      if (rank == PATH_NONE) continue;
      if (t.far[s]) SMX_LAKE_MAX(FH + m.off + rank, t.far[s], SMX_LAKE_AGENT);   // (every basin, whatever cap is)
      if (rank >= m.cap) continue;
      PathAcc& r = acc[m.rec0 + rank];
      SMX_LAKE_ADD(&r.cells, t.cells[s], SMX_LAKE_AGENT);
      if (t.first[s] != 0xFFFFFFFFu) SMX_LAKE_MIN(&r.first_cell, t.first[s], SMX_LAKE_AGENT);
      if (t.ssum[s]) SMX_LAKE_ADD(&r.straight_sum, t.ssum[s], SMX_LAKE_AGENT);
      if (t.dsum[s]) SMX_LAKE_ADD(&r.diagonal_sum, t.dsum[s], SMX_LAKE_AGENT);
      SMX_LAKE_MAX(&r.dmax, t.dmax[s], SMX_LAKE_AGENT);
    }
}

// ---- up: workgroup `block` takes g.lanes() cells; every access to P and UP is an agent-scope atomic, as in drain_area_group ----
template <class G>
SMX_D void path_up_group(const LakeMember& m, G& g, uint32_t block, const uint32_t* R, uint32_t* P, uint64_t* UP) {
  const uint32_t nl = g.lanes();
  const uint64_t n = (uint64_t)m.dimx * (uint64_t)m.dimy;
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    const uint64_t c = (uint64_t)block * nl + l;
    if (c >= n) continue;
    uint32_t cur = m.off + (uint32_t)c;
    if (SMX_LAKE_LD(P + cur, SMX_LAKE_AGENT) != DRAIN_LEAF) continue;   // (a leaf's P never changes, and nobody raises its word: it stays its own key)
    uint64_t carry = SMX_LAKE_LD(UP + cur, SMX_LAKE_AGENT);
    // Every turn moves cur to its receiver, one step down a path that strictly descends in h: the walk ends at a sink, at a wet
    // cell, or earlier, where another donor is still to report. It never waits: the lane whose decrement is the last one goes on.
    for (;;) {
      const uint32_t r = R[cur];
      if (r == DRAIN_NONE) break;                        // cur is a sink: its word is complete
      SMX_LAKE_MAX(UP + r, carry, SMX_LAKE_AGENT);
      if (SMX_DRAIN_DEC_RELEASE(P + r) != 1u) break;     // a donor of r is still to come (or r is wet)
      SMX_DRAIN_ACQUIRE();                               // every donor's max happened before its decrement: r's word is complete
      carry = SMX_LAKE_LD(UP + r, SMX_LAKE_AGENT);
      cur = r;
    }
  }
}

// ---- lengths: workgroup `block` takes g.lanes() words, each as a cell and as a rank (nb: the member's basins, counted by k_drain_stats) ----
template <class G>
SMX_D void path_lengths_group(const LakeMember& m, G& g, uint32_t block, const uint32_t* T, const uint32_t* S, const uint32_t* Gd, const uint32_t* FH, uint32_t* FS,
                              uint32_t* L, const uint32_t* nbasins) {
  const uint32_t nl = g.lanes(), nb = *nbasins;
  const uint64_t n = (uint64_t)m.dimx * (uint64_t)m.dimy;
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    const uint64_t c = (uint64_t)block * nl + l;
    if (c >= n) continue;
    const uint32_t a = m.off + (uint32_t)c, at = m.off + T[a];
    if (S[a] + Gd[a] == FH[at]) SMX_LAKE_MIN(FS + at, (uint32_t)c, SMX_LAKE_AGENT);
    L[a] = c < nb ? FH[a] + 1u : 0u;
  }
}

// ---- stem: workgroup `block` takes g.lanes() cells. T, J and UP are read by the cell's own lane and then, where the plane is asked
//      for, overwritten with stem, terminal and drop. FH, FS and PA are read-only here. ----
struct PathOut {
  uint32_t want_terminal, want_stem, want_drop, profile_cap;
  uint32_t *upstream, *source, *profile;   // null = not asked for
};
template <class G>
SMX_D void path_stem_group(const LakeMember& m, G& g, uint32_t block, uint32_t* T, uint32_t* J, const uint32_t* S, const uint32_t* Gd, uint64_t* UP, const uint32_t* FH,
                           const uint32_t* FS, const uint32_t* PA, PathAcc* acc, const uint32_t* nbasins, uint32_t* nprofile, const PathOut& o) {
  const uint32_t nl = g.lanes();
  const uint64_t n = (uint64_t)m.dimx * (uint64_t)m.dimy;
  const uint32_t before = PA[m.off];
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    const uint64_t c = (uint64_t)block * nl + l;
    if (c >= n) continue;
    const uint32_t a = m.off + (uint32_t)c;
    if (c == n - 1) *nprofile = PA[a] + (c < *nbasins ? FH[a] + 1u : 0u) - before;
    const uint64_t u = UP[a];
    const uint32_t rank = T[a], at = m.off + rank, t = J[a], steps = S[a] + Gd[a];
    const uint32_t fh = FH[at], src = 0xFFFFFFFFu - (uint32_t)u;
    const bool on = (uint32_t)(u >> 32) == fh && src == FS[at];
    const uint32_t st = on ? fh - steps : PATH_NONE;
    double d = 0.0;
    if (t != a) d = drain_height(m.cells[c]) - drain_height(m.cells[t - m.off]);
    if (o.want_terminal) J[a] = t - m.off;
    if (o.want_stem) T[a] = st;
    if (o.upstream) o.upstream[a] = (uint32_t)(u >> 32) - steps;
    if (o.source) o.source[a] = src;
    if (o.want_drop) UP[a] = path_bits(d);
    if (!on) continue;
    const uint32_t pa = PA[at] - before;
    if (o.profile && (uint64_t)pa + st < (uint64_t)o.profile_cap) o.profile[pa + st] = (uint32_t)c;   // (one map's list: profile_cap entries of room)
    if (st == 0u && rank < m.cap) {   // the source: the only writer of these
      PathAcc& r = acc[m.rec0 + rank];
      r.source_cell = (uint32_t)c; r.terminal_cell = t - m.off; r.steps_max = fh; r.diagonal = Gd[a]; r.profile_at = pa;
      r.flags = m.cells[t - m.off].type == AIR ? PATH_F_WET : 0u;
      r.drop_source = d;
    }
  }
}

}  // namespace smx
