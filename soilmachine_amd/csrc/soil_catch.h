// soil_catch.h -- the catchments of listed outlets (smx_catchments / smx_ensemble_catchments): which land drains through each cell of
// the caller's list -- a gauge, a dam site, the last cell of a stream segment --, one record per listed cell, the tree the gauges form
// along the flow and, where asked for, the height distribution of every catchment (hypsometry). The bodies of k_catch_mark,
// k_catch_init, k_catch_fold and k_catch_hist; the pointer doubling between init and fold is k_hill_jump of soil_hills.h, unchanged.
// Nothing here writes a map.
//
// Cells, h(c), wet cells, receivers, sinks, basins and their ranks are those of soil_drain.h. The GAUGES are the n >= 1 distinct
// cells of the list, any cell: dry, wet or a sink. The ENTRY e(c) of a dry cell is the first cell on c, R(c), R(R(c)), ... (c
// included) that is a gauge, a sink or a wet cell; a wet cell is its own. gauge(c) is the list position of e(c), CATCH_NONE where e(c)
// is no gauge; straight(c) / diagonal(c) count the steps to e(c); drop(c) = h(c) - h(e(c)) in one f64 subtraction, +0.0 where
// e(c) == c -- defined for every cell, and flowpaths' figures where no gauge lies on the path. The OWN CATCHMENT of gauge i is the
// set of cells with gauge(c) == i, the gauge cell included. downstream(i) = gauge(R(g)) for a gauge cell g that is dry and no sink,
// else CATCH_NONE: a path strictly descends, so the gauges form a forest, and area(i), the cells of the whole catchment, is cells
// summed over the gauge and every gauge above it (catch_area: on the host, children into parents).
//
// The planes are read as the drainage chain left them with its statistics and without its area step: T the basin's rank per cell, R
// the receivers. M is the mark plane; two sets of three u32 planes (J, S, G of soil_hills.h) are written in turns by k_hill_jump:
//   mark   M is CATCH_NONE everywhere (the caller's fill); one lane per list entry writes M[cell] = its position. The caller has
//          refused cells outside a member and duplicates: no two lanes write the same word.
//   init   J[c] = c with no step where M[c] is set or R[c] == DRAIN_NONE; else J[c] = R[c] with that one step in S or G. R stays:
//          downstream reads it. The same workgroups set the member's records to the fold's identities.
//   jump   k_hill_jump, hill_rounds(cells of the largest map - 1) rounds: J becomes the entry, S and G the steps to it.
//   fold   each cell reads its settled (e, s, g), writes the planes asked for and, where M[e] is set, folds its figures per gauge in
//          an LDS table; then ONE set of atomics per gauge and workgroup goes to the record. The lane of a gauge cell writes what
//          only it knows: cell, basin, downstream = M[J[R[g]]], the wet and sink flags.
//   hist   (only with bins) each cell of an own catchment counts in bin min((u32)(drop / bin_height), nbins - 1) of its gauge: an
//          LDS table keyed by gauge * nbins + bin, ONE global add per occupied slot and workgroup.
// Integer adds, order-free extremes, once-subtracted and once-divided doubles only: nothing depends on the order of the contributions.
// The file compiles for the device and, under SMX_D / SMX_HOSTSIM, for the host (tests/catchments_host), as soil_paths.h does.
#pragma once
#include "soil_hills.h"

namespace smx {

constexpr uint32_t CATCH_NONE = 0xFFFFFFFFu;   // gauge: the entry is no gauge; downstream: none; the free key of the tables
constexpr uint32_t CATCH_F_DROP = 1u;          // drop_sum_q40 unreliable
constexpr uint32_t CATCH_F_WET = 2u;           // the gauge cell is wet
constexpr uint32_t CATCH_F_SINK = 4u;          // the gauge cell is a sink
constexpr uint32_t CATCH_MAX_BINS = 64u;

struct CatchAcc {     // a record while it is folded (64 bytes, as smx_catchment): steps_max and farthest_cell as HillAcc::far
  uint32_t cell, cells, basin, downstream;
  uint64_t far;       // (steps << 32) | (0xFFFFFFFF - cell)
  uint64_t straight_sum, diagonal_sum;
  uint64_t dmax;      // the ordered image of drop_max
  uint64_t drop_sum_q40;
  uint32_t flags, pad;
};
struct CatchRec {     // == smx_catchment (include/soilmx.h)
  uint32_t cell, cells, area, downstream;
  uint32_t basin, steps_max, farthest_cell, flags;
  uint64_t straight_sum, diagonal_sum;
  double drop_max;
  uint64_t drop_sum_q40;
};
static_assert(sizeof(CatchAcc) == 64 && sizeof(CatchRec) == 64, "catchment record layouts");

// (area: the own catchment's cells until catch_area has folded the forest)
SMX_HD void catch_finish(const CatchAcc& a, CatchRec& r) {
  r.cell = a.cell; r.cells = a.cells; r.area = a.cells; r.downstream = a.downstream;
  r.basin = a.basin; r.steps_max = (uint32_t)(a.far >> 32); r.farthest_cell = 0xFFFFFFFFu - (uint32_t)a.far; r.flags = a.flags;
  r.straight_sum = a.straight_sum; r.diagonal_sum = a.diagonal_sum;
  r.drop_max = lake_unkey(a.dmax);   // (the gauge cell itself always counts: at least the image of +0.0)
  r.drop_sum_q40 = a.drop_sum_q40;
}
// area of the n records of one map, each still its own cells: children into parents along downstream, every record handled once.
// pending[i] (n words of room) counts the children of i still to report; order (n words) is the stack of the records that are complete.
inline void catch_area(CatchRec* r, uint32_t n, uint32_t* pending, uint32_t* order) {
  uint32_t top = 0u;
  for (uint32_t i = 0; i < n; i++) pending[i] = 0u;
  for (uint32_t i = 0; i < n; i++) if (r[i].downstream != CATCH_NONE) pending[r[i].downstream]++;
  for (uint32_t i = 0; i < n; i++) if (!pending[i]) order[top++] = i;
  while (top) {
    const uint32_t i = order[--top], d = r[i].downstream;
    if (d == CATCH_NONE) continue;
    r[d].area += r[i].area;
    if (--pending[d] == 0u) order[top++] = d;
  }
}
// the bin of a drop: written this way round so that a NaN or an infinity lands in the last bin and nothing out of range is converted
SMX_HD uint32_t catch_bin(double drop, double bin_height, uint32_t nbins) {
  const double q = drop / bin_height;
  return q < (double)nbins ? (uint32_t)q : nbins - 1u;
}

// ---- mark: workgroup `block` takes g.lanes() list entries ----
template <class G>
SMX_D void catch_mark_group(const LakeMember& m, G& g, uint32_t block, const uint32_t* list, uint32_t n, uint32_t* M) {
  const uint32_t nl = g.lanes();
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    const uint64_t i = (uint64_t)block * nl + l;
    if (i >= n) continue;
    M[m.off + list[i]] = (uint32_t)i;   // (list[i] < the member's cells, and no other entry names it: the caller's checks)
  }
}

// ---- init: workgroup `block` of `nblocks` takes g.lanes() cells ----
template <class G>
SMX_D void catch_init_group(const LakeMember& m, G& g, uint32_t block, uint32_t nblocks, const uint32_t* R, const uint32_t* M, uint32_t* J, uint32_t* S, uint32_t* Gd,
                            CatchAcc* acc) {
  const uint32_t nl = g.lanes(), dimy = (uint32_t)m.dimy;
  const uint64_t n = (uint64_t)m.dimx * (uint64_t)m.dimy;
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    for (uint64_t r = (uint64_t)block * nl + l; r < m.cap; r += (uint64_t)nblocks * nl) {   // the member's records: the identities of the fold
      CatchAcc z;
      z.cell = 0u; z.cells = 0u; z.basin = 0u; z.downstream = CATCH_NONE; z.far = 0ull; z.straight_sum = 0ull; z.diagonal_sum = 0ull; z.dmax = 0ull;
      z.drop_sum_q40 = 0ull; z.flags = 0u; z.pad = 0u;
      acc[m.rec0 + r] = z;
    }
    const uint64_t c = (uint64_t)block * nl + l;
    if (c >= n) continue;
    const uint32_t a = m.off + (uint32_t)c;
    const uint32_t r = R[a];   // (DRAIN_NONE for a sink and for a wet cell)
    if (M[a] != CATCH_NONE || r == DRAIN_NONE) { J[a] = a; S[a] = 0u; Gd[a] = 0u; continue; }
    const uint32_t cc = (uint32_t)c, rc = r - m.off;
    const uint32_t diag = cc / dimy != rc / dimy && cc % dimy != rc % dimy ? 1u : 0u;
    J[a] = r; S[a] = 1u - diag; Gd[a] = diag;
  }
}

// ---- fold: workgroup `block` takes (SLOTS / lanes) * lanes cells; the LDS table has a slot for every one of them ----
template <int SLOTS>
struct CatchTable {
  uint64_t far[SLOTS], ssum[SLOTS], dsum[SLOTS], dmax[SLOTS], q40[SLOTS];
  uint32_t key[SLOTS], cells[SLOTS], flags[SLOTS];
};

// (T: the ranks; R: the receivers; M: the marks; J, S, Gd: the settled set; gauge / drop: the planes to write, null = not asked for)
template <int SLOTS, class G>
SMX_D void catch_fold_group(const LakeMember& m, G& g, uint32_t block, CatchTable<SLOTS>& t, const uint32_t* T, const uint32_t* R, const uint32_t* M, const uint32_t* J,
                            const uint32_t* S, const uint32_t* Gd, CatchAcc* acc, uint32_t* gauge, double* drop) {
  const uint32_t nl = g.lanes(), items = (uint32_t)SLOTS / nl;
  const uint64_t n = (uint64_t)m.dimx * (uint64_t)m.dimy, c0 = (uint64_t)block * items * nl;
  for (uint32_t l = g.lo(); l < g.hi(); l++)
    for (uint32_t s = l; s < (uint32_t)SLOTS; s += nl) {
      t.key[s] = CATCH_NONE; t.cells[s] = 0u; t.flags[s] = 0u; t.far[s] = 0ull; t.ssum[s] = 0ull; t.dsum[s] = 0ull; t.dmax[s] = 0ull; t.q40[s] = 0ull;
    }
  g.barrier();
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    for (uint32_t it = 0; it < items; it++) {
      const uint64_t c = c0 + (uint64_t)it * nl + l;
      if (c >= n) break;
      const size_t a = (size_t)m.off + (size_t)c;
      const uint32_t e = J[a], gi = M[e], own = M[a];
      double d = 0.0;
      if (e != (uint32_t)a) d = drain_height(m.cells[c]) - drain_height(m.cells[e - m.off]);
      if (gauge) gauge[a] = gi;
      if (drop) drop[a] = d;
      if (own != CATCH_NONE) {   // a gauge cell: the only writer of these (flags: an OR, the fold's lanes raise CATCH_F_DROP)
        CatchAcc& r = acc[m.rec0 + own];
        const uint32_t rv = R[a];
        const bool wet = m.cells[c].type == AIR;
        r.cell = (uint32_t)c; r.basin = T[a];
        r.downstream = rv == DRAIN_NONE ? CATCH_NONE : M[J[rv]];
        if (rv == DRAIN_NONE) SMX_LAKE_OR(&r.flags, wet ? CATCH_F_WET : CATCH_F_SINK, SMX_LAKE_AGENT);
      }
      if (gi == CATCH_NONE) continue;
      const uint32_t sc = S[a], dc = Gd[a];
      uint32_t f = 0u, lf = 0u;
      const uint64_t q = lake_q40(d, lf);
      if (lf) f |= CATCH_F_DROP;
      uint32_t s = (gi * 2654435761u) % (uint32_t)SLOTS;
      for (;;) {   // (at most SLOTS keys are ever inserted: a free or matching slot exists)
        const uint32_t k = SMX_LAKE_CAS(t.key + s, CATCH_NONE, gi, SMX_LAKE_WG);
        if (k == CATCH_NONE || k == gi) break;
        s = s + 1u == (uint32_t)SLOTS ? 0u : s + 1u;
      }
      SMX_LAKE_ADD(t.cells + s, 1u, SMX_LAKE_WG);
      SMX_LAKE_MAX(t.far + s, ((uint64_t)(sc + dc) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)c), SMX_LAKE_WG);
      if (sc) SMX_LAKE_ADD(t.ssum + s, (uint64_t)sc, SMX_LAKE_WG);
      if (dc) SMX_LAKE_ADD(t.dsum + s, (uint64_t)dc, SMX_LAKE_WG);
      SMX_LAKE_MAX(t.dmax + s, lake_key(d), SMX_LAKE_WG);
      if (q) { const uint64_t o = SMX_LAKE_ADD(t.q40 + s, q, SMX_LAKE_WG); if (o + q < o) f |= CATCH_F_DROP; }
      if (f) SMX_LAKE_OR(t.flags + s, f, SMX_LAKE_WG);
    }
  }
  g.barrier();
  for (uint32_t l = g.lo(); l < g.hi(); l++)
    for (uint32_t s = l; s < (uint32_t)SLOTS; s += nl) {
      if (t.key[s] == CATCH_NONE) continue;
      CatchAcc& r = acc[m.rec0 + t.key[s]];
      uint32_t f = t.flags[s];
      SMX_LAKE_ADD(&r.cells, t.cells[s], SMX_LAKE_AGENT);
      SMX_LAKE_MAX(&r.far, t.far[s], SMX_LAKE_AGENT);
      if (t.ssum[s]) SMX_LAKE_ADD(&r.straight_sum, t.ssum[s], SMX_LAKE_AGENT);
      if (t.dsum[s]) SMX_LAKE_ADD(&r.diagonal_sum, t.dsum[s], SMX_LAKE_AGENT);
      SMX_LAKE_MAX(&r.dmax, t.dmax[s], SMX_LAKE_AGENT);
      if (t.q40[s]) { const uint64_t v = t.q40[s], o = SMX_LAKE_ADD(&r.drop_sum_q40, v, SMX_LAKE_AGENT); if (o + v < o) f |= CATCH_F_DROP; }
      if (f) SMX_LAKE_OR(&r.flags, f, SMX_LAKE_AGENT);
    }
}

// ---- hist: workgroup `block` takes (SLOTS / lanes) * lanes cells: at most that many distinct keys, a slot for every one of them ----
template <int SLOTS>
struct CatchHistTable {
  uint32_t key[SLOTS], count[SLOTS];
};

// (hist: nbins words per record, record m.rec0 + i for gauge i of the member; the caller has set them to 0)
template <int SLOTS, class G>
SMX_D void catch_hist_group(const LakeMember& m, G& g, uint32_t block, CatchHistTable<SLOTS>& t, const uint32_t* M, const uint32_t* J, uint32_t* hist, uint32_t nbins,
                            double bin_height) {
  const uint32_t nl = g.lanes(), items = (uint32_t)SLOTS / nl;
  const uint64_t n = (uint64_t)m.dimx * (uint64_t)m.dimy, c0 = (uint64_t)block * items * nl;
  for (uint32_t l = g.lo(); l < g.hi(); l++)
    for (uint32_t s = l; s < (uint32_t)SLOTS; s += nl) { t.key[s] = CATCH_NONE; t.count[s] = 0u; }
  g.barrier();
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    for (uint32_t it = 0; it < items; it++) {
      const uint64_t c = c0 + (uint64_t)it * nl + l;
      if (c >= n) break;
      const size_t a = (size_t)m.off + (size_t)c;
      const uint32_t e = J[a], gi = M[e];
      if (gi == CATCH_NONE) continue;
      double d = 0.0;
      if (e != (uint32_t)a) d = drain_height(m.cells[c]) - drain_height(m.cells[e - m.off]);
      const uint32_t key = gi * nbins + catch_bin(d, bin_height, nbins);   // (below n * nbins < 2^31: the caller's check)
      uint32_t s = (key * 2654435761u) % (uint32_t)SLOTS;
      for (;;) {   // (at most SLOTS keys are ever inserted: a free or matching slot exists)
        const uint32_t k = SMX_LAKE_CAS(t.key + s, CATCH_NONE, key, SMX_LAKE_WG);
        if (k == CATCH_NONE || k == key) break;
        s = s + 1u == (uint32_t)SLOTS ? 0u : s + 1u;
      }
      SMX_LAKE_ADD(t.count + s, 1u, SMX_LAKE_WG);
    }
  }
  g.barrier();
  for (uint32_t l = g.lo(); l < g.hi(); l++)
    for (uint32_t s = l; s < (uint32_t)SLOTS; s += nl)
      if (t.key[s] != CATCH_NONE) SMX_LAKE_ADD(hist + (size_t)m.rec0 * nbins + t.key[s], t.count[s], SMX_LAKE_AGENT);
}

}  // namespace smx
