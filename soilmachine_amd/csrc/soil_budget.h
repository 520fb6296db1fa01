// soil_budget.h -- the sediment budget (smx_budget / smx_ensemble_budget): what changed from a BASE map to the map of NOW, per
// drainage basin of the base, per soil type, and per cell. The bodies of k_budget_fold and k_budget_where. Nothing here writes a map.
//
// Per map and cell (a column is walked TOP -> BOTTOM with the link validation of soil_strata.h):
//   ground(c)  0.0 for an empty column; the top section's floor where it is Air; else its floor + size in one f64 addition
//   h(c)       drain_height of soil_drain.h
//   V_t(c)     the sum over the column's sections of type t of strata_q40(size), H_t(c) the same on size * sat, S(c) the sum of V_t
//              over every t != 0, W(c) = V_0(c) -- all of them modulo 2^64; a wrap is flagged
// Per cell, now against base: dground and dheight are one f64 subtraction each, dsolid = (int64)(S_now - S_base), dwater the same on
// W. A cell is LOWERED where ground_now < ground_base, RAISED where >, RESURFACED where the top types differ (EMPTY is a type).
//
// k_budget_fold  workgroup `tile` of member blockIdx.y takes a TX x TY tile of cells, one lane a cell. A lane walks BOTH columns in one
//                loop: the two next links are validated and their loads issued before either current section is folded, so the two
//                pointer chases are in flight together. Types 0..BUDGET_PRIV-1 are folded in registers, chosen by unrolled
//                compares; the other types < ntypes the lane met are noted in a 64-bit mask, and the lane walks the two columns once
//                more for each of them (the golden maps hold types 0..4: none). Nothing is indexed by a run-time value outside
//                LDS. The cell's figures go to two LDS tables -- a slot per basin met in the tile (the label plane T of the drainage
//                chain on the base gives the rank), an entry per soil type -- and from there ONE set of agent-scope atomics per
//                basin, and per type, and workgroup goes to the records. Integer adds with wrap detection, and maxima on the bit
//                image of a non-negative f64: no result depends on the launch shape.
// k_budget_where one lane per cell, behind the fold: a lowered cell whose -dground is its basin's cut_max reports itself through a
//                maximum on ~cell, so the SMALLEST such cell stays; likewise the raised cells and fill_max.
// A bad chain in either map is reported through a maximum on ~cell of the map's error word (word 0: the base, word 1 + i: member i).
// The records begin as zeros: 0 is the identity of every add and of the two maxima (the image of +0.0; ~cell of no cell).
// The file compiles for the device and, under SMX_D / SMX_HOSTSIM, for the host (tests/budget_host), as soil_drain.h does.
#pragma once
#include "soil_drain.h"
#include "soil_strata.h"

namespace smx {

constexpr int BUDGET_MAX_TYPES = 64;   // == SMX_TOTALS_MAX_TYPES
constexpr int BUDGET_PRIV = 5;         // types folded in a lane's registers
constexpr uint32_t BUDGET_F_TERM = 1u, BUDGET_F_WRAP = 2u, BUDGET_F_NAN = 4u;
constexpr uint32_t BUDGET_NONE = 0xFFFFFFFFu;

struct BudgetBase {   // the base map and what every member shares; passed by value
  const Sec* cells; const Sec* pool;
  uint64_t cap;       // its pool capacity
  int32_t dimx, dimy;
  uint32_t bcap;      // basin records kept for each member: basins of rank < bcap
  uint32_t ntypes;    // soil records of each member (0: no soil table)
};
struct BudgetMap {    // one map of NOW; 40 bytes
  const Sec* cells; const Sec* pool;
  uint64_t cap;
  uint32_t brec0, srec0;   // its first basin record, its first soil record
  uint32_t index, pad;     // its error word is word 1 + index
};
struct BudgetPlanes { double* dground; double* dheight; int64_t* dsolid; int64_t* dwater; };   // each may be null (smx_budget only)
struct BudgetAcc {    // a basin's record while it is folded (96 bytes, as smx_budget_basin)
  uint32_t first_cell, cells;   // (the drainage record's: set when the record is finished)
  uint32_t lowered, raised, resurfaced, flags;
  uint64_t eroded, deposited, wgained, wlost;
  uint64_t cutmax, fillmax;     // the bits of a non-negative f64: ordered as the values are
  uint32_t cut_img, fill_img;   // ~cell of the smallest cell that attains it; 0: none
  uint32_t reserved[4];
};
struct BudgetBasinRec {   // == smx_budget_basin (include/soilmx.h)
  uint32_t first_cell, cells, lowered_cells, raised_cells, resurfaced_cells, flags;
  uint64_t eroded_q40, deposited_q40, water_gained_q40, water_lost_q40;
  double cut_max, fill_max;
  uint32_t cut_cell, fill_cell;
  uint32_t reserved[4];
};
struct BudgetSoilRec {    // == smx_budget_soil (include/soilmx.h); also the record while it is folded
  uint64_t gained_q40, lost_q40, held_gained_q40, held_lost_q40;
  uint32_t cells_gained, cells_lost, surfaced, covered, flags;
  uint32_t reserved[3];
};
static_assert(sizeof(BudgetMap) == 40 && sizeof(BudgetAcc) == 96 && sizeof(BudgetBasinRec) == 96 && sizeof(BudgetSoilRec) == 64, "budget record layouts");

SMX_HD uint64_t budget_bits(double v) { uint64_t b; __builtin_memcpy(&b, &v, 8); return b; }
SMX_HD double budget_unbits(uint64_t b) { double v; __builtin_memcpy(&v, &b, 8); return v; }
SMX_HD void budget_finish(const BasinAcc& b, const BudgetAcc& a, BudgetBasinRec& r) {
  r.first_cell = b.first_cell; r.cells = b.cells;
  r.lowered_cells = a.lowered; r.raised_cells = a.raised; r.resurfaced_cells = a.resurfaced; r.flags = a.flags;
  r.eroded_q40 = a.eroded; r.deposited_q40 = a.deposited; r.water_gained_q40 = a.wgained; r.water_lost_q40 = a.wlost;
  r.cut_max = budget_unbits(a.cutmax); r.fill_max = budget_unbits(a.fillmax);
  r.cut_cell = a.cut_img ? ~a.cut_img : BUDGET_NONE; r.fill_cell = a.fill_img ? ~a.fill_img : BUDGET_NONE;
  r.reserved[0] = r.reserved[1] = r.reserved[2] = r.reserved[3] = 0u;
}
SMX_D double budget_ground(const Sec& s) { return s.type == EMPTY ? 0.0 : (s.type == AIR ? s.floor : s.floor + s.size); }
SMX_HD uint32_t budget_tiles(int dimx, int dimy, int tx, int ty) { return (uint32_t)((dimx + tx - 1) / tx) * (uint32_t)((dimy + ty - 1) / ty); }

// ---- a column's walk: the section it stands on, the links it has followed
struct BudgetWalk {
  Sec s;
  uint64_t links;
  bool live, bad;
};
SMX_D void budget_start(const Sec* cells, uint64_t c, BudgetWalk& w) {
  w.s = cells[c]; w.links = 0ull; w.bad = false; w.live = w.s.type != EMPTY;
}
// where the section below w.s lies: null at the bottom of the column, or on a link that leaves the pool / one link more than the
// pool holds (strata_down's rule)
SMX_D const Sec* budget_below(const Sec* pool, uint64_t cap, BudgetWalk& w) {
  const uint32_t pv = w.s.prev;
  if (!w.live || pv == NIL) return nullptr;
  if (pv >= cap || w.links >= cap) { w.bad = true; return nullptr; }
  w.links++;
  return pool + pv;
}

// the sums of one column: the private types' V and H, S, and the flags that go to the private types' records and to the basin's
struct BudgetCol {
  uint64_t v[BUDGET_PRIV], h[BUDGET_PRIV], solid;
  uint32_t pf[BUDGET_PRIV], fb;
};
SMX_D void budget_col_zero(BudgetCol& a) {
#pragma unroll
  for (int k = 0; k < BUDGET_PRIV; k++) { a.v[k] = 0ull; a.h[k] = 0ull; a.pf[k] = 0u; }
  a.solid = 0ull; a.fb = 0u;
}
// one section into its column's sums; a type in [BUDGET_PRIV, ntypes) is noted in `rest`
SMX_D void budget_take(const Sec& s, uint32_t ntypes, BudgetCol& a, uint64_t& rest) {
  const uint32_t ty = s.type;
  uint32_t f = 0u;
  const uint64_t qv = strata_q40(s.size, BUDGET_F_TERM, f);
  a.fb |= f;
  if (ty != AIR) {
    if (a.solid + qv < qv) a.fb |= BUDGET_F_WRAP;
    a.solid += qv;
  }
  if (ty < (uint32_t)BUDGET_PRIV) {
    const uint64_t qh = strata_q40(s.size * s.sat, BUDGET_F_TERM, f);
#pragma unroll
    for (int k = 0; k < BUDGET_PRIV; k++) {
      if (ty != (uint32_t)k) continue;
      if (a.v[k] + qv < qv) { f |= BUDGET_F_WRAP; if (k == 0) a.fb |= BUDGET_F_WRAP; }
      if (a.h[k] + qh < qh) f |= BUDGET_F_WRAP;
      a.v[k] += qv; a.h[k] += qh; a.pf[k] |= f;
    }
  } else if (ty < ntypes) {
    rest |= 1ull << ty;
  }
}
// V and H of ONE type over a column whose chain the first walk found good
SMX_D void budget_one_type(const Sec* cells, const Sec* pool, uint64_t cap, uint64_t c, uint32_t ty, uint64_t& v, uint64_t& h, uint32_t& f) {
  BudgetWalk w;
  budget_start(cells, c, w);
  while (w.live) {
    if (w.s.type == ty) {
      const uint64_t qv = strata_q40(w.s.size, BUDGET_F_TERM, f), qh = strata_q40(w.s.size * w.s.sat, BUDGET_F_TERM, f);
      if (v + qv < qv || h + qh < qh) f |= BUDGET_F_WRAP;
      v += qv; h += qh;
    }
    const Sec* p = budget_below(pool, cap, w);
    w.live = p != nullptr;
    if (p) w.s = *p;
  }
}

// ---- the LDS tables of a workgroup: a slot per basin met in its tile (SLOTS >= the tile's cells), an entry per soil type
template <int SLOTS>
struct BudgetBasinTable {
  uint64_t eroded[SLOTS], deposited[SLOTS], wgained[SLOTS], wlost[SLOTS], cutmax[SLOTS], fillmax[SLOTS];
  uint32_t key[SLOTS], lowered[SLOTS], raised[SLOTS], resurfaced[SLOTS], flags[SLOTS];
};
struct BudgetSoilTable {
  uint64_t gained[BUDGET_MAX_TYPES], lost[BUDGET_MAX_TYPES], hgained[BUDGET_MAX_TYPES], hlost[BUDGET_MAX_TYPES];
  uint32_t cells_gained[BUDGET_MAX_TYPES], cells_lost[BUDGET_MAX_TYPES], surfaced[BUDGET_MAX_TYPES], covered[BUDGET_MAX_TYPES], flags[BUDGET_MAX_TYPES];
};
// one cell's change of type ty into the workgroup's soil table
SMX_D void budget_soil_cell(BudgetSoilTable& t, uint32_t ty, uint64_t vn, uint64_t vb, uint64_t hn, uint64_t hb, uint32_t f) {
  if (vn > vb) { strata_sum<SMX_STRATA_WG>(t.gained + ty, vn - vb, BUDGET_F_WRAP, f); SMX_LAKE_ADD(t.cells_gained + ty, 1u, SMX_LAKE_WG); }
  if (vn < vb) { strata_sum<SMX_STRATA_WG>(t.lost + ty, vb - vn, BUDGET_F_WRAP, f); SMX_LAKE_ADD(t.cells_lost + ty, 1u, SMX_LAKE_WG); }
  if (hn > hb) strata_sum<SMX_STRATA_WG>(t.hgained + ty, hn - hb, BUDGET_F_WRAP, f);
  if (hn < hb) strata_sum<SMX_STRATA_WG>(t.hlost + ty, hb - hn, BUDGET_F_WRAP, f);
  if (f) SMX_LAKE_OR(t.flags + ty, f, SMX_LAKE_WG);
}

// ---- fold: workgroup `tile` of the base's tiles on member m. T: the rank plane of the base (read only); acc, soils: the records of
//      ALL members; bad: the error words. The planes are written for every cell with good chains, whatever bcap is.
//      Three stretches with a barrier between them (tests/budget_host runs each with the lanes in the order it likes): the tables
//      cleared, the cells folded, the tables flushed.
template <int SLOTS, class G>
SMX_D void budget_fold_clear(G& g, BudgetBasinTable<SLOTS>& bt, BudgetSoilTable& st) {
  const uint32_t nl = g.lanes();
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    for (uint32_t s = l; s < (uint32_t)SLOTS; s += nl) {
      bt.key[s] = LAKE_DRY; bt.lowered[s] = 0u; bt.raised[s] = 0u; bt.resurfaced[s] = 0u; bt.flags[s] = 0u;
      bt.eroded[s] = 0ull; bt.deposited[s] = 0ull; bt.wgained[s] = 0ull; bt.wlost[s] = 0ull; bt.cutmax[s] = 0ull; bt.fillmax[s] = 0ull;
    }
    for (uint32_t i = l; i < (uint32_t)BUDGET_MAX_TYPES; i += nl) {
      st.gained[i] = 0ull; st.lost[i] = 0ull; st.hgained[i] = 0ull; st.hlost[i] = 0ull;
      st.cells_gained[i] = 0u; st.cells_lost[i] = 0u; st.surfaced[i] = 0u; st.covered[i] = 0u; st.flags[i] = 0u;
    }
  }
}
template <int TX, int TY, int SLOTS, class G>
SMX_D void budget_fold_cells(const BudgetBase& b, const BudgetMap& m, G& g, uint32_t tile, BudgetBasinTable<SLOTS>& bt, BudgetSoilTable& st, const uint32_t* T,
                             uint64_t* bad, const BudgetPlanes& pl) {
  static_assert(SLOTS >= TX * TY, "a slot for every cell of the tile");
  const uint32_t nl = g.lanes();
  const int nty = (b.dimy + TY - 1) / TY;
  const int x0 = (int)(tile / (uint32_t)nty) * TX, y0 = (int)(tile % (uint32_t)nty) * TY;
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    for (uint32_t i = l; i < (uint32_t)(TX * TY); i += nl) {   // (y runs fastest: adjacent lanes, adjacent records)
      const int x = x0 + (int)(i / TY), y = y0 + (int)(i % TY);
      if (x >= b.dimx || y >= b.dimy) continue;
      const uint64_t c = (uint64_t)x * (uint64_t)b.dimy + (uint64_t)y;
      BudgetWalk wn, wb;
      budget_start(m.cells, c, wn);
      budget_start(b.cells, c, wb);
      const Sec topn = wn.s, topb = wb.s;
      BudgetCol cn, cb;
      budget_col_zero(cn); budget_col_zero(cb);
      uint64_t rest = 0ull;
      while (wn.live || wb.live) {
        // both next links first: two independent loads in flight while the two current sections are folded
        const Sec* pn = budget_below(m.pool, m.cap, wn);
        const Sec* pb = budget_below(b.pool, b.cap, wb);
        Sec nn = wn.s, nb = wb.s;
        if (pn) nn = *pn;
        if (pb) nb = *pb;
        if (wn.live) budget_take(wn.s, b.ntypes, cn, rest);
        if (wb.live) budget_take(wb.s, b.ntypes, cb, rest);
        wn.live = pn != nullptr; wn.s = nn;
        wb.live = pb != nullptr; wb.s = nb;
      }
      if (wb.bad) strata_report(bad, c);
      if (wn.bad) strata_report(bad + 1u + m.index, c);
      if (wn.bad || wb.bad) continue;
      // per cell
      const double gn = budget_ground(topn), gb = budget_ground(topb), dg = gn - gb;
      const bool lower = gn < gb, raise = gn > gb, nan = gn != gn || gb != gb, resurf = topn.type != topb.type;
      if (pl.dground) pl.dground[c] = dg;
      if (pl.dheight) pl.dheight[c] = drain_height(topn) - drain_height(topb);
      if (pl.dsolid) pl.dsolid[c] = (int64_t)(cn.solid - cb.solid);
      if (pl.dwater) pl.dwater[c] = (int64_t)(cn.v[0] - cb.v[0]);
      // per soil type
      if (b.ntypes) {
#pragma unroll
        for (int k = 0; k < BUDGET_PRIV; k++)
          if ((uint32_t)k < b.ntypes) budget_soil_cell(st, (uint32_t)k, cn.v[k], cb.v[k], cn.h[k], cb.h[k], cn.pf[k] | cb.pf[k]);
        while (rest) {   // the types beyond the registers: one more walk of the two columns for each
          const uint32_t ty = (uint32_t)__builtin_ctzll(rest);
          rest &= rest - 1ull;
          uint64_t vn = 0ull, vb = 0ull, hn = 0ull, hb = 0ull;
          uint32_t f = 0u;
          budget_one_type(m.cells, m.pool, m.cap, c, ty, vn, hn, f);
          budget_one_type(b.cells, b.pool, b.cap, c, ty, vb, hb, f);
          budget_soil_cell(st, ty, vn, vb, hn, hb, f);
        }
        if (resurf) {
          if (topn.type < b.ntypes) SMX_LAKE_ADD(st.surfaced + topn.type, 1u, SMX_LAKE_WG);
          if (topb.type < b.ntypes) SMX_LAKE_ADD(st.covered + topb.type, 1u, SMX_LAKE_WG);
        }
      }
      // per basin
      const uint32_t rank = T[c];
      if (rank >= b.bcap) continue;
      uint32_t s = (rank * 2654435761u) % (uint32_t)SLOTS;
      for (;;) {   // (at most TX * TY keys are ever inserted: a free or matching slot exists)
        const uint32_t k = SMX_LAKE_CAS(bt.key + s, LAKE_DRY, rank, SMX_LAKE_WG);
        if (k == LAKE_DRY || k == rank) break;
        s = s + 1u == (uint32_t)SLOTS ? 0u : s + 1u;
      }
      uint32_t f = cn.fb | cb.fb | (nan ? BUDGET_F_NAN : 0u);
      if (lower) { SMX_LAKE_ADD(bt.lowered + s, 1u, SMX_LAKE_WG); SMX_LAKE_MAX(bt.cutmax + s, budget_bits(-dg), SMX_LAKE_WG); }
      if (raise) { SMX_LAKE_ADD(bt.raised + s, 1u, SMX_LAKE_WG); SMX_LAKE_MAX(bt.fillmax + s, budget_bits(dg), SMX_LAKE_WG); }
      if (resurf) SMX_LAKE_ADD(bt.resurfaced + s, 1u, SMX_LAKE_WG);
      if (cb.solid > cn.solid) strata_sum<SMX_STRATA_WG>(bt.eroded + s, cb.solid - cn.solid, BUDGET_F_WRAP, f);
      if (cn.solid > cb.solid) strata_sum<SMX_STRATA_WG>(bt.deposited + s, cn.solid - cb.solid, BUDGET_F_WRAP, f);
      if (cn.v[0] > cb.v[0]) strata_sum<SMX_STRATA_WG>(bt.wgained + s, cn.v[0] - cb.v[0], BUDGET_F_WRAP, f);
      if (cb.v[0] > cn.v[0]) strata_sum<SMX_STRATA_WG>(bt.wlost + s, cb.v[0] - cn.v[0], BUDGET_F_WRAP, f);
      if (f) SMX_LAKE_OR(bt.flags + s, f, SMX_LAKE_WG);
    }
  }
}
template <int SLOTS, class G>
SMX_D void budget_fold_flush(const BudgetBase& b, const BudgetMap& m, G& g, BudgetBasinTable<SLOTS>& bt, BudgetSoilTable& st, BudgetAcc* acc, BudgetSoilRec* soils) {
  const uint32_t nl = g.lanes();
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    for (uint32_t s = l; s < (uint32_t)SLOTS; s += nl) {
      if (bt.key[s] == LAKE_DRY) continue;
      BudgetAcc& r = acc[(size_t)m.brec0 + bt.key[s]];
      uint32_t f = bt.flags[s];
      if (bt.lowered[s]) SMX_LAKE_ADD(&r.lowered, bt.lowered[s], SMX_LAKE_AGENT);
      if (bt.raised[s]) SMX_LAKE_ADD(&r.raised, bt.raised[s], SMX_LAKE_AGENT);
      if (bt.resurfaced[s]) SMX_LAKE_ADD(&r.resurfaced, bt.resurfaced[s], SMX_LAKE_AGENT);
      strata_sum<SMX_STRATA_AGENT>(&r.eroded, bt.eroded[s], BUDGET_F_WRAP, f);
      strata_sum<SMX_STRATA_AGENT>(&r.deposited, bt.deposited[s], BUDGET_F_WRAP, f);
      strata_sum<SMX_STRATA_AGENT>(&r.wgained, bt.wgained[s], BUDGET_F_WRAP, f);
      strata_sum<SMX_STRATA_AGENT>(&r.wlost, bt.wlost[s], BUDGET_F_WRAP, f);
      if (bt.cutmax[s]) SMX_LAKE_MAX(&r.cutmax, bt.cutmax[s], SMX_LAKE_AGENT);
      if (bt.fillmax[s]) SMX_LAKE_MAX(&r.fillmax, bt.fillmax[s], SMX_LAKE_AGENT);
      if (f) SMX_LAKE_OR(&r.flags, f, SMX_LAKE_AGENT);
    }
    for (uint32_t i = l; i < b.ntypes; i += nl) {
      BudgetSoilRec& r = soils[(size_t)m.srec0 + i];
      uint32_t f = st.flags[i];
      strata_sum<SMX_STRATA_AGENT>(&r.gained_q40, st.gained[i], BUDGET_F_WRAP, f);
      strata_sum<SMX_STRATA_AGENT>(&r.lost_q40, st.lost[i], BUDGET_F_WRAP, f);
      strata_sum<SMX_STRATA_AGENT>(&r.held_gained_q40, st.hgained[i], BUDGET_F_WRAP, f);
      strata_sum<SMX_STRATA_AGENT>(&r.held_lost_q40, st.hlost[i], BUDGET_F_WRAP, f);
      if (st.cells_gained[i]) SMX_LAKE_ADD(&r.cells_gained, st.cells_gained[i], SMX_LAKE_AGENT);
      if (st.cells_lost[i]) SMX_LAKE_ADD(&r.cells_lost, st.cells_lost[i], SMX_LAKE_AGENT);
      if (st.surfaced[i]) SMX_LAKE_ADD(&r.surfaced, st.surfaced[i], SMX_LAKE_AGENT);
      if (st.covered[i]) SMX_LAKE_ADD(&r.covered, st.covered[i], SMX_LAKE_AGENT);
      if (f) SMX_LAKE_OR(&r.flags, f, SMX_LAKE_AGENT);
    }
  }
}
template <int TX, int TY, int SLOTS, class G>
SMX_D void budget_fold_group(const BudgetBase& b, const BudgetMap& m, G& g, uint32_t tile, BudgetBasinTable<SLOTS>& bt, BudgetSoilTable& st, const uint32_t* T,
                             BudgetAcc* acc, BudgetSoilRec* soils, uint64_t* bad, const BudgetPlanes& pl) {
  budget_fold_clear(g, bt, st);
  g.barrier();
  budget_fold_cells<TX, TY>(b, m, g, tile, bt, st, T, bad, pl);
  g.barrier();
  budget_fold_flush(b, m, g, bt, st, acc, soils);
}

// ---- where: workgroup `block` takes g.lanes() cells of member m, behind the fold (the extremes are final; only the top records are read)
template <class G>
SMX_D void budget_where_group(const BudgetBase& b, const BudgetMap& m, G& g, uint32_t block, const uint32_t* T, BudgetAcc* acc) {
  const uint32_t nl = g.lanes();
  const uint64_t n = (uint64_t)b.dimx * (uint64_t)b.dimy;
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    const uint64_t c = (uint64_t)block * nl + l;
    if (c >= n) continue;
    const uint32_t rank = T[c];
    if (rank >= b.bcap) continue;
    const double gn = budget_ground(m.cells[c]), gb = budget_ground(b.cells[c]), dg = gn - gb;
    BudgetAcc& r = acc[(size_t)m.brec0 + rank];
    if (gn < gb && budget_bits(-dg) == r.cutmax) SMX_LAKE_MAX(&r.cut_img, ~(uint32_t)c, SMX_LAKE_AGENT);
    if (gn > gb && budget_bits(dg) == r.fillmax) SMX_LAKE_MAX(&r.fill_img, ~(uint32_t)c, SMX_LAKE_AGENT);
  }
}

}  // namespace smx
