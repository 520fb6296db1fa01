// soil_strata.h -- reading the strata on the device (smx_soil_totals / smx_ensemble_soil_totals, smx_soil_thickness, smx_cores): the
// bodies of k_strata_totals, k_strata_thickness, k_core_count and k_core_scatter. Nothing here writes a map.
//
// A column is walked TOP -> BOTTOM: the top section inline in the cell record, then the `prev` links into the pool. Every link is
// validated as the fork's count pass validates it (prev < pool capacity, no more links than the pool holds); a column that fails
// ends its walk and reports its cell through one max on the image ~cell of the member's error word (0: no bad cell, else ~ of the
// LOWEST bad cell). One lane takes one column; a workgroup strides over the map, so a deep column holds up its own wavefront only.
//   totals     per type < ntypes: sections, cells (columns holding the type: one bit per type in a 64-bit mask), top_cells, and two
//              exact integer sums, floor(size * 2^40) and floor((size * sat) * 2^40). Types 0..STRATA_PRIV-1 are folded in the lane's
//              registers (chosen by unrolled compares, never an indexed array), the others by workgroup-scope atomics on a table in
//              LDS; at the end of its columns a lane adds its registers to the same table, and lane t of the workgroup issues one
//              agent-scope add per non-zero field of type t. Only integers are added and a wrap is detected on every add, so no
//              result depends on the launch shape: the wraps seen over any order of adds number floor(true sum / 2^64).
//              volume_q40 * 2^-40 lies below the exact sum of the sizes by less than sections * 2^-40 (each floor drops less than
//              one unit); a section smaller than 2^-40 contributes 0.
//   thickness  for up to 8 listed types, ONE walk: thickness (the sizes of the type's sections summed in walk order from +0.0), cover
//              (the running sum of ALL sizes before the type's highest section is added; -1.0 without one) and the section count.
//              f64 without contraction: a host loop over the exported column, reversed, gives the same bits. Planes are type-major.
//   cores      count (sections of each listed cell), an exclusive scan (the caller's business: rocPRIM on the device, a loop in
//              tests/strata_host), scatter (section j from the top of list entry i goes to base[i] + count[i] - 1 - j: bottom -> top,
//              the snapshot layout).
// The file compiles for the device and, under SMX_D / SMX_HOSTSIM, for the host (tests/strata_host runs the same bodies with the
// lanes of a workgroup looped), with the group object of soil_observe.h: lanes(), lo(), hi(), barrier().
#pragma once
#include "soil_core.h"

#ifdef SMX_HOSTSIM
namespace smx {
// (one lane after the other: a read-modify-write is a read and a write)
template <class T> inline T strata_hs_add(T* p, T v) { const T o = *p; *p = (T)(o + v); return o; }
template <class T> inline T strata_hs_or(T* p, T v) { const T o = *p; *p = (T)(o | v); return o; }
template <class T> inline T strata_hs_max(T* p, T v) { const T o = *p; if (v > o) *p = v; return o; }
}  // namespace smx
#define SMX_STRATA_WG 0
#define SMX_STRATA_AGENT 0
#define SMX_STRATA_ADD(p, v, scope) smx::strata_hs_add((p), (v))
#define SMX_STRATA_OR(p, v, scope) smx::strata_hs_or((p), (v))
#define SMX_STRATA_MAX(p, v, scope) smx::strata_hs_max((p), (v))
#else
#define SMX_STRATA_WG __HIP_MEMORY_SCOPE_WORKGROUP
#define SMX_STRATA_AGENT __HIP_MEMORY_SCOPE_AGENT
#define SMX_STRATA_ADD(p, v, scope) __hip_atomic_fetch_add((p), (v), __ATOMIC_RELAXED, scope)
#define SMX_STRATA_OR(p, v, scope) __hip_atomic_fetch_or((p), (v), __ATOMIC_RELAXED, scope)
#define SMX_STRATA_MAX(p, v, scope) __hip_atomic_fetch_max((p), (v), __ATOMIC_RELAXED, scope)
#endif

namespace smx {

constexpr int STRATA_MAX_TYPES = 64;   // == SMX_TOTALS_MAX_TYPES: one bit per type in the "seen in this column" mask
constexpr int STRATA_PRIV = 4;         // types folded in a lane's registers
constexpr int STRATA_MAX_LIST = 8;     // types of one thickness call
#ifndef SMX_STRATA_WG_LANES
#define SMX_STRATA_WG_LANES 64         // (an experiment build may widen the workgroup: profiles/r12_strata.md)
#endif
constexpr int STRATA_LANES = SMX_STRATA_WG_LANES;   // a workgroup is one wavefront
constexpr uint32_t STRATA_F_VOLUME = 1u, STRATA_F_HELD = 2u;

struct StrataMap {    // one map of a call, read only; 40 bytes
  const Sec* cells; const Sec* pool;
  uint64_t cap;       // its pool capacity: the bound of its links
  uint64_t ncells;
  uint32_t rec0;      // totals: its first record
  uint32_t index;     // totals: its error word and its count of other sections
};
struct StrataRec {    // == smx_soil_total (include/soilmx.h); also the record while it is folded
  uint64_t sections, cells, top_cells, volume_q40, held_q40;
  uint32_t flags, reserved;
};
struct StrataTable {  // the workgroup's partial records (LDS)
  uint64_t sections[STRATA_MAX_TYPES], cells[STRATA_MAX_TYPES], top_cells[STRATA_MAX_TYPES], volume[STRATA_MAX_TYPES], held[STRATA_MAX_TYPES];
  uint64_t other;
  uint32_t flags[STRATA_MAX_TYPES];
};
struct StrataTypes { uint32_t t[STRATA_MAX_LIST]; uint32_t n; };
static_assert(sizeof(StrataMap) == 40 && sizeof(StrataRec) == 48, "strata record layouts");

// the section below s: false at the bottom of the column, or on a link that leaves the pool / one link more than the pool holds
SMX_D bool strata_down(const StrataMap& m, Sec& s, uint64_t& links, bool& bad) {
  const uint32_t pv = s.prev;
  if (pv == NIL) return false;
  if (pv >= m.cap || links >= m.cap) { bad = true; return false; }
  links++;
  s = m.pool[pv];
  return true;
}
SMX_D void strata_report(uint64_t* bad, uint64_t c) { SMX_STRATA_MAX(bad, ~c, SMX_STRATA_AGENT); }
// the lowest bad cell of an error word (only where the word is not 0)
SMX_HD uint64_t strata_bad_cell(uint64_t word) { return ~word; }

// floor(v * 2^40); a term that is not finite, is negative (-0 is 0) or is >= 2^24 contributes 0 and raises `bit`
SMX_HD uint64_t strata_q40(double v, uint32_t bit, uint32_t& flags) {
  if (!(v >= 0.0) || !(v < 16777216.0)) { flags |= bit; return 0ull; }
  return (uint64_t)floor(v * 1099511627776.0);
}
// *p += v where v != 0, on the table (WG) or a record (AGENT); a wrap raises `bit`
template <int SCOPE>
SMX_D void strata_sum(uint64_t* p, uint64_t v, uint32_t bit, uint32_t& flags) {
  if (!v) return;
  const uint64_t o = SMX_STRATA_ADD(p, v, SCOPE);
  if (o + v < o) flags |= bit;
}

// ---- totals: workgroup `block` of `nblocks` strides over the columns of m; acc: the records of ALL maps, other / bad: one word per map ----
template <class G>
SMX_D void strata_totals_group(const StrataMap& m, G& g, uint64_t block, uint64_t nblocks, uint32_t ntypes, StrataTable& t, StrataRec* acc, uint64_t* other,
                               uint64_t* bad) {
  const uint32_t nl = g.lanes();
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    for (uint32_t i = l; i < (uint32_t)STRATA_MAX_TYPES; i += nl) {
      t.sections[i] = 0ull; t.cells[i] = 0ull; t.top_cells[i] = 0ull; t.volume[i] = 0ull; t.held[i] = 0ull; t.flags[i] = 0u;
    }
    if (l == 0) t.other = 0ull;
  }
  g.barrier();
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    uint64_t ps[STRATA_PRIV], pc[STRATA_PRIV], pt[STRATA_PRIV], pv[STRATA_PRIV], ph[STRATA_PRIV], oth = 0ull;
    uint32_t pf[STRATA_PRIV];
#pragma unroll
    for (int k = 0; k < STRATA_PRIV; k++) { ps[k] = 0ull; pc[k] = 0ull; pt[k] = 0ull; pv[k] = 0ull; ph[k] = 0ull; pf[k] = 0u; }
    for (uint64_t c = block * nl + l; c < m.ncells; c += nblocks * nl) {
      Sec s = m.cells[c];
      if (s.type == EMPTY) continue;
      if (s.type < ntypes) {
        if (s.type < (uint32_t)STRATA_PRIV) {
#pragma unroll
          for (int k = 0; k < STRATA_PRIV; k++) if (s.type == (uint32_t)k) pt[k]++;
        } else {
          SMX_STRATA_ADD(t.top_cells + s.type, (uint64_t)1, SMX_STRATA_WG);
        }
      }
      uint64_t seen = 0ull, links = 0ull;
      bool broken = false;
      do {
        const uint32_t ty = s.type;
        if (ty >= ntypes) { oth++; continue; }
        uint32_t f = 0u;
        const uint64_t qv = strata_q40(s.size, STRATA_F_VOLUME, f), qh = strata_q40(s.size * s.sat, STRATA_F_HELD, f);
        const uint64_t bit = 1ull << ty;
        if (ty < (uint32_t)STRATA_PRIV) {
#pragma unroll
          for (int k = 0; k < STRATA_PRIV; k++) {
            if (ty != (uint32_t)k) continue;
            ps[k]++;
            if (pv[k] + qv < qv) f |= STRATA_F_VOLUME;
            if (ph[k] + qh < qh) f |= STRATA_F_HELD;
            pv[k] += qv; ph[k] += qh; pf[k] |= f;
          }
        } else {
          SMX_STRATA_ADD(t.sections + ty, (uint64_t)1, SMX_STRATA_WG);
          if (!(seen & bit)) SMX_STRATA_ADD(t.cells + ty, (uint64_t)1, SMX_STRATA_WG);
          strata_sum<SMX_STRATA_WG>(t.volume + ty, qv, STRATA_F_VOLUME, f);
          strata_sum<SMX_STRATA_WG>(t.held + ty, qh, STRATA_F_HELD, f);
          if (f) SMX_STRATA_OR(t.flags + ty, f, SMX_STRATA_WG);
        }
        seen |= bit;
      } while (strata_down(m, s, links, broken));
#pragma unroll
      for (int k = 0; k < STRATA_PRIV; k++) pc[k] += (seen >> k) & 1ull;
      if (broken) strata_report(bad + m.index, c);
    }
#pragma unroll
    for (int k = 0; k < STRATA_PRIV; k++) {
      if (ps[k]) SMX_STRATA_ADD(t.sections + k, ps[k], SMX_STRATA_WG);
      if (pc[k]) SMX_STRATA_ADD(t.cells + k, pc[k], SMX_STRATA_WG);
      if (pt[k]) SMX_STRATA_ADD(t.top_cells + k, pt[k], SMX_STRATA_WG);
      strata_sum<SMX_STRATA_WG>(t.volume + k, pv[k], STRATA_F_VOLUME, pf[k]);
      strata_sum<SMX_STRATA_WG>(t.held + k, ph[k], STRATA_F_HELD, pf[k]);
      if (pf[k]) SMX_STRATA_OR(t.flags + k, pf[k], SMX_STRATA_WG);
    }
    if (oth) SMX_STRATA_ADD(&t.other, oth, SMX_STRATA_WG);
  }
  g.barrier();
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    if (l == 0 && t.other) SMX_STRATA_ADD(other + m.index, t.other, SMX_STRATA_AGENT);
    for (uint32_t i = l; i < ntypes; i += nl) {
      StrataRec& r = acc[(size_t)m.rec0 + i];
      uint32_t f = t.flags[i];
      if (t.sections[i]) SMX_STRATA_ADD(&r.sections, t.sections[i], SMX_STRATA_AGENT);
      if (t.cells[i]) SMX_STRATA_ADD(&r.cells, t.cells[i], SMX_STRATA_AGENT);
      if (t.top_cells[i]) SMX_STRATA_ADD(&r.top_cells, t.top_cells[i], SMX_STRATA_AGENT);
      strata_sum<SMX_STRATA_AGENT>(&r.volume_q40, t.volume[i], STRATA_F_VOLUME, f);
      strata_sum<SMX_STRATA_AGENT>(&r.held_q40, t.held[i], STRATA_F_HELD, f);
      if (f) SMX_STRATA_OR(&r.flags, f, SMX_STRATA_AGENT);
    }
  }
}

// ---- thickness: the planes hold ty.n * ncells values, [k * ncells + c]; each may be null ----
template <class G>
SMX_D void strata_thickness_group(const StrataMap& m, G& g, uint64_t block, uint64_t nblocks, const StrataTypes& ty, double* thickness, double* cover,
                                  uint32_t* sections, uint64_t* bad) {
  const uint32_t nl = g.lanes();
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    for (uint64_t c = block * nl + l; c < m.ncells; c += nblocks * nl) {
      double th[STRATA_MAX_LIST], cv[STRATA_MAX_LIST], run = 0.0;
      uint32_t n[STRATA_MAX_LIST];
#pragma unroll
      for (int k = 0; k < STRATA_MAX_LIST; k++) { th[k] = 0.0; cv[k] = -1.0; n[k] = 0u; }
      Sec s = m.cells[c];
      uint64_t links = 0ull;
      bool broken = false;
      if (s.type != EMPTY) {
        do {
#pragma unroll
          for (int k = 0; k < STRATA_MAX_LIST; k++) {
            if ((uint32_t)k >= ty.n || s.type != ty.t[k]) continue;
            if (n[k] == 0u) cv[k] = run;
            th[k] += s.size; n[k]++;
          }
          run += s.size;
        } while (strata_down(m, s, links, broken));
      }
      if (broken) { strata_report(bad, c); continue; }
#pragma unroll
      for (int k = 0; k < STRATA_MAX_LIST; k++) {
        if ((uint32_t)k >= ty.n) continue;
        const size_t at = (size_t)k * (size_t)m.ncells + (size_t)c;
        if (thickness) thickness[at] = th[k];
        if (cover) cover[at] = cv[k];
        if (sections) sections[at] = n[k];
      }
    }
  }
}

// ---- cores: list entry i is cell list[i] of m (the caller has checked it against ncells) ----
template <class G>
SMX_D void core_count_group(const StrataMap& m, G& g, uint64_t block, uint64_t nblocks, const uint32_t* list, uint64_t n, uint32_t* count, uint64_t* bad) {
  const uint32_t nl = g.lanes();
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    for (uint64_t i = block * nl + l; i < n; i += nblocks * nl) {
      const uint64_t c = list[i];
      Sec s = m.cells[c];
      uint64_t links = 0ull;
      uint32_t k = 0u;
      bool broken = false;
      if (s.type != EMPTY) {
        do k++; while (strata_down(m, s, links, broken));
      }
      count[i] = k;
      if (broken) strata_report(bad, c);
    }
  }
}
// `room`: sections the four arrays hold (the count pass validated the chains; a map that changed under the call must not write out of bounds)
template <class G>
SMX_D void core_scatter_group(const StrataMap& m, G& g, uint64_t block, uint64_t nblocks, const uint32_t* list, uint64_t n, const uint32_t* count,
                              const uint64_t* base, uint64_t room, uint32_t* type, double* size, double* floor, double* sat) {
  const uint32_t nl = g.lanes();
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    for (uint64_t i = block * nl + l; i < n; i += nblocks * nl) {
      const uint32_t k = count[i];
      if (k == 0u) continue;
      Sec s = m.cells[list[i]];
      uint64_t links = 0ull;
      bool broken = false;
      for (uint32_t j = 0; j < k; j++) {
        const uint64_t at = base[i] + (uint64_t)(k - 1u - j);
        if (at >= room) break;
        type[at] = s.type; size[at] = s.size; floor[at] = s.floor; sat[at] = s.sat;
        if (!strata_down(m, s, links, broken)) break;
      }
    }
  }
}
// the scan's input (the caller's iterator on the device, its loop on the host)
SMX_HD uint64_t core_widen(const uint32_t* count, size_t i) { return (uint64_t)count[i]; }

}  // namespace smx
