// soil_prox.h -- proximity (smx_proximity / smx_ensemble_proximity): the exact Euclidean distance transform of a set of SITES, which
// site is nearest to every cell, the zone of every group of sites and, where asked for, how much of each zone lies how far out
// (buffers). The bodies of k_prox_mark, k_prox_columns, k_prox_envelope, k_prox_query and k_prox_hist; in WATER mode the labelling
// and the rank scan in front of them are the census's (soil_lakes.h), unchanged. Nothing here writes a map.
//
// Cells, c = x*dimy + y, wet cells, lakes and their ranks are those of soil_lakes.h. The SITES are a set of cells, each with a GROUP:
// in LIST mode the n >= 1 distinct cells of the caller's list, site list[i] in group i; in WATER mode the wet cells, each in the group
// that is its lake's rank. d2(c, s) = (xc - xs)^2 + (yc - ys)^2; nearest(c) is the site with the smallest (d2(c, s), s) -- the smaller
// squared distance, then the smaller cell index --; dist2(c) = d2(c, nearest(c)); group(c) = group(nearest(c)). Without a site all
// three are PROX_NONE. The ZONE of group g is the set of cells with group(c) == g. r(c) is the integer with r^2 <= dist2 < (r+1)^2; a
// cell of zone g counts in bin min(r / bin_width, nbins - 1) of row g.
//
// The transform is separable (Meijster, Roerdink, Hesselink 2000), on u32 planes that all members share, member i at words [off_i,
// off_i + cells_i):
//   mark      M[c] = the group at a site, PROX_NONE elsewhere. LIST: M is PROX_NONE everywhere (the caller's fill) and one lane per
//             list entry writes its position; the caller has refused duplicates, so no two lanes write the same word. WATER: M holds
//             the flattened roots of the census's labelling and B the scan of the root marks; one lane per cell turns its own word
//             into the rank B[root] - B[off] (as k_lake_stats does), and the last cell's lane writes the number of lakes. The same
//             workgroups set the member's records to the fold's identities.
//   columns   a workgroup per column x -- the direction that is contiguous in memory. P[x, y] = the site row y' of column x with the
//             smallest (|y - y'|, y'), PROX_NONE in a column without a site. The column's sites become a bit mask in LDS (a bit per
//             row); every 64-row word learns the last site below it and the first above it; every cell then looks at its own word
//             on both sides and falls back on those two. One load and one store per cell, both coalesced.
//   envelope  a lane per row y, the lanes of a wavefront on consecutive y, so that every load at equal column is one contiguous
//             stretch. Over the columns i with a candidate, g(i) = |y - P[i, y]|, the lane builds the lower envelope of the parabolas
//             f_i(x) = (x - i)^2 + g(i)^2 as a stack: S[q] = (i << 16) | g(i), T[q] = the first x the q-th parabola holds, both laid
//             out [q*dimy + y] for the same reason; D[y] = the depth. Column i holds x <= Sep(i, u) = floor((u^2 - i^2 + g(u)^2 -
//             g(i)^2) / (2(u - i))) against a later column u: there f_i(x) <= f_u(x). 64-bit integers throughout. A parabola is
//             popped when the newcomer is STRICTLY below it at its own first x; so the numerator is never negative when Sep is
//             taken, and the truncating division is the floor. BANDS: the columns are cut into `bands` stretches of
//             prox_band_width columns and every (band, row) has a lane of its own, which builds the envelope of its band's columns
//             alone -- still over all x of the row -- into the band's stretch of the stack, S and T at [(band*width + q)*dimy + y],
//             its depth in D[band*dimy + y]. The pass is bound by the latency of its dependent steps, and a band has 1 / bands of
//             them. bands == 1 is the plain scan.
//   query     a lane per cell: per band a binary search of its row's T for the segment that holds x; of the bands' candidates the
//             smallest d2, of equals the one of the lower band (a STRICT < in ascending band order), then nearest, dist2 and
//             group; the records are folded per group in an LDS table and ONE set of atomics per group and workgroup goes to the
//             record.
//   hist      (only with bins) a lane per cell, from the dist2 and group planes: an LDS table keyed by group * nbins + bin, ONE global
//             add per occupied slot and workgroup.
// Ties. nearest(c) minimises (d2, s) with s = xs*dimy + ys, that is (d2, xs, ys). Inside one column xs is fixed and d2 grows with
// |y - ys|: the column's best site is the one with the smallest (|y - ys|, ys), which is P. Between two columns i < u of equal f at
// x the envelope keeps i (x <= Sep(i, u) belongs to i, and a pop needs a strict inequality): the smaller column; between two bands
// the query keeps the lower band's, whose columns are all smaller. Together that is the smallest (d2, xs, ys).
// Every figure is an integer add or an order-free extreme ((dist2 << 32) | (0xFFFFFFFF - cell), as HorizonAcc::far); r comes from
// one f64 square root of an integer below 2^31, corrected in integers, so it is exact whatever the root's last bit. Nothing waits for
// another lane or workgroup, and no launch strides: smx_set_analysis_launch has no family for these kernels. A side is at most
// PROX_MAX_SIDE: dist2 < 2^31 keeps PROX_NONE free, a column and a g fit 16 bits each, and a column's mask fits ProxColumn.
// The file compiles for the device and, under SMX_D / SMX_HOSTSIM, for the host (tests/prox_host), as soil_catch.h does.
#pragma once
#include "soil_lakes.h"

namespace smx {

constexpr uint32_t PROX_NONE = 0xFFFFFFFFu;    // M, P: no site; nearest, group, dist2: the map has no site; the free key of the tables
constexpr uint32_t PROX_F_BORDER = 1u;         // the zone has a cell on the map border
constexpr uint32_t PROX_MAX_BINS = 64u;
constexpr uint32_t PROX_MAX_SIDE = 32768u;
constexpr uint32_t PROX_WORDS = PROX_MAX_SIDE / 64u;   // the mask words of the longest column
#ifndef SMX_PROX_BANDS
#define SMX_PROX_BANDS 8                               // (measured: profiles/r26_proximity.md; a bench build overrides it)
#endif
constexpr uint32_t PROX_BANDS = SMX_PROX_BANDS;        // the bands the library asks for
static_assert(PROX_BANDS >= 1u, "at least one band");

// the bands of a member where `want` are asked for -- at most a band per column, so that the depths fit a plane --, and their width
SMX_HD uint32_t prox_bands(const LakeMember& m, uint32_t want) { return want < 1u ? 1u : want > (uint32_t)m.dimx ? (uint32_t)m.dimx : want; }
SMX_HD uint32_t prox_band_width(const LakeMember& m, uint32_t bands) { return ((uint32_t)m.dimx + bands - 1u) / bands; }

struct ProxAcc {      // a record while it is folded (64 bytes, as smx_proximity_record)
  uint32_t site, sites, cells, flags;
  uint64_t far;       // (dist2 << 32) | (0xFFFFFFFF - cell)
  uint64_t sum;
  uint32_t x0, y0, x1, y1;
  uint32_t pad[4];
};
struct ProxRec {      // == smx_proximity_record (include/soilmx.h)
  uint32_t site, sites, cells, dist2_max, farthest_cell, flags;
  uint64_t dist2_sum;
  uint16_t x0, y0, x1, y1;
  uint32_t reserved[6];
};
static_assert(sizeof(ProxAcc) == 64 && sizeof(ProxRec) == 64, "proximity record layouts");

SMX_HD void prox_finish(const ProxAcc& a, ProxRec& r) {
  r.site = a.site; r.sites = a.sites; r.cells = a.cells;
  r.dist2_max = (uint32_t)(a.far >> 32); r.farthest_cell = 0xFFFFFFFFu - (uint32_t)a.far; r.flags = a.flags;
  r.dist2_sum = a.sum;
  r.x0 = (uint16_t)a.x0; r.y0 = (uint16_t)a.y0; r.x1 = (uint16_t)a.x1; r.y1 = (uint16_t)a.y1;
  for (uint32_t& w : r.reserved) w = 0u;
}
// r with r^2 <= d < (r+1)^2 for d < 2^31: the f64 root (exact for an integer below 2^52 up to its last bit), then put right in integers
SMX_HD uint32_t prox_root(uint32_t d) {
  uint32_t r = (uint32_t)sqrt((double)d);
  while ((uint64_t)r * r > d) r--;
  while ((uint64_t)(r + 1u) * (r + 1u) <= d) r++;
  return r;
}
SMX_HD uint32_t prox_bin(uint32_t d, uint32_t bin_width, uint32_t nbins) {
  const uint32_t b = prox_root(d) / bin_width;
  return b < nbins ? b : nbins - 1u;
}
SMX_HD uint32_t prox_mark_blocks(const LakeMember& m, bool list, uint32_t n, uint32_t lanes) {   // the workgroups k_prox_mark needs for a member
  const uint64_t items = list ? (uint64_t)n : (uint64_t)m.dimx * (uint64_t)m.dimy;
  return (uint32_t)((items + lanes - 1u) / lanes);
}

// ---- mark: workgroup `block` of `nblocks` takes g.lanes() list entries (list given) or cells (WATER: list null, M the roots, B the scan) ----
template <class G>
SMX_D void prox_mark_group(const LakeMember& m, G& g, uint32_t block, uint32_t nblocks, const uint32_t* list, uint32_t n, uint32_t* M, const uint32_t* B, ProxAcc* acc,
                           uint32_t* nlakes) {
  const uint32_t nl = g.lanes();
  const uint64_t cells = (uint64_t)m.dimx * (uint64_t)m.dimy;
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    for (uint64_t r = (uint64_t)block * nl + l; r < m.cap; r += (uint64_t)nblocks * nl) {   // the member's records: the identities of the fold
      ProxAcc z;
      z.site = 0xFFFFFFFFu; z.sites = 0u; z.cells = 0u; z.flags = 0u; z.far = 0ull; z.sum = 0ull;
      z.x0 = 0xFFFFFFFFu; z.y0 = 0xFFFFFFFFu; z.x1 = 0u; z.y1 = 0u; z.pad[0] = z.pad[1] = z.pad[2] = z.pad[3] = 0u;
      acc[m.rec0 + r] = z;
    }
    const uint64_t i = (uint64_t)block * nl + l;
    if (list) {
      if (i < n) M[m.off + list[i]] = (uint32_t)i;   // (list[i] < the member's cells, and no other entry names it: the caller's checks)
      continue;
    }
    if (i >= cells) continue;
    const size_t a = (size_t)m.off + (size_t)i;
    const uint32_t root = M[a], before = B[m.off];   // (flattened by the launch before; this kernel rewrites M[a] only, and only this lane reads it)
    if (i == cells - 1) *nlakes = B[a] + (root == (uint32_t)a ? 1u : 0u) - before;
    if (root != LAKE_DRY) M[a] = B[root] - before;
  }
}

// ---- columns: the workgroup takes column x of member m ----
struct ProxColumn {   // (the LDS: 8 KB)
  uint64_t mask[PROX_WORDS];
  uint32_t below[PROX_WORDS], above[PROX_WORDS];   // the last site row in front of word k, the first behind it
};
template <class G>
SMX_D void prox_columns_group(const LakeMember& m, G& g, uint32_t x, ProxColumn& s, const uint32_t* M, uint32_t* P) {
  const uint32_t nl = g.lanes(), dimy = (uint32_t)m.dimy, nw = (dimy + 63u) / 64u;
  const size_t base = (size_t)m.off + (size_t)x * dimy;
  for (uint32_t l = g.lo(); l < g.hi(); l++)
    for (uint32_t k = l; k < nw; k += nl) s.mask[k] = 0ull;
  g.barrier();
  for (uint32_t l = g.lo(); l < g.hi(); l++)
    for (uint32_t y = l; y < dimy; y += nl)
      if (M[base + y] != PROX_NONE) SMX_LAKE_OR(s.mask + (y >> 6), (uint64_t)1 << (y & 63u), SMX_LAKE_WG);
  g.barrier();
  for (uint32_t l = g.lo(); l < g.hi(); l++) {   // two linear carries over the words, a lane each: at most PROX_WORDS steps
    if (l == 0u) {
      uint32_t lo = PROX_NONE;
      for (uint32_t k = 0; k < nw; k++) {
        s.below[k] = lo;
        if (s.mask[k]) lo = k * 64u + 63u - (uint32_t)__builtin_clzll(s.mask[k]);
      }
    }
    if (l == nl - 1u) {
      uint32_t hi = PROX_NONE;
      for (uint32_t k = nw; k-- > 0u;) {
        s.above[k] = hi;
        if (s.mask[k]) hi = k * 64u + (uint32_t)__builtin_ctzll(s.mask[k]);
      }
    }
  }
  g.barrier();
  for (uint32_t l = g.lo(); l < g.hi(); l++)
    for (uint32_t y = l; y < dimy; y += nl) {
      const uint32_t k = y >> 6, b = y & 63u;
      const uint64_t w = s.mask[k], dn = w & (~0ull >> (63u - b)), up = w >> b;   // the sites of the word at or below y, at or above it
      const uint32_t lo = dn ? k * 64u + 63u - (uint32_t)__builtin_clzll(dn) : s.below[k];
      const uint32_t hi = up ? y + (uint32_t)__builtin_ctzll(up) : s.above[k];
      uint32_t py = lo;                                                     // (of two equally far the smaller row: lo)
      if (lo == PROX_NONE || (hi != PROX_NONE && hi - y < y - lo)) py = hi;
      P[base + y] = py;
    }
}

// ---- envelope: workgroup `block` takes g.lanes() (band, row) pairs, band * dimy + row: the lanes of a wavefront on consecutive rows ----
template <class G>
SMX_D void prox_envelope_group(const LakeMember& m, G& g, uint32_t block, uint32_t want, const uint32_t* P, uint32_t* S, uint32_t* T, uint32_t* D) {
  const uint32_t nl = g.lanes(), dimx = (uint32_t)m.dimx, dimy = (uint32_t)m.dimy;
  const uint32_t bands = prox_bands(m, want), width = prox_band_width(m, bands);
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    const uint64_t r = (uint64_t)block * nl + l;
    if (r >= (uint64_t)bands * dimy) continue;
    const uint32_t band = (uint32_t)(r / dimy), y = (uint32_t)(r % dimy);
    const uint32_t u0 = band * width, u1 = u0 + width < dimx ? u0 + width : dimx;   // (u0 >= dimx: a band behind the last column, depth 0)
    const uint32_t* const p = P + m.off + y;
    uint32_t* const sp = S + (size_t)m.off + (size_t)u0 * dimy + y;
    uint32_t* const tp = T + (size_t)m.off + (size_t)u0 * dimy + y;
    uint32_t depth = 0u;
    int64_t si = 0, gi = 0, ti = 0;   // the top of the stack: its column, its g, its first x
    for (uint32_t u = u0; u < u1; u++) {
      const uint32_t py = p[(size_t)u * dimy];
      if (py == PROX_NONE) continue;
      const int64_t uu = (int64_t)u, gu = py > y ? (int64_t)(py - y) : (int64_t)(y - py);
      while (depth) {
        if ((ti - si) * (ti - si) + gi * gi <= (ti - uu) * (ti - uu) + gu * gu) break;
        depth--;
        if (depth) {
          const uint32_t v = sp[(size_t)(depth - 1u) * dimy];
          si = (int64_t)(v >> 16); gi = (int64_t)(v & 0xFFFFu); ti = (int64_t)tp[(size_t)(depth - 1u) * dimy];
        }
      }
      int64_t w = 0;
      if (depth) {
        w = 1 + (uu * uu - si * si + gu * gu - gi * gi) / (2 * (uu - si));   // (the numerator is not negative: the top holds its first x against u)
        if (w >= (int64_t)dimx) continue;
      }
      sp[(size_t)depth * dimy] = (u << 16) | (uint32_t)gu;
      tp[(size_t)depth * dimy] = (uint32_t)w;
      si = uu; gi = gu; ti = w; depth++;
    }
    D[(size_t)m.off + (size_t)band * dimy + y] = depth;
  }
}

// ---- query: workgroup `block` takes (SLOTS / lanes) * lanes cells; the LDS table has a slot for every one of them ----
template <int SLOTS>
struct ProxTable {
  uint64_t far[SLOTS], sum[SLOTS];
  uint32_t key[SLOTS], cells[SLOTS], sites[SLOTS], site[SLOTS], x0[SLOTS], y0[SLOTS], x1[SLOTS], y1[SLOTS], flags[SLOTS];
};

// (M: the marks; P: the columns' candidates; S, T, D: the envelopes; nearest / dist2 / group: the planes to write, null = not asked for)
template <int SLOTS, class G>
SMX_D void prox_query_group(const LakeMember& m, G& g, uint32_t block, uint32_t want, ProxTable<SLOTS>& t, const uint32_t* M, const uint32_t* P, const uint32_t* S,
                            const uint32_t* T, const uint32_t* D, ProxAcc* acc, uint32_t* nearest, uint32_t* dist2, uint32_t* group) {
  const uint32_t nl = g.lanes(), items = (uint32_t)SLOTS / nl, dimy = (uint32_t)m.dimy;
  const uint32_t bands = prox_bands(m, want), width = prox_band_width(m, bands);
  const uint64_t n = (uint64_t)m.dimx * (uint64_t)m.dimy, c0 = (uint64_t)block * items * nl;
  for (uint32_t l = g.lo(); l < g.hi(); l++)
    for (uint32_t s = l; s < (uint32_t)SLOTS; s += nl) {
      t.key[s] = PROX_NONE; t.cells[s] = 0u; t.sites[s] = 0u; t.site[s] = 0xFFFFFFFFu; t.far[s] = 0ull; t.sum[s] = 0ull;
      t.x0[s] = 0xFFFFFFFFu; t.y0[s] = 0xFFFFFFFFu; t.x1[s] = 0u; t.y1[s] = 0u; t.flags[s] = 0u;
    }
  g.barrier();
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    for (uint32_t it = 0; it < items; it++) {
      const uint64_t c = c0 + (uint64_t)it * nl + l;
      if (c >= n) break;
      const size_t a = (size_t)m.off + (size_t)c;
      const uint32_t x = (uint32_t)(c / dimy), y = (uint32_t)(c % dimy);
      uint32_t near = PROX_NONE, d2 = PROX_NONE, gi = PROX_NONE;
      for (uint32_t band = 0; band < bands; band++) {
        const uint32_t depth = D[(size_t)m.off + (size_t)band * dimy + y];
        if (!depth) continue;
        const size_t base = (size_t)m.off + (size_t)band * width * dimy + y;
        const uint32_t* const tp = T + base;
        uint32_t lo = 0u, hi = depth - 1u;
        while (lo < hi) {   // the last segment that starts at or in front of x (T[0] == 0: there is one)
          const uint32_t mid = (lo + hi + 1u) >> 1;
          if (tp[(size_t)mid * dimy] <= x) lo = mid; else hi = mid - 1u;
        }
        const uint32_t v = S[base + (size_t)lo * dimy], i = v >> 16, ay = v & 0xFFFFu;
        const uint32_t ax = x > i ? x - i : i - x, d = ax * ax + ay * ay;
        if (d < d2) { d2 = d; near = i; }   // (of equals the lower band's: its columns are smaller)
      }
      if (near != PROX_NONE) {
        near = near * dimy + P[(size_t)m.off + (size_t)near * dimy + y];
        gi = M[(size_t)m.off + near];
      }
      if (nearest) nearest[a] = near;
      if (dist2) dist2[a] = d2;
      if (group) group[a] = gi;
      if (gi >= m.cap) continue;   // (PROX_NONE, or a lake whose record is not kept)
      const uint32_t f = (x == 0u || y == 0u || x == (uint32_t)m.dimx - 1u || y == dimy - 1u) ? PROX_F_BORDER : 0u;
      uint32_t s = (gi * 2654435761u) % (uint32_t)SLOTS;
      for (;;) {   // (at most SLOTS keys are ever inserted: a free or matching slot exists)
        const uint32_t k = SMX_LAKE_CAS(t.key + s, PROX_NONE, gi, SMX_LAKE_WG);
        if (k == PROX_NONE || k == gi) break;
        s = s + 1u == (uint32_t)SLOTS ? 0u : s + 1u;
      }
      SMX_LAKE_ADD(t.cells + s, 1u, SMX_LAKE_WG);
      if (d2 == 0u) { SMX_LAKE_ADD(t.sites + s, 1u, SMX_LAKE_WG); SMX_LAKE_MIN(t.site + s, (uint32_t)c, SMX_LAKE_WG); }
      else SMX_LAKE_ADD(t.sum + s, (uint64_t)d2, SMX_LAKE_WG);
      SMX_LAKE_MAX(t.far + s, ((uint64_t)d2 << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)c), SMX_LAKE_WG);
      SMX_LAKE_MIN(t.x0 + s, x, SMX_LAKE_WG); SMX_LAKE_MAX(t.x1 + s, x, SMX_LAKE_WG);
      SMX_LAKE_MIN(t.y0 + s, y, SMX_LAKE_WG); SMX_LAKE_MAX(t.y1 + s, y, SMX_LAKE_WG);
      if (f) SMX_LAKE_OR(t.flags + s, f, SMX_LAKE_WG);
    }
  }
  g.barrier();
  for (uint32_t l = g.lo(); l < g.hi(); l++)
    for (uint32_t s = l; s < (uint32_t)SLOTS; s += nl) {
      if (t.key[s] == PROX_NONE) continue;
      ProxAcc& r = acc[m.rec0 + t.key[s]];
      SMX_LAKE_ADD(&r.cells, t.cells[s], SMX_LAKE_AGENT);
      if (t.sites[s]) { SMX_LAKE_ADD(&r.sites, t.sites[s], SMX_LAKE_AGENT); SMX_LAKE_MIN(&r.site, t.site[s], SMX_LAKE_AGENT); }
      if (t.sum[s]) SMX_LAKE_ADD(&r.sum, t.sum[s], SMX_LAKE_AGENT);
      SMX_LAKE_MAX(&r.far, t.far[s], SMX_LAKE_AGENT);
      SMX_LAKE_MIN(&r.x0, t.x0[s], SMX_LAKE_AGENT); SMX_LAKE_MAX(&r.x1, t.x1[s], SMX_LAKE_AGENT);
      SMX_LAKE_MIN(&r.y0, t.y0[s], SMX_LAKE_AGENT); SMX_LAKE_MAX(&r.y1, t.y1[s], SMX_LAKE_AGENT);
      if (t.flags[s]) SMX_LAKE_OR(&r.flags, t.flags[s], SMX_LAKE_AGENT);
    }
}

// ---- hist: workgroup `block` takes (SLOTS / lanes) * lanes cells: at most that many distinct keys, a slot for every one of them ----
template <int SLOTS>
struct ProxHistTable {
  uint32_t key[SLOTS], count[SLOTS];
};

// (hist: nbins words per record, record m.rec0 + g for group g of the member; the caller has set them to 0)
template <int SLOTS, class G>
SMX_D void prox_hist_group(const LakeMember& m, G& g, uint32_t block, ProxHistTable<SLOTS>& t, const uint32_t* dist2, const uint32_t* group, uint32_t* hist, uint32_t nbins,
                           uint32_t bin_width) {
  const uint32_t nl = g.lanes(), items = (uint32_t)SLOTS / nl;
  const uint64_t n = (uint64_t)m.dimx * (uint64_t)m.dimy, c0 = (uint64_t)block * items * nl;
  for (uint32_t l = g.lo(); l < g.hi(); l++)
    for (uint32_t s = l; s < (uint32_t)SLOTS; s += nl) { t.key[s] = PROX_NONE; t.count[s] = 0u; }
  g.barrier();
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    for (uint32_t it = 0; it < items; it++) {
      const uint64_t c = c0 + (uint64_t)it * nl + l;
      if (c >= n) break;
      const size_t a = (size_t)m.off + (size_t)c;
      const uint32_t gi = group[a];
      if (gi >= m.cap) continue;
      const uint32_t key = gi * nbins + prox_bin(dist2[a], bin_width, nbins);   // (below cap * nbins < 2^31: the caller's check)
      uint32_t s = (key * 2654435761u) % (uint32_t)SLOTS;
      for (;;) {   // (at most SLOTS keys are ever inserted: a free or matching slot exists)
        const uint32_t k = SMX_LAKE_CAS(t.key + s, PROX_NONE, key, SMX_LAKE_WG);
        if (k == PROX_NONE || k == key) break;
        s = s + 1u == (uint32_t)SLOTS ? 0u : s + 1u;
      }
      SMX_LAKE_ADD(t.count + s, 1u, SMX_LAKE_WG);
    }
  }
  g.barrier();
  for (uint32_t l = g.lo(); l < g.hi(); l++)
    for (uint32_t s = l; s < (uint32_t)SLOTS; s += nl)
      if (t.key[s] != PROX_NONE) SMX_LAKE_ADD(hist + (size_t)m.rec0 * nbins + t.key[s], t.count[s], SMX_LAKE_AGENT);
}

}  // namespace smx
