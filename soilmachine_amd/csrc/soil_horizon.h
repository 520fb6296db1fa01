// soil_horizon.h -- the horizons of every cell in up to sixteen lattice directions (smx_horizons / smx_ensemble_horizons): the largest
// upward slope along each ray and the step that has it, and what follows from them -- the sky-view factor, the open directions, cast
// shadows for a list of suns, the shelter from a wind (Winstral's Sx is the horizon slope of the upwind direction within a reach).
// The bodies of k_horizon_heights, k_horizon_scan and k_horizon_sky. Nothing here writes a map.
//
// Cells and h(c) are those of soil_drain.h (drain_height: the top record's floor + size, a lake's surface, 0.0 for an empty column).
// DIRECTION d = 0..15 is (ux, uy) of horizon_dir, counter-clockwise from +x; len(d) is 1.0, the f64 nearest sqrt 2 or the f64 nearest
// sqrt 5. The RAY of c = (x, y) is c_k = (x + k ux, y + k uy), k = 1, 2, ... while c_k lies in the map and k <= reach (0: no limit);
// no cell is interpolated. s_k = (h(c_k) - h(c)) / ((double)k * len): one subtraction, one multiplication, one division. The horizon
// step K is the smallest k with the largest s_k among those with s_k > +0.0 (plain f64 >: a NaN is never a horizon and a NaN cell has
// none), 0 where there is none; the horizon slope S is that s_k, +0.0 where there is none.
//
//   heights  one workgroup per COARSE x COARSE tile of a member: every lane writes h of its cells to the plane H and folds it into
//            the maximum of its FINE x FINE tile in LDS; the fine maxima go to FM, their maximum to CM, and ONE atomic per workgroup
//            folds that into the member's maximum MM (an ordered image; the caller's fill of 0 is below every image). A maximum
//            ignores NaN: only v > -inf enters, from -inf.
//   scan     one lane per cell and selected direction (the direction is the workgroup's: blockIdx.z), the lanes of a workgroup on
//            consecutive cells of a column, so at equal k they read one contiguous stretch of H. At step k the lane asks the member's
//            maximum, then the coarse tile that holds c_k, then the fine one: with b = (max - h(c)) / ((double)k * len), unless
//            b > best nothing in that tile (in the rest of the ray) can win -- subtraction, multiplication and division round
//            monotonically and k * len grows with k, so every s_j there is <= b <= best or not positive, and a tie belongs to the
//            smaller k that already has it; a NaN bound skips, which is right because a NaN s never wins -- and k advances past the
//            last step inside the tile by integer arithmetic. Only when all three say b > best is h(c_k) loaded. The result is the
//            plain walk's, bit for bit; no lane waits for another. The epilogue folds the direction's record and the counts of its
//            suns in LDS and sends ONE set of atomics per workgroup.
//   sky      (only with sky, open or lit) one lane per cell reads its nd slopes and steps: sky = (sum over the selected directions in
//            ascending d, from 0.0, of 1.0 / (1.0 + S * S)) / (double)nd; open: bit d where K == 0; lit: the suns with !(S > tangent).
// Every figure is a comparison, an exact integer, an order-free extreme or a fixed sequence of single f64 operations. The file
// compiles for the device and, under SMX_D / SMX_HOSTSIM, for the host (tests/horizons_host), as soil_catch.h does.
#pragma once
#include "soil_drain.h"

namespace smx {

constexpr int HORIZON_FINE = 8, HORIZON_COARSE = 64;   // the tile levels' sides, powers of two (tests/horizons_host takes others as a variant)
constexpr uint32_t HORIZON_DIRS = 16u, HORIZON_MAX_SUNS = 64u;
constexpr double HORIZON_SQRT2 = 0x1.6A09E667F3BCDp+0;   // 0x3FF6A09E667F3BCD
constexpr double HORIZON_SQRT5 = 0x1.1E3779B97F4A8p+1;   // 0x4001E3779B97F4A8

#ifdef SMX_HOSTSIM
// (the host build counts what a ray asks: the tile bounds it computes and the heights it loads)
struct HorizonProbes { uint64_t rays = 0, bounds = 0, loads = 0; };
inline HorizonProbes& horizon_probes() { static HorizonProbes p; return p; }
#define SMX_HORIZON_COUNT(field) (void)(horizon_probes().field++)
#else
#define SMX_HORIZON_COUNT(field) (void)0
#endif

struct HorizonSun {   // == smx_sun (include/soilmx.h)
  uint32_t direction, reserved;
  double tangent;
};
struct HorizonAcc {   // a record while it is folded (64 bytes): all zero is the identity of every field
  uint32_t bounded, pad0;
  uint64_t far;       // (step << 32) | (0xFFFFFFFF - cell): the largest step, the smallest cell among equals
  uint64_t step_sum;
  uint64_t smax;      // the ordered image of slope_max (every S that enters is > +0.0: its image is above 0)
  uint64_t pad[4];
};
struct HorizonRec {   // == smx_horizon_record (include/soilmx.h)
  uint32_t direction;
  int16_t ux, uy;
  uint32_t bounded, step_max, step_max_cell, reserved0;
  uint64_t step_sum;
  double slope_max;
  uint32_t reserved[6];
};
static_assert(sizeof(HorizonSun) == 16 && sizeof(HorizonAcc) == 64 && sizeof(HorizonRec) == 64, "horizon record layouts");

// (ux, uy) of direction d < 16: (1,0) (2,1) (1,1) (1,2) (0,1) (-1,2) (-1,1) (-2,1) (-1,0) (-2,-1) (-1,-1) (-1,-2) (0,-1) (1,-2) (1,-1)
// (2,-1). A nibble per direction holds ux + 2; uy(d) = ux(d + 12): the same sequence a quarter turn behind.
SMX_HD void horizon_dir(uint32_t d, int& ux, int& uy) {
  const uint64_t UX = 0x4332110101123343ull;
  ux = (int)((UX >> (4u * (d & 15u))) & 15u) - 2;
  uy = (int)((UX >> (4u * ((d + 12u) & 15u))) & 15u) - 2;
}
SMX_HD double horizon_len(uint32_t d) { return (d & 1u) ? HORIZON_SQRT5 : (d & 2u) ? HORIZON_SQRT2 : 1.0; }
// the d of the j-th selected direction in ascending d (j < popcount(mask))
SMX_HD uint32_t horizon_nth(uint32_t mask, uint32_t j) {
  uint32_t d = 0u;
  for (;; d++)
    if ((mask >> d) & 1u) { if (!j) break; j--; }
  return d;
}
SMX_HD uint32_t horizon_count(uint32_t mask) {
  uint32_t n = 0u;
  for (; mask; mask &= mask - 1u) n++;
  return n;
}
SMX_HD void horizon_finish(const HorizonAcc& a, uint32_t d, HorizonRec& r) {
  int ux, uy;
  horizon_dir(d, ux, uy);
  r.direction = d; r.ux = (int16_t)ux; r.uy = (int16_t)uy;
  r.bounded = a.bounded; r.step_max = (uint32_t)(a.far >> 32); r.step_max_cell = a.bounded ? 0xFFFFFFFFu - (uint32_t)a.far : 0xFFFFFFFFu; r.reserved0 = 0u;
  r.step_sum = a.step_sum;
  r.slope_max = a.bounded ? lake_unkey(a.smax) : 0.0;
  for (uint32_t& w : r.reserved) w = 0u;
}
// the tiles of a member at a level of side T
SMX_HD uint32_t horizon_tiles(const LakeMember& m, int T) { return (uint32_t)((m.dimx + T - 1) / T) * (uint32_t)((m.dimy + T - 1) / T); }

// The planes the scan reads. A member appears twice in the tables: m, as everywhere (off: its first word in H and the per-cell
// planes; rec0: its first record; cap: nd), and t, the view of its tiles (off: its first fine maximum in FM; rec0: its first coarse
// maximum in CM; cap: its position in the call, the index of its maximum in MM and of its row of sun counts).
struct HorizonView {
  const double *H, *FM, *CM;
  const uint64_t* MM;
};

// ---- heights: workgroup `tile` takes the COARSE x COARSE cells of coarse tile `tile` of member m ----
template <int F, int C>
struct HorizonTileMax {
  uint64_t fine[(C / F) * (C / F)];
  uint64_t coarse;
};

template <int F, int C, class G>
SMX_D void horizon_heights_group(const LakeMember& m, const LakeMember& t, G& g, uint32_t tile, HorizonTileMax<F, C>& s, double* H, double* FM, double* CM, uint64_t* MM) {
  static_assert(F > 0 && C >= F && (F & (F - 1)) == 0 && (C & (C - 1)) == 0, "the tile sides are powers of two");
  constexpr uint32_t NF = (uint32_t)(C / F), NT = NF * NF;
  const uint32_t nl = g.lanes(), dimx = (uint32_t)m.dimx, dimy = (uint32_t)m.dimy;
  const uint32_t ncy = (dimy + (uint32_t)C - 1u) / (uint32_t)C, nfy = (dimy + (uint32_t)F - 1u) / (uint32_t)F;
  const uint32_t x0 = (tile / ncy) * (uint32_t)C, y0 = (tile % ncy) * (uint32_t)C;
  const double low = -__builtin_huge_val();
  const uint64_t none = lake_key(low);
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    for (uint32_t i = l; i < NT; i += nl) s.fine[i] = none;
    if (l == 0u) s.coarse = none;
  }
  g.barrier();
  for (uint32_t l = g.lo(); l < g.hi(); l++)
    for (uint32_t i = l; i < (uint32_t)(C * C); i += nl) {   // (consecutive lanes along y: consecutive 32-byte records)
      const uint32_t lx = i / (uint32_t)C, ly = i % (uint32_t)C, x = x0 + lx, y = y0 + ly;
      if (x >= dimx || y >= dimy) continue;
      const size_t c = (size_t)x * dimy + y;
      const double v = drain_height(m.cells[c]);
      H[(size_t)m.off + c] = v;
      if (v > low) SMX_LAKE_MAX(s.fine + (lx / (uint32_t)F) * NF + ly / (uint32_t)F, lake_key(v), SMX_LAKE_WG);
    }
  g.barrier();
  for (uint32_t l = g.lo(); l < g.hi(); l++)
    for (uint32_t i = l; i < NT; i += nl) {
      const uint32_t fx = x0 / (uint32_t)F + i / NF, fy = y0 / (uint32_t)F + i % NF;
      if (fx * (uint32_t)F >= dimx || fy * (uint32_t)F >= dimy) continue;
      FM[(size_t)t.off + (size_t)fx * nfy + fy] = lake_unkey(s.fine[i]);
      SMX_LAKE_MAX(&s.coarse, s.fine[i], SMX_LAKE_WG);
    }
  g.barrier();
  for (uint32_t l = g.lo(); l < g.hi(); l++)
    if (l == 0u) {
      CM[(size_t)t.rec0 + tile] = lake_unkey(s.coarse);
      SMX_LAKE_MAX(MM + t.cap, s.coarse, SMX_LAKE_AGENT);
    }
}

// ---- one ray: the horizon (S, K) of cell c = (x, y) of member m in direction (ux, uy) ----
// the steps from p that stay inside [lo, lo + side) along one axis moving by u (|u| <= 2); no limit where u == 0
SMX_HD uint32_t horizon_room(uint32_t p, uint32_t lo, uint32_t side, int u) {
  if (u == 0) return 0xFFFFFFFFu;
  const uint32_t room = u > 0 ? lo + side - 1u - p : p - lo;
  return (u == 2 || u == -2) ? room >> 1 : room;
}
template <int F, int C>
SMX_D void horizon_ray(const LakeMember& m, const LakeMember& t, const HorizonView& v, uint32_t x, uint32_t y, int ux, int uy, double len, uint32_t reach, double& S, uint32_t& K) {
  const uint32_t dimx = (uint32_t)m.dimx, dimy = (uint32_t)m.dimy;
  const double* const H = v.H + m.off;
  const double h0 = H[(size_t)x * dimy + y];
  uint32_t last = horizon_room(x, 0u, dimx, ux);   // the last step inside the map and the reach (at most 65535: one axis moves)
  const uint32_t ry = horizon_room(y, 0u, dimy, uy);
  if (ry < last) last = ry;
  if (reach && reach < last) last = reach;
  double best = 0.0;
  uint32_t bk = 0u;
  SMX_HORIZON_COUNT(rays);
#ifndef SMX_HORIZON_NO_TILES
  const uint32_t ncy = (dimy + (uint32_t)C - 1u) / (uint32_t)C, nfy = (dimy + (uint32_t)F - 1u) / (uint32_t)F;
  const double* const FM = v.FM + t.off;
  const double* const CM = v.CM + t.rec0;
  const double top = lake_unkey(v.MM[t.cap]);
#else
  (void)t;
#endif
  // ONE loop whose every turn is a step, a skip or the end: the lanes of a wavefront stay in one body. (Measured against it: the
  // levels as nested loops, a fine tile walked to its end once entered, with the divisions filtered by a product -- a third of the
  // bounds and 1.9 times the time, profiles/r25_horizons.md.)
  for (uint32_t k = 1u; k <= last;) {
    const uint32_t px = (uint32_t)((int)x + (int)k * ux), py = (uint32_t)((int)y + (int)k * uy);
    const double den = (double)k * len;
#ifndef SMX_HORIZON_NO_TILES
    SMX_HORIZON_COUNT(bounds);
    if (!((top - h0) / den > best)) break;   // nothing on the rest of the ray
    const uint32_t cx = px / (uint32_t)C, cy = py / (uint32_t)C;
    SMX_HORIZON_COUNT(bounds);
    if (!((CM[(size_t)cx * ncy + cy] - h0) / den > best)) {
      const uint32_t a = horizon_room(px, cx * (uint32_t)C, (uint32_t)C, ux), b = horizon_room(py, cy * (uint32_t)C, (uint32_t)C, uy);
      const uint32_t stay = a < b ? a : b;
      if (stay >= last - k) break;
      k += stay + 1u;
      continue;
    }
    const uint32_t fx = px / (uint32_t)F, fy = py / (uint32_t)F;
    SMX_HORIZON_COUNT(bounds);
    if (!((FM[(size_t)fx * nfy + fy] - h0) / den > best)) {
      const uint32_t a = horizon_room(px, fx * (uint32_t)F, (uint32_t)F, ux), b = horizon_room(py, fy * (uint32_t)F, (uint32_t)F, uy);
      const uint32_t stay = a < b ? a : b;
      if (stay >= last - k) break;
      k += stay + 1u;
      continue;
    }
#endif
    SMX_HORIZON_COUNT(loads);
    const double s = (H[(size_t)px * dimy + py] - h0) / den;
    if (s > best) { best = s; bk = k; }
    k++;
  }
  S = best; K = bk;
}

// ---- scan: workgroup `block` takes g.lanes() consecutive cells of member m in direction d, the j-th selected one ----
struct HorizonFold {
  uint64_t far, sum, smax;
  uint32_t bounded;
  uint32_t lit[HORIZON_MAX_SUNS];
};

// (Sp / Kp: the slope and step planes of all directions, nd * words each, null = not kept; acc: the records; lit_cells: nsuns counts a member)
template <int F, int C, class G>
SMX_D void horizon_scan_group(const LakeMember& m, const LakeMember& t, G& g, uint32_t block, HorizonFold& f, const HorizonView& v, uint32_t d, uint32_t j, uint32_t reach,
                              const HorizonSun* suns, uint32_t nsuns, uint64_t words, double* Sp, uint32_t* Kp, HorizonAcc* acc, uint32_t* lit_cells) {
  const uint32_t nl = g.lanes(), dimy = (uint32_t)m.dimy;
  const uint64_t n = (uint64_t)m.dimx * (uint64_t)m.dimy;
  int ux, uy;
  horizon_dir(d, ux, uy);
  const double len = horizon_len(d);
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    for (uint32_t i = l; i < HORIZON_MAX_SUNS; i += nl) f.lit[i] = 0u;
    if (l == 0u) { f.far = 0ull; f.sum = 0ull; f.smax = 0ull; f.bounded = 0u; }
  }
  g.barrier();
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    const uint64_t c = (uint64_t)block * nl + l;
    if (c >= n) continue;
    double S;
    uint32_t K;
    horizon_ray<F, C>(m, t, v, (uint32_t)(c / dimy), (uint32_t)(c % dimy), ux, uy, len, reach, S, K);
    const size_t at = (size_t)j * (size_t)words + (size_t)m.off + (size_t)c;
    if (Sp) Sp[at] = S;
    if (Kp) Kp[at] = K;
    if (K) {
      SMX_LAKE_ADD(&f.bounded, 1u, SMX_LAKE_WG);
      SMX_LAKE_MAX(&f.far, ((uint64_t)K << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)c), SMX_LAKE_WG);
      SMX_LAKE_ADD(&f.sum, (uint64_t)K, SMX_LAKE_WG);
      SMX_LAKE_MAX(&f.smax, lake_key(S), SMX_LAKE_WG);
    }
    for (uint32_t i = 0; i < nsuns; i++)
      if (suns[i].direction == d && !(S > suns[i].tangent)) SMX_LAKE_ADD(f.lit + i, 1u, SMX_LAKE_WG);
  }
  g.barrier();
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    if (l == 0u && f.bounded) {
      HorizonAcc& r = acc[(size_t)m.rec0 + j];
      SMX_LAKE_ADD(&r.bounded, f.bounded, SMX_LAKE_AGENT);
      SMX_LAKE_MAX(&r.far, f.far, SMX_LAKE_AGENT);
      SMX_LAKE_ADD(&r.step_sum, f.sum, SMX_LAKE_AGENT);
      SMX_LAKE_MAX(&r.smax, f.smax, SMX_LAKE_AGENT);
    }
    for (uint32_t i = l; i < nsuns; i += nl)
      if (f.lit[i]) SMX_LAKE_ADD(lit_cells + (size_t)t.cap * nsuns + i, f.lit[i], SMX_LAKE_AGENT);
  }
}

// ---- sky: workgroup `block` takes g.lanes() cells of member m; what needs all directions of a cell ----
template <class G>
SMX_D void horizon_sky_group(const LakeMember& m, G& g, uint32_t block, uint32_t mask, const HorizonSun* suns, uint32_t nsuns, uint64_t words, const double* Sp,
                             const uint32_t* Kp, double* sky, uint32_t* open, uint32_t* lit) {
  const uint32_t nl = g.lanes(), nd = horizon_count(mask);
  const uint64_t n = (uint64_t)m.dimx * (uint64_t)m.dimy;
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    const uint64_t c = (uint64_t)block * nl + l;
    if (c >= n) continue;
    const size_t a = (size_t)m.off + (size_t)c;
    if (sky || open) {
      double sum = 0.0;
      uint32_t bits = 0u, j = 0u;
      for (uint32_t d = 0; d < HORIZON_DIRS; d++) {
        if (!((mask >> d) & 1u)) continue;
        const size_t at = (size_t)j * (size_t)words + a;
        const double S = Sp[at];
        sum = sum + 1.0 / (1.0 + S * S);
        if (Kp[at] == 0u) bits |= 1u << d;
        j++;
      }
      if (sky) sky[a] = sum / (double)nd;
      if (open) open[a] = bits;
    }
    if (lit) {
      uint32_t count = 0u;
      for (uint32_t i = 0; i < nsuns; i++) {
        const uint32_t j = horizon_count(mask & ((1u << suns[i].direction) - 1u));
        if (!(Sp[(size_t)j * (size_t)words + a] > suns[i].tangent)) count++;
      }
      lit[a] = count;
    }
  }
}

}  // namespace smx
