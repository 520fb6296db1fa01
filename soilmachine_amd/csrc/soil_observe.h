// soil_observe.h -- observing an ensemble as one thing (smx_ensemble_figures / smx_ensemble_plane_stats): the bodies of
// k_ens_figures and k_ens_plane_stats. Nothing here writes a member's state.
//
// The file compiles for the device and, under SMX_D / SMX_HOSTSIM, for the host (tests/observe_host runs the very same bodies
// with the lanes of a workgroup looped). A body sees its workgroup through a group object G:
//   g.lanes()          lanes of the workgroup (a multiple of 64)
//   g.lo() .. g.hi()   the lanes THIS caller executes: [threadIdx.x, threadIdx.x + 1) on the device, [0, lanes) on the host
//   g.barrier()        __syncthreads() / nothing
// Between two barriers no lane reads what another lane writes, so the host's lane-after-lane order is one legal device order.
//
// Figures of one member (struct ObsFigures = smx_member_figures + a verdict on the section chains):
//   sumh, water_volume   sequential f64 sums over the cells in index order x*dimy+y   } order-DEPENDENT by definition: each is
//   typehash             h = (h ^ type) * prime, cells in index order, top -> bottom  } folded by ONE lane
//   nsec, wet_cells, empty_cells, hmin, hmax                                            order-free: per-lane partials, tree-reduced at the end
// Layermap::height(ivec2) = floor + size of the top section, 0 for an empty column (layermap.h:422-425); a wet cell is one whose
// top section is Air (surface 0, layermap.h:417-420, on a non-empty column).
//
// The cells are streamed tile by tile (TILE consecutive cells). STAGER lanes read the 32-byte cell records -- adjacent lanes
// adjacent cells -- walk up to K buried sections of their column and leave per cell in LDS: height, water size, top type, the
// chain's first K types and the pool index where the chain goes on (NIL: all of it is staged). The HASH lane folds the staged
// types and walks what did not fit (chains run from 1 to hundreds of sections) straight from memory; the SUM lane folds heights
// and water. With four or more wavefronts the two fold lanes sit in wavefronts of their own (0 and 1) and the stagers fill tile
// k+1 while tile k is folded; narrower workgroups do one after the other. The results do not depend on TILE, K or the width:
// every order-dependent value is produced in cell order by one lane, whatever was staged.
#pragma once
#include "soil_core.h"

namespace smx {

struct ObsFigures {   // the first 80 bytes are smx_member_figures (include/soilmx.h)
  double sumh;
  uint64_t nsec, typehash, wet_cells;
  double water_volume, hmin, hmax;
  uint64_t empty_cells, rand_calls, live_sections;
  uint64_t corrupt;   // not 0: a section chain leaves the pool or has more links than the pool holds (smx_digest's -5)
};

constexpr uint64_t FNV_START = 1469598103934665603ull, FNV_PRIME = 1099511628211ull;

template <int TILE, int K>
struct FigTile {
  double h[TILE];                          // Layermap::height of the cell
  double wsz[TILE];                        // size of the top section where it is water, else 0
  uint32_t ttype[TILE];                    // type of the top section (EMPTY: no column)
  uint32_t next[TILE];                     // pool index of the first buried section that is NOT staged (NIL: none)
  uint32_t cnt[TILE];                      // buried sections staged (<= K)
  uint32_t types[(K > 0 ? K : 1) * TILE];  // [k * TILE + cell]: lanes of a wavefront write neighbouring words
};
struct FigPart { unsigned long long nsec, wet, empty; double hmin, hmax; };   // one stager lane's order-free partials
struct FigFold { uint64_t hash, nsec_more; double sumh, wvol; };              // the fold lanes' running values
template <int TILE, int K, int LANES>
struct FigShared {
  FigTile<TILE, K> tile[2];
  FigPart part[LANES];
  FigFold fold;
  uint32_t err[2];   // [iteration parity]: set during an iteration, read by all lanes after that iteration's barrier
};

// (-0 < +0, so that the extremes do not depend on which lane saw which cell)
SMX_D void fig_min(double& m, double h) { if (h < m || (h == m && signbit(h) && !signbit(m))) m = h; }
SMX_D void fig_max(double& m, double h) { if (h > m || (h == m && !signbit(h) && signbit(m))) m = h; }

// stager `sl` of `nsl`: cells sl, sl + nsl, ... of tile `tile`
template <int TILE, int K>
SMX_D void fig_stage(const DevState& s, size_t n, size_t tile, uint32_t sl, uint32_t nsl, FigTile<TILE, K>& t, FigPart& p, uint32_t& err) {
  const size_t c0 = tile * TILE;
  for (uint32_t i = sl; i < (uint32_t)TILE; i += nsl) {
    const size_t c = c0 + i;
    if (c >= n) break;
    const Sec top = s.cells[c];
    double h = 0.0, w = 0.0;
    uint32_t cnt = 0, nx = NIL;
    if (top.type == EMPTY) p.empty++;
    else {
      h = top.floor + top.size;
      if (top.type == AIR) { p.wet++; w = top.size; }
      nx = top.prev;
      while (nx != NIL && cnt < (uint32_t)K) {
        if (nx >= s.pool_capacity) { err = 1u; nx = NIL; break; }
        const uint32_t ty = s.pool[nx].type, pv = s.pool[nx].prev;   // (the last 8 bytes of the record: one load)
        t.types[cnt * TILE + i] = ty;
        cnt++;
        nx = pv;
      }
      p.nsec += 1ull + cnt;
    }
    fig_min(p.hmin, h); fig_max(p.hmax, h);
    t.h[i] = h; t.wsz[i] = w; t.ttype[i] = top.type; t.next[i] = nx; t.cnt[i] = cnt;
  }
}

// the hash lane: tile `tile` in cell order, every column top -> bottom; what is not staged comes from memory
template <int TILE, int K>
SMX_D void fig_fold_hash(const DevState& s, size_t n, size_t tile, const FigTile<TILE, K>& t, FigFold& f, uint32_t& err) {
  const size_t c0 = tile * TILE;
  const uint32_t m = n - c0 < (size_t)TILE ? (uint32_t)(n - c0) : (uint32_t)TILE;
  uint64_t h = f.hash, more = 0;
  for (uint32_t i = 0; i < m; i++) {
    const uint32_t ty = t.ttype[i];
    if (ty == EMPTY) continue;
    h = (h ^ (uint64_t)ty) * FNV_PRIME;
    const uint32_t cnt = t.cnt[i];
    for (uint32_t k = 0; k < cnt; k++) h = (h ^ (uint64_t)t.types[k * TILE + i]) * FNV_PRIME;
    uint32_t nx = t.next[i];
    uint64_t links = cnt;
    while (nx != NIL) {
      if (nx >= s.pool_capacity || ++links > s.pool_capacity) { err = 1u; f.hash = h; f.nsec_more += more; return; }
      const uint32_t bt = s.pool[nx].type, pv = s.pool[nx].prev;
      h = (h ^ (uint64_t)bt) * FNV_PRIME;
      more++;
      nx = pv;
    }
  }
  f.hash = h; f.nsec_more += more;
}

// the sum lane: heights and water of tile `tile`, sequential f64 in cell order
template <int TILE, int K>
SMX_D void fig_fold_sums(size_t n, size_t tile, const FigTile<TILE, K>& t, FigFold& f) {
  const size_t c0 = tile * TILE;
  const uint32_t m = n - c0 < (size_t)TILE ? (uint32_t)(n - c0) : (uint32_t)TILE;
  double sh = f.sumh, wv = f.wvol;
  for (uint32_t i = 0; i < m; i++) {
    sh += t.h[i];
    if (t.ttype[i] == AIR) wv += t.wsz[i];
  }
  f.sumh = sh; f.wvol = wv;
}

// one workgroup, one member
template <int TILE, int K, int LANES, class G>
SMX_D void figures_group(const DevState& s, G& g, FigShared<TILE, K, LANES>& sh, ObsFigures* out) {
  const uint32_t nl = g.lanes();                       // <= LANES
  const uint32_t st0 = nl >= 256u ? 128u : 0u;         // wavefronts 0 and 1 fold only, where there are four or more
  const uint32_t nst = nl - st0;
  const uint32_t hash_lane = 0u, sum_lane = nl > 64u ? 64u : 0u;
  const size_t n = (size_t)s.dimx * s.dimy, ntiles = (n + TILE - 1) / TILE;
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    FigPart& p = sh.part[l];
    p.nsec = 0; p.wet = 0; p.empty = 0; p.hmin = INFINITY; p.hmax = -INFINITY;
    if (l == 0) { sh.fold.hash = FNV_START; sh.fold.nsec_more = 0; sh.fold.sumh = 0.0; sh.fold.wvol = 0.0; sh.err[0] = 0u; sh.err[1] = 0u; }
  }
  g.barrier();
  bool bad = false;
  for (size_t it = 0; it <= ntiles && !bad; it++) {
    uint32_t& err = sh.err[it & 1];
    for (uint32_t l = g.lo(); l < g.hi(); l++) {
      if (it < ntiles && l >= st0) fig_stage<TILE, K>(s, n, it, l - st0, nst, sh.tile[it & 1], sh.part[l], err);
      if (it >= 1 && l == hash_lane) fig_fold_hash<TILE, K>(s, n, it - 1, sh.tile[(it - 1) & 1], sh.fold, err);
      if (it >= 1 && l == sum_lane) fig_fold_sums<TILE, K>(n, it - 1, sh.tile[(it - 1) & 1], sh.fold);
    }
    g.barrier();
    bad = sh.err[it & 1] != 0u;   // (written before this barrier or two iterations from now: every lane reads the same)
  }
  // the order-free partials: a tree over the lanes (sums of integers and extremes with a total order: any tree gives the same)
  uint32_t top = 1u;
  while (top < nl) top <<= 1;
  for (uint32_t w = top >> 1; w >= 1u; w >>= 1) {
    for (uint32_t l = g.lo(); l < g.hi(); l++) {
      if (l >= w || l + w >= nl) continue;
      FigPart& p = sh.part[l];
      const FigPart& q = sh.part[l + w];
      p.nsec += q.nsec; p.wet += q.wet; p.empty += q.empty;
      fig_min(p.hmin, q.hmin); fig_max(p.hmax, q.hmax);
    }
    g.barrier();
  }
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    if (l != 0) continue;
    ObsFigures r;
    const FigPart& p = sh.part[0];
    r.nsec = sh.fold.nsec_more + p.nsec; r.wet_cells = p.wet; r.empty_cells = p.empty; r.hmin = p.hmin; r.hmax = p.hmax;
    r.sumh = sh.fold.sumh; r.water_volume = sh.fold.wvol; r.typehash = sh.fold.hash;
    r.rand_calls = s.rnd->calls;
    r.live_sections = s.ctr[C_LIVE_SECTIONS];
    r.corrupt = bad ? 1ull : 0ull;
    *out = r;
  }
}

// ---------------- cross-member statistics of one plane ----------------
enum { OBS_PLANE_HEIGHT = 0, OBS_PLANE_WATER = 1, OBS_PLANE_WFREQ = 2, OBS_PLANE_WINDFREQ = 3 };   // == SMX_PLANE_*

// The value of cell `c` in one member. M names the selected members in fold order: m.cells(i), m.wfreq(i), m.windfreq(i).
// HEIGHT / WATER index the cell records (x*dimy+y), the frequency planes their own arrays (y*dimx+x): `c` is the plane's own index.
template <int PLANE, class M>
SMX_D double obs_value(const M& m, uint32_t i, size_t c) {
  if constexpr (PLANE == OBS_PLANE_HEIGHT) {
    const Sec* t = m.cells(i) + c;
    const double fl = t->floor, sz = t->size;
    return t->type == EMPTY ? 0.0 : fl + sz;
  } else if constexpr (PLANE == OBS_PLANE_WATER) {
    const Sec* t = m.cells(i) + c;
    const double sz = t->size;
    return t->type == AIR ? sz : 0.0;
  } else if constexpr (PLANE == OBS_PLANE_WFREQ) {
    return (double)m.wfreq(i)[c];
  } else {
    return (double)m.windfreq(i)[c];
  }
}

// One cell over the n selected members, in their order: mean = (((v0 + v1) + ...) / n, var = (((v0 - mean)^2 + ...) / n (a second
// pass, only where var is wanted), the extremes and the number of members with v != 0. No contraction (-ffp-contract=off).
template <int PLANE, class M>
SMX_D void plane_stats_cell(const M& m, uint32_t n, size_t c, double* mean, double* var, double* vmin, double* vmax, uint32_t* nonzero) {
  double acc = 0.0, lo = 0.0, hi = 0.0;
  uint32_t nz = 0;
#pragma unroll 4
  for (uint32_t i = 0; i < n; i++) {
    const double v = obs_value<PLANE>(m, i, c);
    acc += v;
    if (i == 0) { lo = v; hi = v; }
    else { if (v < lo) lo = v; if (v > hi) hi = v; }
    if (v != 0.0) nz++;
  }
  const double mu = acc / (double)n;
  if (mean) mean[c] = mu;
  if (vmin) vmin[c] = lo;
  if (vmax) vmax[c] = hi;
  if (nonzero) nonzero[c] = nz;
  if (var) {
    double a2 = 0.0;
#pragma unroll 4
    for (uint32_t i = 0; i < n; i++) {
      const double d = obs_value<PLANE>(m, i, c) - mu;
      a2 += d * d;
    }
    var[c] = a2 / (double)n;
  }
}

}  // namespace smx
