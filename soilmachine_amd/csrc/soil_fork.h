// soil_fork.h -- copying a map's state into other contexts on the device (smx_copy_state / smx_ensemble_fork): the bodies of
// k_fork_count, k_fork_scatter and k_fork_planes. Nothing here writes the source.
//
// The destination's pool layout is the one smx_import_columns produces, whatever the source pool looks like: buried sections at
// pool indices 0..used-1 in cell order x*dimy+y, bottom -> top within a column, the top section inline in the cell record, `prev`
// renumbered, freelist[i] = cap-1-i for i < cap-used. A fork is therefore a COMPACTING copy in three steps:
//   count    one lane per cell walks its chain: buried sections, the flag byte as smx_load derives it (F_AIR from the top section,
//            F_SAT from any saturation in the column, OR the source's sticky F_SAT bit), and every link validated (prev < cap,
//            links <= cap). Per workgroup one add to the totals and one min on the error word (the first bad cell).
//   scan     exclusive prefix sum of the buried counts in cell order = each column's first pool index (the caller's business:
//            rocPRIM on the device, a loop in tests/fork_host)
//   scatter  one lane per cell and destination walks the chain again and writes section j (counted from the top) at
//            base + (k-1-j), then the cell record, the flag byte, its share of the free list; lane 0 of workgroup 0 writes
//            free_count, the live-section counter and the generator (the source's, or srandom_r(seed)), workgroup 0 the soil table.
// The file compiles for the device and, under SMX_D / SMX_HOSTSIM, for the host (tests/fork_host runs the same bodies with the
// lanes of a workgroup looped), with the group object of soil_observe.h: lanes(), lo(), hi(), barrier().
#pragma once
#include "soil_serial.h"

#ifdef SMX_HOSTSIM
#define SMX_FORK_ADD64(p, v) (void)(*(p) += (v))
#define SMX_FORK_MIN64(p, v) (void)(*(p) = *(p) < (v) ? *(p) : (v))
#else
#define SMX_FORK_ADD64(p, v) (void)atomicAdd((p), (v))
#define SMX_FORK_MIN64(p, v) (void)atomicMin((p), (v))
#endif

namespace smx {

struct ForkSrc {    // the source, read only
  const Sec* cells; const Sec* pool; const uint8_t* flags;
  const float* wfreq; const float* wtrack; const float* windfreq;
  const SoilP* soils; const RandState* rnd;
  uint64_t cap;     // the SOURCE's pool capacity: the bound of its links
  uint64_t ncells;
  uint32_t nsoils;
};
struct ForkDst {    // one destination
  Sec* cells; Sec* pool; uint32_t* freelist; uint32_t* free_count; uint8_t* flags;
  float* wfreq; float* wtrack; float* windfreq;
  SoilP* soils; RandState* rnd; unsigned long long* ctr;
  uint64_t cap;     // its own pool capacity
  uint32_t seeded, seed;   // seeded != 0: the generator as after smx_srand(seed); else the source's, continued
};
constexpr unsigned long long FORK_NONE = ~0ull;
struct ForkTotals {
  unsigned long long used;       // buried sections = pool records the destination needs
  unsigned long long nonempty;   // columns with a top section; used + nonempty = live sections
  unsigned long long bad;        // FORK_NONE, or the lowest cell whose chain leaves the pool or has more links than it holds
};
constexpr int FORK_LANES = 256;
struct ForkShared { unsigned long long used[FORK_LANES], nonempty[FORK_LANES], bad[FORK_LANES]; };
struct alignas(16) ForkQuad { float a, b, c, d; };

// 0, -4 (more live sections than the destination's pool holds: smx_import_columns's rule) or -5 (a corrupt chain in the source)
SMX_HD int fork_verdict(const ForkTotals& t, uint64_t dst_cap) {
  if (t.bad != FORK_NONE) return -5;
  if (t.used + t.nonempty > dst_cap) return -4;
  return 0;
}

// workgroup `block` of g.lanes() cells: buried[c], flag[c]; the totals once per workgroup
template <class G>
SMX_D void fork_count_group(const ForkSrc& s, G& g, size_t block, ForkShared& sh, uint32_t* buried, uint8_t* flag, ForkTotals* tot) {
  const uint32_t nl = g.lanes();
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    const size_t c = block * nl + l;
    unsigned long long u = 0, ne = 0, bad = FORK_NONE;
    if (c < s.ncells) {
      const Sec top = s.cells[c];
      uint8_t f = (uint8_t)(s.flags[c] & F_SAT);
      uint32_t k = 0;
      if (top.type != EMPTY) {
        ne = 1;
        if (top.type == AIR) f |= F_AIR;
        if (top.sat != 0.0) f |= F_SAT;
        uint32_t pv = top.prev;
        while (pv != NIL) {
          if (pv >= s.cap || (uint64_t)k >= s.cap) { bad = c; break; }
          const double sat = s.pool[pv].sat;
          const uint32_t nx = s.pool[pv].prev;
          if (sat != 0.0) f |= F_SAT;
          k++;
          pv = nx;
        }
      }
      buried[c] = k; flag[c] = f; u = k;
    }
    sh.used[l] = u; sh.nonempty[l] = ne; sh.bad[l] = bad;
  }
  g.barrier();
  uint32_t top2 = 1u;
  while (top2 < nl) top2 <<= 1;
  for (uint32_t w = top2 >> 1; w >= 1u; w >>= 1) {
    for (uint32_t l = g.lo(); l < g.hi(); l++) {
      if (l >= w || l + w >= nl) continue;
      sh.used[l] += sh.used[l + w]; sh.nonempty[l] += sh.nonempty[l + w];
      if (sh.bad[l + w] < sh.bad[l]) sh.bad[l] = sh.bad[l + w];
    }
    g.barrier();
  }
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    if (l != 0) continue;
    if (sh.used[0]) SMX_FORK_ADD64(&tot->used, sh.used[0]);
    if (sh.nonempty[0]) SMX_FORK_ADD64(&tot->nonempty, sh.nonempty[0]);
    if (sh.bad[0] != FORK_NONE) SMX_FORK_MIN64(&tot->bad, sh.bad[0]);
  }
}

// cell c of the source into destination d: k buried sections, the first of them (the bottom one) at pool index b
SMX_D void fork_scatter_cell(const ForkSrc& s, const ForkDst& d, size_t c, uint32_t k, uint32_t b) {
  Sec top = s.cells[c];
  if (top.type == EMPTY) { top.size = 0; top.floor = 0; top.sat = 0; top.prev = NIL; }
  else {
    uint32_t pv = top.prev;
    for (uint32_t j = 0; j < k; j++) {
      const uint32_t up = k - 1u - j, at = b + up;
      if (pv >= s.cap || (uint64_t)at >= d.cap) break;   // (the count pass validated both; a source that changed under the call must not write out of bounds)
      Sec r = s.pool[pv];
      pv = r.prev;
      r.prev = up ? at - 1u : NIL;
      d.pool[at] = r;
    }
    top.prev = k ? b + k - 1u : NIL;
  }
  d.cells[c] = top;
}

// workgroup `block` of `nblocks`, one destination
template <class G>
SMX_D void fork_scatter_group(const ForkSrc& s, const ForkDst& d, G& g, size_t block, size_t nblocks, const uint32_t* buried, const uint32_t* base,
                              const uint8_t* flag, ForkTotals tot) {
  const uint32_t nl = g.lanes();
  const uint64_t nfree = d.cap - tot.used, nthreads = (uint64_t)nblocks * nl;
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    const uint64_t gid = (uint64_t)block * nl + l;
    if (gid < s.ncells) {
      fork_scatter_cell(s, d, (size_t)gid, buried[gid], base[gid]);
      d.flags[gid] = flag[gid];
    }
    for (uint64_t i = gid; i < nfree; i += nthreads) d.freelist[i] = (uint32_t)(d.cap - 1u - i);
    if (block != 0) continue;
    const uint32_t* sw = reinterpret_cast<const uint32_t*>(s.soils);
    uint32_t* dw = reinterpret_cast<uint32_t*>(d.soils);
    for (uint32_t i = l; i < s.nsoils * (uint32_t)(sizeof(SoilP) / 4); i += nl) dw[i] = sw[i];
    if (l != 0) continue;
    *d.free_count = (uint32_t)nfree;
    d.ctr[C_LIVE_SECTIONS] = tot.used + tot.nonempty;
    RandState r;
    if (d.seeded) rand_seed(r, d.seed); else r = *s.rnd;
    *d.rnd = r;
  }
}

// the three f32 planes, lane gid of nthreads: quads of four values, then the n % 4 values after them
SMX_D void fork_planes_lane(const ForkSrc& s, const ForkDst& d, uint64_t gid, uint64_t nthreads) {
  const uint64_t n4 = s.ncells / 4, rest = s.ncells - 4 * n4;
  const float* const src[3] = {s.wfreq, s.wtrack, s.windfreq};
  float* const dst[3] = {d.wfreq, d.wtrack, d.windfreq};
  for (int p = 0; p < 3; p++) {
    const ForkQuad* a = reinterpret_cast<const ForkQuad*>(src[p]);
    ForkQuad* o = reinterpret_cast<ForkQuad*>(dst[p]);
    for (uint64_t i = gid; i < n4; i += nthreads) o[i] = a[i];
    if (gid < rest) dst[p][4 * n4 + gid] = src[p][4 * n4 + gid];
  }
}

}  // namespace smx
