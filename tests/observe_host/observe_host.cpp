// observe_host -- TEST-ONLY host build of soilmachine_amd/csrc/soil_observe.h (the bodies of k_ens_figures and k_ens_plane_stats).
//
// The same header the kernels are made of, compiled by g++ (-ffp-contract=off) and run with the lanes of a workgroup looped one
// after the other: one legal order of the device's lanes between two barriers. A member's DevState is built from a snapshot's
// columns the way hostsim's hs_import does it. tests/observe_host_lib.py builds and binds this file; the product never loads it.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#define SMX_D inline
#define SMX_HOSTSIM 1
#include "../../soilmachine_amd/csrc/soil_core.h"
#include "../../soilmachine_amd/csrc/soil_observe.h"

using namespace smx;

struct oh_ctx {
  DevState d;
  std::vector<Sec> cells, pool;
  std::vector<float> wfreq, windfreq;
  RandState rnd;
  unsigned long long ctr[C_COUNT];
  uint32_t longest = 0;   // sections of the longest column
};

struct HostGroup {   // a workgroup whose lanes the caller runs one after the other
  uint32_t n;
  uint32_t lanes() const { return n; }
  uint32_t lo() const { return 0u; }
  uint32_t hi() const { return n; }
  void barrier() const {}
};

struct HostMembers {
  oh_ctx* const* m;
  const Sec* cells(uint32_t i) const { return m[i]->d.cells; }
  const float* wfreq(uint32_t i) const { return m[i]->d.wfreq; }
  const float* windfreq(uint32_t i) const { return m[i]->d.windfreq; }
};

template <int TILE, int K>
static void run_figures(oh_ctx* c, uint32_t lanes, ObsFigures* out) {
  static FigShared<TILE, K, 256> sh;   // (the "LDS")
  HostGroup g{lanes};
  figures_group<TILE, K, 256>(c->d, g, sh, out);
}

template <int PLANE>
static void run_plane(oh_ctx* const* m, uint32_t n, size_t cells, double* mean, double* var, double* vmin, double* vmax, uint32_t* nonzero) {
  const HostMembers hm{m};
  for (size_t c = 0; c < cells; c++) plane_stats_cell<PLANE>(hm, n, c, mean, var, vmin, vmax, nonzero);
}

extern "C" {

// columns bottom -> top in cell order (the snapshot layout); buried sections go into the pool in the order they are met
oh_ctx* oh_create(int dimx, int dimy, uint64_t cap, const uint32_t* count, const uint32_t* type, const double* size, const double* floor,
                  const double* sat, const float* wfreq, const float* windfreq, uint64_t rand_calls) {
  oh_ctx* c = new oh_ctx();
  memset(&c->d, 0, sizeof(c->d));
  memset(&c->rnd, 0, sizeof(c->rnd));
  memset(c->ctr, 0, sizeof(c->ctr));
  const size_t n = (size_t)dimx * dimy;
  c->d.dimx = dimx; c->d.dimy = dimy; c->d.x_lo = 0; c->d.x_hi = dimx; c->d.pool_capacity = cap;
  c->cells.resize(n); c->pool.resize(cap ? cap : 1);
  size_t off = 0; uint32_t used = 0; unsigned long long live = 0;
  for (size_t i = 0; i < n; i++) {
    Sec cell; cell.size = cell.floor = cell.sat = 0; cell.type = EMPTY; cell.prev = NIL;
    uint32_t pv = NIL;
    if (count[i] > c->longest) c->longest = count[i];
    for (uint32_t j = 0; j < count[i]; j++, off++, live++) {
      Sec r; r.size = size[off]; r.floor = floor[off]; r.sat = sat[off]; r.type = type[off]; r.prev = pv;
      if (j == count[i] - 1) cell = r;
      else {
        if (used >= cap) { delete c; return nullptr; }
        pv = used; c->pool[used++] = r;
      }
    }
    c->cells[i] = cell;
  }
  c->ctr[C_LIVE_SECTIONS] = live;
  c->rnd.calls = rand_calls;
  c->wfreq.assign(n, 0.0f); c->windfreq.assign(n, 0.0f);
  if (wfreq) c->wfreq.assign(wfreq, wfreq + n);
  if (windfreq) c->windfreq.assign(windfreq, windfreq + n);
  c->d.cells = c->cells.data(); c->d.pool = c->pool.data();
  c->d.wfreq = c->wfreq.data(); c->d.windfreq = c->windfreq.data();
  c->d.rnd = &c->rnd; c->d.ctr = c->ctr;
  return c;
}
void oh_destroy(oh_ctx* c) { delete c; }
uint32_t oh_longest_column(oh_ctx* c) { return c->longest; }
// overwrite the `prev` link of cell `cell`'s top section (pool_index == NIL) or of a pool record: plants a corrupt chain
void oh_set_prev(oh_ctx* c, uint64_t cell, uint32_t pool_index, uint32_t prev) {
  if (pool_index == NIL) c->cells[cell].prev = prev; else c->pool[pool_index].prev = prev;
}
uint32_t oh_top_prev(oh_ctx* c, uint64_t cell) { return c->cells[cell].prev; }

// k_ens_figures' body on one member: `lanes` = workgroup width (64 .. 256), variant = the (tile, staged types per cell) pair.
// out = 11 u64 words (ObsFigures); returns 0, -5 for a corrupt chain, -2 for an unknown variant
int oh_figures(oh_ctx* c, uint32_t lanes, int variant, void* out) {
  if (lanes == 0 || lanes > 256 || lanes % 64) return -2;
  ObsFigures r;
  memset(&r, 0, sizeof(r));
  switch (variant) {
    case 0: run_figures<256, 8>(c, lanes, &r); break;   // the kernel's own shape
    case 1: run_figures<256, 1>(c, lanes, &r); break;   // one staged type: the overflow path takes most buried sections
    case 2: run_figures<64, 0>(c, lanes, &r); break;    // nothing staged: all of them
    case 3: run_figures<96, 3>(c, lanes, &r); break;    // a tile no dimension is a multiple of
    default: return -2;
  }
  memcpy(out, &r, sizeof(r));
  return r.corrupt ? -5 : 0;
}
int oh_figures_bytes() { return (int)sizeof(ObsFigures); }
int oh_staged_types(int variant) { const int k[4] = {8, 1, 0, 3}; return variant >= 0 && variant < 4 ? k[variant] : -1; }

// k_ens_plane_stats' body over the members m[0..n) in that order (equal dims: the caller's business)
int oh_plane_stats(oh_ctx* const* m, uint32_t n, int plane, double* mean, double* var, double* vmin, double* vmax, uint32_t* nonzero) {
  if (n == 0) return -2;
  const size_t cells = (size_t)m[0]->d.dimx * m[0]->d.dimy;
  switch (plane) {
    case OBS_PLANE_HEIGHT: run_plane<OBS_PLANE_HEIGHT>(m, n, cells, mean, var, vmin, vmax, nonzero); break;
    case OBS_PLANE_WATER: run_plane<OBS_PLANE_WATER>(m, n, cells, mean, var, vmin, vmax, nonzero); break;
    case OBS_PLANE_WFREQ: run_plane<OBS_PLANE_WFREQ>(m, n, cells, mean, var, vmin, vmax, nonzero); break;
    case OBS_PLANE_WINDFREQ: run_plane<OBS_PLANE_WINDFREQ>(m, n, cells, mean, var, vmin, vmax, nonzero); break;
    default: return -2;
  }
  return 0;
}

}  // extern "C"
