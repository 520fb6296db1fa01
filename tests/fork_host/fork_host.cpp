// fork_host -- TEST-ONLY host build of soilmachine_amd/csrc/soil_fork.h (the bodies of k_fork_count, k_fork_scatter and k_fork_planes).
//
// The same header the kernels are made of, compiled by g++ and run with the lanes of a workgroup looped one after the other: one
// legal order of the device's lanes between two barriers. fh_fork is the library's driver in small: count every workgroup, scan
// the buried counts (a plain loop where the library calls rocPRIM), take the verdict, and only then scatter into the caller's
// destination image. tests/fork_host_lib.py builds and binds this file; the product never loads it.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#define SMX_D inline
#define SMX_HOSTSIM 1
#include "../../soilmachine_amd/csrc/soil_core.h"
#include "../../soilmachine_amd/csrc/soil_serial.h"
#include "../../soilmachine_amd/csrc/soil_fork.h"

using namespace smx;

struct HostGroup {   // a workgroup whose lanes the caller runs one after the other
  uint32_t n;
  uint32_t lanes() const { return n; }
  uint32_t lo() const { return 0u; }
  uint32_t hi() const { return n; }
  void barrier() const {}
};

extern "C" {

int fh_sec_bytes() { return (int)sizeof(Sec); }
int fh_rand_bytes() { return (int)sizeof(RandState); }
int fh_soil_bytes() { return (int)sizeof(SoilP); }
int fh_max_lanes() { return FORK_LANES; }

// Source image: ncells cell records, src_cap pool records, one flag byte per cell, three f32 planes of ncells values, nsoils soil
// records, the generator. Destination image: the same arrays for a pool of dst_cap records (freelist: dst_cap words), `ctr` C_COUNT
// words, written ONLY when the verdict is 0. seeded != 0: the generator is srandom_r(seed). info = {used, nonempty, bad cell}.
// Returns the verdict (0, -4, -5) or -2 for lanes outside 1..256.
int fh_fork(uint64_t ncells, const void* src_cells, const void* src_pool, uint64_t src_cap, const uint8_t* src_flags, const float* src_planes,
            const void* src_soils, uint32_t nsoils, const void* src_rnd, uint32_t lanes, uint64_t dst_cap, void* dst_cells, void* dst_pool,
            uint32_t* dst_freelist, uint32_t* dst_free_count, uint8_t* dst_flags, float* dst_planes, void* dst_soils, void* dst_rnd,
            unsigned long long* dst_ctr, uint32_t seeded, uint32_t seed, unsigned long long* info) {
  if (lanes == 0 || lanes > (uint32_t)FORK_LANES) return -2;
  ForkSrc s;
  s.cells = (const Sec*)src_cells; s.pool = (const Sec*)src_pool; s.flags = src_flags;
  // (each plane in a 16-byte aligned buffer of its own, as the device's allocations are: the body copies quads of four values)
  std::vector<ForkQuad> sp[3], dp[3];
  for (int p = 0; p < 3; p++) {
    sp[p].resize(ncells / 4 + 1); dp[p].resize(ncells / 4 + 1);
    memcpy(sp[p].data(), src_planes + p * ncells, ncells * 4);
  }
  s.wfreq = &sp[0][0].a; s.wtrack = &sp[1][0].a; s.windfreq = &sp[2][0].a;
  s.soils = (const SoilP*)src_soils; s.rnd = (const RandState*)src_rnd;
  s.cap = src_cap; s.ncells = ncells; s.nsoils = nsoils;
  std::vector<uint32_t> buried(ncells), base(ncells);
  std::vector<uint8_t> flag(ncells);
  ForkTotals tot = {0ull, 0ull, FORK_NONE};
  static ForkShared sh;   // (the "LDS")
  HostGroup g{lanes};
  const size_t nblocks = (size_t)((ncells + lanes - 1) / lanes);
  for (size_t b = 0; b < nblocks; b++) fork_count_group(s, g, b, sh, buried.data(), flag.data(), &tot);
  uint32_t acc = 0;
  for (uint64_t c = 0; c < ncells; c++) { base[c] = acc; acc += buried[c]; }   // the exclusive scan
  info[0] = tot.used; info[1] = tot.nonempty; info[2] = tot.bad;
  const int v = fork_verdict(tot, dst_cap);
  if (v != 0) return v;
  ForkDst d;
  d.cells = (Sec*)dst_cells; d.pool = (Sec*)dst_pool; d.freelist = dst_freelist; d.free_count = dst_free_count; d.flags = dst_flags;
  d.wfreq = &dp[0][0].a; d.wtrack = &dp[1][0].a; d.windfreq = &dp[2][0].a;
  d.soils = (SoilP*)dst_soils; d.rnd = (RandState*)dst_rnd; d.ctr = dst_ctr;
  d.cap = dst_cap; d.seeded = seeded; d.seed = seed;
  for (size_t b = 0; b < nblocks; b++) fork_scatter_group(s, d, g, b, nblocks, buried.data(), base.data(), flag.data(), tot);
  const uint64_t nthreads = 3 * (uint64_t)lanes;   // (a grid smaller than the planes: the stride loop runs)
  for (uint64_t t = 0; t < nthreads; t++) fork_planes_lane(s, d, t, nthreads);
  for (int p = 0; p < 3; p++) memcpy(dst_planes + p * ncells, dp[p].data(), ncells * 4);
  return 0;
}

// srandom_r(seed) as the library's smx_srand computes it (soil_serial.h)
void fh_rand_seed(uint32_t seed, void* out) { RandState r; rand_seed(r, seed); memcpy(out, &r, sizeof(r)); }
int fh_live_counter() { return (int)C_LIVE_SECTIONS; }
int fh_counters() { return (int)C_COUNT; }

}  // extern "C"
