// soilmx.hip -- HIP kernels (gfx950) and the C-ABI of include/soilmx.h.
//
// Kernels (DESIGN.md "Kernels"):
//   k_water_serial / k_wind_serial   exact engine: ONE lane walks the particles in reference order
//                                    (SoilMachine.cpp:287-298,303-307) -- the parity anchor
//   k_grid_classify                  O(cells), HBM-streaming: which cells can the grid pass change at all?
//                                    (water.h:285-343 is a provable no-op unless a water top is within the
//                                    3x3 neighbourhood or the column holds a non-zero saturation)
//   k_grid_serial                    exact walk over the (dynamic) active set in the reference's x-major order
//   k_map_frequency / k_reset_frequency   water.h:353-365, float4-vectorised streaming kernels
//   k_ens_*                          ensembles (smx_ensemble_*): the walkers above, one wavefront per member of a device
//                                    table, and the streaming kernels of the serial tick with the member in blockIdx.y
//   k_ens_figures / k_ens_plane_stats   an ensemble observed in one call (soil_observe.h): one workgroup per member folds its
//                                    digest and water figures; one thread per cell folds a plane over the selected members
//   k_strata_totals / k_strata_thickness / k_core_count / k_core_scatter   the strata read on the device (soil_strata.h): one lane
//                                    per column walks the chain -- per-type totals, thickness planes, the columns of listed cells
//   k_budget_fold / k_budget_where   the sediment budget (soil_budget.h): one lane per cell walks the column of two maps at once --
//                                    cut, fill and soil change per basin of the base, per soil type and per cell
//   k_init_terrain                   Layermap::initialize (layermap.h:163-216): FBm OpenSimplex2 per cell + column build
//   k_heights / k_surface / k_normals / k_bilinear   whole-map read-side primitives (layermap.h:341-439)
//   k_fill_vertices                  Layermap::update(Vertexpool&) (layermap.h:475-555): the 44-byte vertex stream
//
// Compile: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -shared (see __graft_entry__.build()).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include <sys/stat.h>
#include <dlfcn.h>
#include <string>
#include <vector>

#include "../../include/soilmx.h"
#ifdef SMX_PROF_FLOOD
__device__ unsigned long long g_sect[32];                    // (experiment build: soil_core.h SMX_SECT)
#endif
#include "soil_core.h"
#include "soil_serial.h"
#include "soil_spec.h"
#include <type_traits>
#include <chrono>
#include "soil_coop.h"
#include "soil_noise.h"
#include "soil_batch.h"
#include "soil_relax.h"
#include "soil_devmem.h"
#include "soil_lbm.h"
#include "soil_observe.h"
#include "soil_fork.h"
#include "soil_lakes.h"
#include "soil_drain.h"
#include "soil_spill.h"
#include "soil_through.h"
#include "soil_streams.h"
#include "soil_hills.h"
#include "soil_paths.h"
#include "soil_catch.h"
#include "soil_horizon.h"
#include "soil_prox.h"
#include "soil_disp.h"
#include "soil_strata.h"
#include "soil_budget.h"
#include "soil_scratch.h"
#include <algorithm>
#include <rocprim/rocprim.hpp>   // device radix sort of the nested particles' keys (children -> next generation, batch_generations)

using namespace smx;

static_assert(sizeof(SoilP) == sizeof(smx_soil), "smx_soil layout");
static_assert(sizeof(Sec) == 32, "Sec must be 32 bytes");

// Environment switches (experiments; README.md lists them). ONE table, read once per process -- at the first look-up or the first
// smx_switches call, whichever comes first: name, default, class and the value this process read. A call site names its switch
// (env_int / env_flag / env_str) and keeps what it makes of the value -- clamps included -- in a function-local static; a name that is not in
// the table aborts. Classes: NEUTRAL selects code or a launch shape and leaves results bit-identical (tests/test_gpu_switches.py holds every
// one of them to that); CHANGES is part of a schedule's definition (the restatement in oracle/ and tests/hostsim depend on the value:
// SMX_BATCH_CHUNK is the oracle's B_CHUNK -- the batched schedule looks at the number of running particles once per chunk --, the
// schedule pins and the relaxed steps per epoch); DIAGNOSTIC is tracing, profiling, poll pacing and the spin budget.
// A default of nullptr: the switch acts only where the variable is set.
enum { SW_NEUTRAL = 0, SW_CHANGES = 1, SW_DIAGNOSTIC = 2 };
struct EnvSwitch { const char* name; const char* dflt; int cls; };
static const EnvSwitch ENV_SWITCHES[] = {
  // exact (speculative) engine
  {"SMX_COOP", "1", SW_NEUTRAL},                      // (0: one particle per lane instead of the wave-loop kernels of soil_coop.h)
  {"SMX_SPEC_LANES", "1", SW_NEUTRAL},                // (particles per wavefront under SMX_COOP=0, 1..64)
  {"SMX_SPEC_MODE", "3", SW_NEUTRAL},                 // (bit0 blocked-particle filter, bit1 suspend/resume: water)
  {"SMX_SPEC_MODE_WIND", "2", SW_NEUTRAL},
  {"SMX_WIND_SCOUT", "1", SW_NEUTRAL},
  {"SMX_SPEC_SUB", "4096", SW_NEUTRAL},               // (top-level particles of a sub-phase, >= 64)
  {"SMX_SPEC_MAXNEST", "8192", SW_NEUTRAL},           // (nested-particle slots of a sub-phase, 128..60000)
  {"SMX_TRACE_ROUNDS", "0", SW_DIAGNOSTIC},
  // grid pass
  {"SMX_CLASSIFY_SCALAR", "0", SW_NEUTRAL},           // (1: k_grid_classify also where k_grid_classify8 fits)
  {"SMX_GRID_FLOW_WAVES", "2048", SW_NEUTRAL},        // (wavefronts of k_grid_tiles_flow, >= 1)
  {"SMX_GRID_POLL_NAPS", "2", SW_DIAGNOSTIC},         // (x 3.4 us between two polls of a waiting tile)
  // throughput engines: launch shapes
  {"SMX_BATCH_WAVES", "256", SW_NEUTRAL},             // (wavefronts the running particles are spread over; 0 = 64 per wavefront)
  {"SMX_BATCH_OCC2_ABOVE", "65536", SW_NEUTRAL},      // (running particles above which k_batch_epoch2 runs)
  {"SMX_RELAX_CHUNK_KIDS", "8", SW_NEUTRAL},          // (epochs per chunk of a nested relaxed generation: without strips the result does not depend on where a generation is cut)
  {"SMX_RELAX_TAIL", "1", SW_NEUTRAL},
  {"SMX_RELAX_TAIL_AT", "256", SW_NEUTRAL},           // (RELAX_TAIL)
  {"SMX_RELAX_MEGA", "0", SW_NEUTRAL},                // (off by default: measured slower, see k_relax_epochs)
  {"SMX_RELAX_MEGA_BLOCKS", "0", SW_NEUTRAL},         // (0: one workgroup per CU)
  {"SMX_RELAX_MEGA_WAVES", "0", SW_NEUTRAL},          // (0: one wavefront per workgroup)
  {"SMX_RELAX_MEGA_CHUNK", "0", SW_NEUTRAL},          // (0: the chunk lengths of the per-phase launches)
  {"SMX_RELAX_MEGA_FLAGS", "0", SW_NEUTRAL},          // (1: every thread fences at a barrier; 2: k_relax_epochs keeps workgroup 0's clock)
  {"SMX_RELAX_FLOOD_BLOCKS", "1024", SW_NEUTRAL},     // (floods: at least this many wavefronts to spread over)
  {"SMX_RELAX_CASC_FLOW", "1024", SW_NEUTRAL},        // (wavefronts of k_relax_cascade_flow; 0: nine launches of k_relax_cascade)
  {"SMX_RELAX_CASC_BLOCKS", "64", SW_NEUTRAL},        // (wavefronts of each of the nine launches)
  // throughput engines: the schedule itself
  {"SMX_BATCH_CHUNK", "32", SW_CHANGES},              // (B_CHUNK)
  {"SMX_BATCH_SCHED", nullptr, SW_CHANGES},           // "tshift,dilate,maxsteps" pins the water schedule
  {"SMX_BATCH_SCHED_WIND", nullptr, SW_CHANGES},
  {"SMX_BATCH_SCHED_TAIL", nullptr, SW_CHANGES},      // "thr:tshift,dilate,maxsteps[;thr2:...]" (ascending thr): first thr >= nlive wins
  {"SMX_BATCH_SCHED_TAIL_WIND", nullptr, SW_CHANGES},
  {"SMX_RELAX_WIND_MIN", nullptr, SW_CHANGES},        // (running wind particles above which the wind phase is relaxed)
  {"SMX_RELAX_WATER_STEPS", "0", SW_CHANGES},         // (1..R_MAXSTEPS; 0: the context's own)
  {"SMX_RELAX_WIND_STEPS", "0", SW_CHANGES},
  // diagnostics
  {"SMX_TRACE_BATCH", "0", SW_DIAGNOSTIC},
  {"SMX_FLOOD_PROF", "0", SW_DIAGNOSTIC},             // (not 0: k_relax_floods and k_grid_tiles_flow keep duration histograms, printed by smx_destroy)
  {"SMX_STEP_EVENT_SAMPLE", "8", SW_DIAGNOSTIC},      // (every n-th launch of the relaxed step kernel sits between a pair of events)
  {"SMX_SPIN_BUDGET", "-1", SW_DIAGNOSTIC},           // (polls a dataflow wait may last; < 0: the kernels' own)
  // LBM wind
  {"SMX_LBM_NT", "0", SW_NEUTRAL},
  {"SMX_LBM_XCD", "0", SW_NEUTRAL},
};
constexpr int N_ENV_SWITCHES = (int)(sizeof(ENV_SWITCHES) / sizeof(ENV_SWITCHES[0]));
static_assert(B_CHUNK == 32, "the default of SMX_BATCH_CHUNK in ENV_SWITCHES is B_CHUNK");
struct EnvValues { const char* v[N_ENV_SWITCHES]; };          // what the process read: the variable's text, or the default where it is not set
static const EnvValues& env_values() {
  static const EnvValues vals = [] {
    EnvValues r;
    for (int i = 0; i < N_ENV_SWITCHES; i++) {
      const char* e = getenv(ENV_SWITCHES[i].name);
      r.v[i] = e ? strdup(e) : ENV_SWITCHES[i].dflt;          // (a copy: a later setenv does not reach a switch that was read)
    }
    return r;
  }();
  return vals;
}
static const char* env_str(const char* name) {
  for (int i = 0; i < N_ENV_SWITCHES; i++)
    if (!strcmp(ENV_SWITCHES[i].name, name)) return env_values().v[i];
  fprintf(stderr, "[soilmx] %s is not in ENV_SWITCHES\n", name);
  abort();
}
static long long env_int(const char* name) { const char* e = env_str(name); return e ? atoll(e) : 0; }
static bool env_flag(const char* name) { return env_int(name) != 0; }
// ... and the switches that more than one site reads
static uint32_t flood_prof() { static const uint32_t v = (uint32_t)env_int("SMX_FLOOD_PROF"); return v; }
static uint32_t relax_mega_flags() { static const uint32_t v = (uint32_t)env_int("SMX_RELAX_MEGA_FLAGS"); return v; }
static bool trace_batch() { static const bool on = env_flag("SMX_TRACE_BATCH"); return on; }
static bool coop_on() { static const bool on = env_flag("SMX_COOP"); return on; }

// ------------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------------
// soil table -> LDS (<= 14 KB); every lane helps, then lane 0 walks
#define SMX_LOAD_SOILS(sh)                                                                          \
  __shared__ SoilP sh[MAX_SOILS];                                                                   \
  for (uint32_t i_ = threadIdx.x; i_ < s.nsoils * (sizeof(SoilP) / 4); i_ += blockDim.x)            \
    reinterpret_cast<uint32_t*>(sh)[i_] = reinterpret_cast<const uint32_t*>(s.soils)[i_];           \
  __syncthreads();

__global__ void __launch_bounds__(64) k_water_serial(DevState s, int n) {
  SMX_LOAD_SOILS(sh)
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  serial_water_walk(s, sh, n);
}

__global__ void __launch_bounds__(64) k_wind_serial(DevState s, int n) {
  SMX_LOAD_SOILS(sh)
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  serial_wind_walk(s, sh, n);
}

// Classification of the grid pass, block `blk` of a context: one thread per cell, 256 consecutive cells (cell order) per block =
// 4 level-0 bitmap words.
SMX_D void grid_classify_block(const DevState& s, size_t blk) {
  const size_t n = (size_t)s.x_hi * s.dimy;
  const size_t c = (size_t)s.x_lo * s.dimy + blk * 256 + threadIdx.x;   // (x_lo*dimy is a multiple of 64: launch_classify)
  bool act = false;
  if (c < n) {
    const int x = (int)(c / s.dimy), y = (int)(c % s.dimy);
    uint8_t f = s.flags[c];
    act = (f & F_SAT) != 0;
    uint8_t any = f;
    const bool xm = x > s.x_lo, xp = x < s.x_hi - 1, ym = y > 0, yp = y < s.dimy - 1;
    if (ym) any |= s.flags[c - 1];
    if (yp) any |= s.flags[c + 1];
    if (xm) { any |= s.flags[c - s.dimy]; if (ym) any |= s.flags[c - s.dimy - 1]; if (yp) any |= s.flags[c - s.dimy + 1]; }
    if (xp) { any |= s.flags[c + s.dimy]; if (ym) any |= s.flags[c + s.dimy - 1]; if (yp) any |= s.flags[c + s.dimy + 1]; }
    act = act || (any & F_AIR);
  }
  const unsigned long long m = __ballot(act);
  if ((threadIdx.x & 63) == 0 && c < n) {
    const size_t w0 = c >> 6;
    s.active[w0] = m;
    if (m) {
      atomicOr(&s.active1[w0 >> 6], 1ull << (w0 & 63));
      atomicOr(&s.active2[w0 >> 12], 1ull << ((w0 >> 6) & 63));
    }
  }
}
__global__ void __launch_bounds__(256) k_grid_classify(DevState s) { grid_classify_block(s, blockIdx.x); }

// The same, eight cells per thread (dimy a multiple of 8: a thread's cells lie in one map row x): three aligned 8-byte
// loads of flag bytes (rows x-1, x, x+1) + the two flanking bytes of each row instead of nine byte loads per cell; a
// wave writes eight complete 64-bit words of the bitmap. 1 B/cell read, 1 bit/cell written: an HBM-streaming kernel.
// `sm`: 32 words of LDS (256 threads x 8 bits).
SMX_D void grid_classify8_block(const DevState& s, size_t blk, unsigned long long* sm) {
  const size_t n = (size_t)s.x_hi * s.dimy, c_lo = (size_t)s.x_lo * s.dimy;   // (c_lo is a multiple of 64: launch_classify)
  const size_t c = c_lo + (blk * 256 + threadIdx.x) * 8;
  uint32_t act = 0;
  if (c < n) {
    const int x = (int)(c / s.dimy), y = (int)(c % s.dimy);
    const bool xm = x > s.x_lo, xp = x < s.x_hi - 1, ym = y > 0, yp = y + 8 < s.dimy;
    const unsigned long long zero = 0ull;
    const unsigned long long r0 = *reinterpret_cast<const unsigned long long*>(s.flags + c);
    const unsigned long long rm = xm ? *reinterpret_cast<const unsigned long long*>(s.flags + c - s.dimy) : zero;
    const unsigned long long rp = xp ? *reinterpret_cast<const unsigned long long*>(s.flags + c + s.dimy) : zero;
    uint32_t lo = 0, hi = 0;                                 // flag bytes left of cell 0 / right of cell 7, the three rows or-ed
    if (ym) { lo |= s.flags[c - 1]; if (xm) lo |= s.flags[c - s.dimy - 1]; if (xp) lo |= s.flags[c + s.dimy - 1]; }
    if (yp) { hi |= s.flags[c + 8]; if (xm) hi |= s.flags[c - s.dimy + 8]; if (xp) hi |= s.flags[c + s.dimy + 8]; }
    const unsigned long long col = r0 | rm | rp;             // per cell: own column of three rows
    // F_AIR anywhere in the 3x3: the cell's own column or-ed with its left and right neighbours'
    const unsigned long long airc = col & 0x0101010101010101ull * F_AIR;
    const unsigned long long left = (airc << 8) | (unsigned long long)(lo & F_AIR);
    const unsigned long long right = (airc >> 8) | ((unsigned long long)(hi & F_AIR) << 56);
    const unsigned long long any = airc | left | right | ((r0 & (0x0101010101010101ull * F_SAT)) >> 1);   // F_SAT = 2 -> bit 0
#pragma unroll
    for (int k = 0; k < 8; k++) act |= (uint32_t)((any >> (8 * k)) & 1ull) << k;
  }
  reinterpret_cast<uint8_t*>(sm)[threadIdx.x] = (uint8_t)act;
  __syncthreads();
  if (threadIdx.x < 32) {
    const size_t w0 = (c_lo >> 6) + blk * 32 + threadIdx.x;   // 2048 cells per block = 32 bitmap words
    if (w0 * 64 < n) {
      const unsigned long long m = sm[threadIdx.x];
      s.active[w0] = m;
      if (m) {
        atomicOr(&s.active1[w0 >> 6], 1ull << (w0 & 63));
        atomicOr(&s.active2[w0 >> 12], 1ull << ((w0 >> 6) & 63));
      }
    }
  }
}
__global__ void __launch_bounds__(256) k_grid_classify8(DevState s) {
  __shared__ unsigned long long sm[32];
  grid_classify8_block(s, blockIdx.x, sm);
}

__global__ void __launch_bounds__(64) k_grid_serial(DevState s) {
  SMX_LOAD_SOILS(sh)
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  serial_grid_walk(s, sh);
}

// ---------------- ensembles of exact contexts (smx_ensemble_*): one launch per phase for every member ----------------
// The host re-uploads the table every tick (smx_set_soils / smx_set_scale change a member's DevState between ticks). A member that
// sits a tick out (on == 0) returns at once in every kernel; bounds come from each member's own DevState (members differ in dims).
struct EnsEntry {
  DevState s;
  int32_t nwater, nwind;   // this tick's particle counts
  int32_t on;              // 0: the member sits this tick out
  int32_t classify8;       // the eight-cells-per-thread classification applies (launch_classify's rule)
};

// The table is written only by the copy queued before a tick's launches, so inside a kernel it is constant memory. Read through the
// constant address space, the compiler may re-load a member's DevState fields (scalar loads) instead of keeping them live in registers
// across the walk -- as it does with a kernel argument: k_ens_wind through a generic pointer took 256 VGPR + 42 AGPR and one wave per
// SIMD, through this one it takes the 190 VGPR and two waves of k_wind_serial (profiles/r07_ensemble_kernel_resources.md).
#if defined(__HIP_DEVICE_COMPILE__)
typedef const EnsEntry __attribute__((address_space(4))) EnsTab;
#else
typedef const EnsEntry EnsTab;   // (the host pass only parses the kernels)
#endif
SMX_D EnsTab* ens_tab(const EnsEntry* p) { return (EnsTab*)p; }

// one wavefront per member (blockIdx.x): the walkers of k_water_serial / k_wind_serial / k_grid_serial on the member's state
__global__ void __launch_bounds__(64) k_ens_water(const EnsEntry* __restrict__ tab_) {
  EnsTab* tab = ens_tab(tab_);
  if (!tab[blockIdx.x].on) return;
  const DevState s = tab[blockIdx.x].s;
  const int n = tab[blockIdx.x].nwater;
  SMX_LOAD_SOILS(sh)
  if (threadIdx.x != 0) return;
  serial_water_walk(s, sh, n);
}
__global__ void __launch_bounds__(64) k_ens_wind(const EnsEntry* __restrict__ tab_) {
  EnsTab* tab = ens_tab(tab_);
  if (!tab[blockIdx.x].on) return;
  const DevState s = tab[blockIdx.x].s;
  const int n = tab[blockIdx.x].nwind;
  SMX_LOAD_SOILS(sh)
  if (threadIdx.x != 0) return;
  serial_wind_walk(s, sh, n);
}
__global__ void __launch_bounds__(64) k_ens_grid(const EnsEntry* __restrict__ tab_) {
  EnsTab* tab = ens_tab(tab_);
  if (!tab[blockIdx.x].on) return;
  const DevState s = tab[blockIdx.x].s;
  SMX_LOAD_SOILS(sh)
  if (threadIdx.x != 0) return;
  serial_grid_walk(s, sh);
}
// the grid pass's memsets of the bitmap's summary levels (smx_grid_pass): one workgroup per member, the words create_range allocated
__global__ void __launch_bounds__(256) k_ens_grid_clear(const EnsEntry* __restrict__ tab_) {
  EnsTab* tab = ens_tab(tab_);
  if (!tab[blockIdx.x].on) return;
  const DevState s = tab[blockIdx.x].s;
  const size_t n = (size_t)s.dimx * s.dimy, nw0 = (n + 63) >> 6, nw1 = (nw0 + 63) >> 6, nw2 = (nw1 + 63) >> 6;
  for (size_t i = threadIdx.x; i < nw1 + 64; i += blockDim.x) s.active1[i] = 0ull;
  for (size_t i = threadIdx.x; i < nw2 + 64; i += blockDim.x) s.active2[i] = 0ull;
}
// k_grid_classify / k_grid_classify8, member blockIdx.y, block blockIdx.x of that member's cells
__global__ void __launch_bounds__(256) k_ens_classify(const EnsEntry* __restrict__ tab_) {
  EnsTab* tab = ens_tab(tab_);
  __shared__ unsigned long long sm[32];
  if (!tab[blockIdx.y].on) return;
  const DevState s = tab[blockIdx.y].s;
  const size_t n = (size_t)s.dimx * s.dimy;
  if (tab[blockIdx.y].classify8) {
    if ((size_t)blockIdx.x * 2048 >= n) return;
    grid_classify8_block(s, blockIdx.x, sm);
  } else {
    if ((size_t)blockIdx.x * 256 >= n) return;
    grid_classify_block(s, blockIdx.x);
  }
}

// ---------------- an ensemble observed as one thing (smx_ensemble_figures / smx_ensemble_plane_stats; bodies: soil_observe.h) ----------------
struct ObsGroup {   // a workgroup as soil_observe.h sees it: this thread is one lane
  SMX_D uint32_t lanes() const { return blockDim.x; }
  SMX_D uint32_t lo() const { return threadIdx.x; }
  SMX_D uint32_t hi() const { return threadIdx.x + 1u; }
  SMX_D void barrier() const { __syncthreads(); }
};
// 256 cells per tile and 8 staged buried types per cell: two tiles + the partials are 41 KB of LDS, three workgroups per CU
constexpr int FIG_TILE = 256, FIG_K = 8, FIG_LANES = 256;
// one workgroup per member (blockIdx.x): wavefront 0 folds the type hash, wavefront 1 the two f64 sums, wavefronts 2-3 stage the next tile
__global__ void __launch_bounds__(FIG_LANES) k_ens_figures(const EnsEntry* __restrict__ tab_, ObsFigures* __restrict__ out) {
  EnsTab* tab = ens_tab(tab_);
  __shared__ FigShared<FIG_TILE, FIG_K, FIG_LANES> sh;
  const DevState s = tab[blockIdx.x].s;
  ObsGroup g;
  figures_group<FIG_TILE, FIG_K, FIG_LANES>(s, g, sh, out + blockIdx.x);
}
// the table holds the SELECTED members in fold order (smx_ensemble_plane_stats uploads it so): entry i is member which[i]
struct ObsMembers {
  EnsTab* tab;
  SMX_D const Sec* cells(uint32_t i) const { return tab[i].s.cells; }
  SMX_D const float* wfreq(uint32_t i) const { return tab[i].s.wfreq; }
  SMX_D const float* windfreq(uint32_t i) const { return tab[i].s.windfreq; }
};
// one thread per cell of the plane (its own index), a loop over the selected members: adjacent lanes read adjacent records of one member
template <int PLANE>
__global__ void __launch_bounds__(256) k_ens_plane_stats(const EnsEntry* __restrict__ tab_, uint32_t n, size_t cells, double* __restrict__ mean,
                                                         double* __restrict__ var, double* __restrict__ vmin, double* __restrict__ vmax,
                                                         uint32_t* __restrict__ nonzero) {
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= cells) return;
  const ObsMembers m{ens_tab(tab_)};
  plane_stats_cell<PLANE>(m, n, c, mean, var, vmin, vmax, nonzero);
}

// ---------------- forking a map on the device (smx_copy_state / smx_ensemble_fork; bodies: soil_fork.h) ----------------
// one lane per cell, adjacent lanes on adjacent 32-byte cell records
__global__ void __launch_bounds__(FORK_LANES) k_fork_count(ForkSrc s, uint32_t* __restrict__ buried, uint8_t* __restrict__ flag, ForkTotals* __restrict__ tot) {
  __shared__ ForkShared sh;
  ObsGroup g;
  fork_count_group(s, g, blockIdx.x, sh, buried, flag, tot);
}
// destination blockIdx.y of the table (tab == null: the one destination `one`), workgroup blockIdx.x of its cells
__global__ void __launch_bounds__(FORK_LANES) k_fork_scatter(ForkSrc s, const uint32_t* __restrict__ buried, const uint32_t* __restrict__ base,
                                                             const uint8_t* __restrict__ flag, ForkTotals tot, const ForkDst* __restrict__ tab, ForkDst one) {
  const ForkDst d = tab ? tab[blockIdx.y] : one;
  ObsGroup g;
  fork_scatter_group(s, d, g, blockIdx.x, gridDim.x, buried, base, flag, tot);
}
__global__ void __launch_bounds__(256) k_fork_planes(ForkSrc s, const ForkDst* __restrict__ tab, ForkDst one) {
  const ForkDst d = tab ? tab[blockIdx.y] : one;
  fork_planes_lane(s, d, (uint64_t)blockIdx.x * 256 + threadIdx.x, (uint64_t)gridDim.x * 256);
}

// ---------------- the lake census (smx_lakes / smx_ensemble_lakes; bodies: soil_lakes.h) ----------------
// Member blockIdx.y of the table, workgroup blockIdx.x of ITS tiles / cells (the grid is sized for the largest member). A tile is 16
// columns of 64 cells: a wavefront reads 64 consecutive 32-byte records, the tile's labels are 4 KB of LDS; the statistics table
// holds 512 cells' worth of lakes (30 KB of LDS).
constexpr int LAKE_TX = 16, LAKE_TY = 64, LAKE_LANES = 256, LAKE_SLOTS = 512;
__global__ void __launch_bounds__(LAKE_LANES) k_lake_tiles(const LakeMember* __restrict__ tab, uint32_t* A, LakeAcc* acc) {
  __shared__ uint32_t lab[LAKE_TX * LAKE_TY];
  const LakeMember m = tab[blockIdx.y];
  const uint32_t nt = lake_tiles(m, LAKE_TX, LAKE_TY);
  if (blockIdx.x >= nt) return;
  ObsGroup g;
  lake_tile_group<LAKE_TX, LAKE_TY>(m, g, blockIdx.x, nt, lab, A, acc);
}
__global__ void __launch_bounds__(LAKE_LANES) k_lake_merge(const LakeMember* __restrict__ tab, uint32_t* A) {
  const LakeMember m = tab[blockIdx.y];
  if (blockIdx.x >= lake_tiles(m, LAKE_TX, LAKE_TY)) return;
  ObsGroup g;
  lake_merge_group<LAKE_TX, LAKE_TY>(m, g, blockIdx.x, A);
}
__global__ void __launch_bounds__(LAKE_LANES) k_lake_flatten(const LakeMember* __restrict__ tab, uint32_t* A) {
  const LakeMember m = tab[blockIdx.y];
  if ((uint64_t)blockIdx.x * LAKE_LANES >= (uint64_t)m.dimx * (uint64_t)m.dimy) return;
  ObsGroup g;
  lake_flatten_group(m, g, blockIdx.x, A);
}
__global__ void __launch_bounds__(LAKE_LANES) k_lake_stats(const LakeMember* __restrict__ tab, uint32_t* A, const uint32_t* __restrict__ B, LakeAcc* acc,
                                                           uint32_t* nlakes) {
  __shared__ LakeTable<LAKE_SLOTS> t;
  const LakeMember m = tab[blockIdx.y];
  if ((uint64_t)blockIdx.x * lake_stats_cells(LAKE_SLOTS, LAKE_LANES) >= (uint64_t)m.dimx * (uint64_t)m.dimy) return;
  ObsGroup g;
  lake_stats_group<LAKE_SLOTS>(m, g, blockIdx.x, t, A, B, acc, nlakes + blockIdx.y);
}
struct LakeMarkFn {   // the scan's input: 1 where plane word g is a root
  const uint32_t* A;
  __host__ __device__ uint32_t operator()(uint32_t g) const { return lake_mark(A, g); }
};

// ---------------- drainage (smx_drainage / smx_ensemble_drainage; bodies: soil_drain.h) ----------------
// The census's tiles, lanes and table size: the height tile with its halo of one is 18 x 66 doubles (9.3 KB of LDS), the statistics
// table holds 512 cells' worth of basins (24 KB).
__global__ void __launch_bounds__(LAKE_LANES) k_drain_recv(const LakeMember* __restrict__ tab, uint32_t* T, uint32_t* R, BasinAcc* acc) {
  __shared__ double hs[(LAKE_TX + 2) * (LAKE_TY + 2)];
  const LakeMember m = tab[blockIdx.y];
  const uint32_t nt = lake_tiles(m, LAKE_TX, LAKE_TY);
  if (blockIdx.x >= nt) return;
  ObsGroup g;
  drain_recv_group<LAKE_TX, LAKE_TY>(m, g, blockIdx.x, nt, hs, T, R, acc);
}
__global__ void __launch_bounds__(LAKE_LANES) k_drain_resolve(const LakeMember* __restrict__ tab, uint32_t* T) {
  const LakeMember m = tab[blockIdx.y];
  if ((uint64_t)blockIdx.x * LAKE_LANES >= (uint64_t)m.dimx * (uint64_t)m.dimy) return;
  ObsGroup g;
  drain_resolve_group(m, g, blockIdx.x, T);
}
__global__ void __launch_bounds__(LAKE_LANES) k_drain_stats(const LakeMember* __restrict__ tab, uint32_t* T, const uint32_t* __restrict__ B, BasinAcc* acc,
                                                            uint32_t* nbasins) {
  __shared__ BasinTable<LAKE_SLOTS> t;
  const LakeMember m = tab[blockIdx.y];
  if ((uint64_t)blockIdx.x * lake_stats_cells(LAKE_SLOTS, LAKE_LANES) >= (uint64_t)m.dimx * (uint64_t)m.dimy) return;
  ObsGroup g;
  drain_stats_group<LAKE_SLOTS>(m, g, blockIdx.x, t, T, B, acc, nbasins + blockIdx.y);
}
__global__ void __launch_bounds__(LAKE_LANES) k_drain_pending(const LakeMember* __restrict__ tab, const uint32_t* __restrict__ R, uint32_t* P, uint32_t* AR) {
  const LakeMember m = tab[blockIdx.y];
  if ((uint64_t)blockIdx.x * LAKE_LANES >= (uint64_t)m.dimx * (uint64_t)m.dimy) return;
  ObsGroup g;
  drain_pending_group(m, g, blockIdx.x, R, P, AR);
}
__global__ void __launch_bounds__(LAKE_LANES) k_drain_area(const LakeMember* __restrict__ tab, const uint32_t* __restrict__ R, uint32_t* P, uint32_t* AR) {
  const LakeMember m = tab[blockIdx.y];
  if ((uint64_t)blockIdx.x * LAKE_LANES >= (uint64_t)m.dimx * (uint64_t)m.dimy) return;
  ObsGroup g;
  drain_area_group(m, g, blockIdx.x, R, P, AR);
}

// ---------------- the stream network (smx_streams / smx_ensemble_streams; bodies: soil_streams.h) ----------------
// One lane per cell, the census's workgroup width. k_stream_order and k_stream_segments are lane-serial walks: a wavefront is busy as
// long as its longest walk.
struct StreamPlanes {   // the u32 planes of one call (soil_streams.h)
  uint32_t *T, *R, *P, *AR, *D, *O, *H, *RE, *B, *SG;
};
__global__ void __launch_bounds__(LAKE_LANES) k_stream_mark(const LakeMember* __restrict__ tab, uint32_t threshold, StreamPlanes p) {
  const LakeMember m = tab[blockIdx.y];
  if ((uint64_t)blockIdx.x * LAKE_LANES >= (uint64_t)m.dimx * (uint64_t)m.dimy) return;
  ObsGroup g;
  stream_mark_group(m, g, blockIdx.x, threshold, p.R, p.AR, p.D, p.P, p.O, p.H, p.RE, p.SG);
}
__global__ void __launch_bounds__(LAKE_LANES) k_stream_order(const LakeMember* __restrict__ tab, uint32_t threshold, StreamPlanes p) {
  const LakeMember m = tab[blockIdx.y];
  if ((uint64_t)blockIdx.x * LAKE_LANES >= (uint64_t)m.dimx * (uint64_t)m.dimy) return;
  ObsGroup g;
  stream_order_group(m, g, blockIdx.x, threshold, p.R, p.AR, p.D, p.P, p.O, p.H, p.RE);
}
__global__ void __launch_bounds__(LAKE_LANES) k_stream_segments(const LakeMember* __restrict__ tab, int with_plane, StreamPlanes p, StreamRec* out, uint32_t* nstreams) {
  const LakeMember m = tab[blockIdx.y];
  if ((uint64_t)blockIdx.x * LAKE_LANES >= (uint64_t)m.dimx * (uint64_t)m.dimy) return;
  ObsGroup g;
  stream_segments_group(m, g, blockIdx.x, with_plane != 0, p.T, p.R, p.AR, p.D, p.O, p.H, p.B, p.SG, out, nstreams + blockIdx.y);
}
struct StreamMarkFn {   // the scan's input: 1 where plane word g starts a segment
  const uint32_t* D;
  __host__ __device__ uint32_t operator()(uint32_t g) const { return stream_mark(D, g); }
};

// ---------------- the hillslopes (smx_hillslopes / smx_ensemble_hillslopes; bodies: soil_hills.h) ----------------
// Behind the streams chain, on its planes. k_hill_init and k_hill_jump take one lane per cell and stream: a round of k_hill_jump reads
// three words, gathers three and writes three per cell. k_hill_fold's table holds 512 cells' worth of segments (30 KB of LDS).
struct HillSet {   // one of the two sets k_hill_jump writes in turns: the jump pointer and the steps to it
  uint32_t *J, *S, *G;
};
__global__ void __launch_bounds__(LAKE_LANES) k_hill_init(const LakeMember* __restrict__ tab, const uint32_t* __restrict__ SG, HillSet s, HillAcc* acc) {
  const LakeMember m = tab[blockIdx.y];
  const uint64_t n = (uint64_t)m.dimx * (uint64_t)m.dimy;
  if ((uint64_t)blockIdx.x * LAKE_LANES >= n) return;
  ObsGroup g;
  hill_init_group(m, g, blockIdx.x, (uint32_t)((n + LAKE_LANES - 1) / LAKE_LANES), SG, s.J, s.S, s.G, acc);
}
__global__ void __launch_bounds__(LAKE_LANES) k_hill_jump(const LakeMember* __restrict__ tab, HillSet from, HillSet to) {
  const LakeMember m = tab[blockIdx.y];
  if ((uint64_t)blockIdx.x * LAKE_LANES >= (uint64_t)m.dimx * (uint64_t)m.dimy) return;
  ObsGroup g;
  hill_jump_group(m, g, blockIdx.x, from.J, from.S, from.G, to.J, to.S, to.G);
}
__global__ void __launch_bounds__(LAKE_LANES) k_hill_fold(const LakeMember* __restrict__ tab, HillSet s, const uint32_t* __restrict__ SG, const uint32_t* __restrict__ D,
                                                          const uint32_t* __restrict__ B, HillAcc* acc, uint32_t* nsegments, uint32_t* entry, uint32_t* hillslope,
                                                          double* hand) {
  __shared__ HillTable<LAKE_SLOTS> t;
  const LakeMember m = tab[blockIdx.y];
  if ((uint64_t)blockIdx.x * lake_stats_cells(LAKE_SLOTS, LAKE_LANES) >= (uint64_t)m.dimx * (uint64_t)m.dimy) return;
  ObsGroup g;
  hill_fold_group<LAKE_SLOTS>(m, g, blockIdx.x, t, s.J, s.S, s.G, SG, D, B, acc, nsegments + blockIdx.y, entry, hillslope, hand);
}

// ---------------- the flow paths (smx_flowpaths / smx_ensemble_flowpaths; bodies: soil_paths.h) ----------------
// Behind the drainage chain and k_drain_pending, on their planes; the pointer doubling is k_hill_jump. One lane per cell throughout;
// k_path_up is the lane-serial walk of k_drain_area with a 64-bit max for the add. k_path_fold's table holds 512 cells' worth of
// basins (20 KB of LDS).
struct PathPlanes {   // what the kernels behind the jump rounds work on (soil_paths.h): s the settled set
  uint32_t *T, *R, *P, *FH, *FS, *L, *PA;
  uint64_t* UP;
  HillSet s;
};
__global__ void __launch_bounds__(LAKE_LANES) k_path_init(const LakeMember* __restrict__ tab, const uint32_t* __restrict__ R, HillSet s, uint32_t* FH, PathAcc* acc) {
  const LakeMember m = tab[blockIdx.y];
  const uint64_t n = (uint64_t)m.dimx * (uint64_t)m.dimy;
  if ((uint64_t)blockIdx.x * LAKE_LANES >= n) return;
  ObsGroup g;
  path_init_group(m, g, blockIdx.x, (uint32_t)((n + LAKE_LANES - 1) / LAKE_LANES), R, s.J, s.S, s.G, FH, acc);
}
__global__ void __launch_bounds__(LAKE_LANES) k_path_fold(const LakeMember* __restrict__ tab, PathPlanes p, PathAcc* acc) {
  __shared__ PathTable<LAKE_SLOTS> t;
  const LakeMember m = tab[blockIdx.y];
  if ((uint64_t)blockIdx.x * lake_stats_cells(LAKE_SLOTS, LAKE_LANES) >= (uint64_t)m.dimx * (uint64_t)m.dimy) return;
  ObsGroup g;
  path_fold_group<LAKE_SLOTS>(m, g, blockIdx.x, t, p.T, p.R, p.s.J, p.s.S, p.s.G, p.UP, p.FH, p.FS, acc);
}
__global__ void __launch_bounds__(LAKE_LANES) k_path_up(const LakeMember* __restrict__ tab, PathPlanes p) {
  const LakeMember m = tab[blockIdx.y];
  if ((uint64_t)blockIdx.x * LAKE_LANES >= (uint64_t)m.dimx * (uint64_t)m.dimy) return;
  ObsGroup g;
  path_up_group(m, g, blockIdx.x, p.R, p.P, p.UP);
}
__global__ void __launch_bounds__(LAKE_LANES) k_path_lengths(const LakeMember* __restrict__ tab, PathPlanes p, const uint32_t* __restrict__ nbasins) {
  const LakeMember m = tab[blockIdx.y];
  if ((uint64_t)blockIdx.x * LAKE_LANES >= (uint64_t)m.dimx * (uint64_t)m.dimy) return;
  ObsGroup g;
  path_lengths_group(m, g, blockIdx.x, p.T, p.s.S, p.s.G, p.FH, p.FS, p.L, nbasins + blockIdx.y);
}
__global__ void __launch_bounds__(LAKE_LANES) k_path_stem(const LakeMember* __restrict__ tab, PathPlanes p, PathAcc* acc, const uint32_t* __restrict__ nbasins,
                                                          uint32_t* nprofile, PathOut o) {
  const LakeMember m = tab[blockIdx.y];
  if ((uint64_t)blockIdx.x * LAKE_LANES >= (uint64_t)m.dimx * (uint64_t)m.dimy) return;
  ObsGroup g;
  path_stem_group(m, g, blockIdx.x, p.T, p.s.J, p.s.S, p.s.G, p.UP, p.FH, p.FS, p.PA, acc, nbasins + blockIdx.y, nprofile + blockIdx.y, o);
}

// ---------------- the catchments of listed outlets (smx_catchments / smx_ensemble_catchments; bodies: soil_catch.h) ----------------
// Behind the drainage chain with its statistics and without its area step, on its planes; the pointer doubling is k_hill_jump.
// k_catch_mark takes one lane per list entry, the others one lane per cell. k_catch_fold's table holds 512 cells' worth of gauges
// (26 KB of LDS), k_catch_hist's 512 cells' worth of (gauge, bin) keys (4 KB).
struct CatchPlanes {   // what the kernels around the jump rounds work on (soil_catch.h): s the first set for k_catch_init, the settled one behind the rounds
  uint32_t *T, *R, *M;
  HillSet s;
};
__global__ void __launch_bounds__(LAKE_LANES) k_catch_mark(const LakeMember* __restrict__ tab, const uint32_t* __restrict__ list, uint32_t n, uint32_t* M) {
  const LakeMember m = tab[blockIdx.y];
  ObsGroup g;
  catch_mark_group(m, g, blockIdx.x, list, n, M);
}
__global__ void __launch_bounds__(LAKE_LANES) k_catch_init(const LakeMember* __restrict__ tab, CatchPlanes p, CatchAcc* acc) {
  const LakeMember m = tab[blockIdx.y];
  const uint64_t n = (uint64_t)m.dimx * (uint64_t)m.dimy;
  if ((uint64_t)blockIdx.x * LAKE_LANES >= n) return;
  ObsGroup g;
  catch_init_group(m, g, blockIdx.x, (uint32_t)((n + LAKE_LANES - 1) / LAKE_LANES), p.R, p.M, p.s.J, p.s.S, p.s.G, acc);
}
__global__ void __launch_bounds__(LAKE_LANES) k_catch_fold(const LakeMember* __restrict__ tab, CatchPlanes p, CatchAcc* acc, uint32_t* gauge, double* drop) {
  __shared__ CatchTable<LAKE_SLOTS> t;
  const LakeMember m = tab[blockIdx.y];
  if ((uint64_t)blockIdx.x * lake_stats_cells(LAKE_SLOTS, LAKE_LANES) >= (uint64_t)m.dimx * (uint64_t)m.dimy) return;
  ObsGroup g;
  catch_fold_group<LAKE_SLOTS>(m, g, blockIdx.x, t, p.T, p.R, p.M, p.s.J, p.s.S, p.s.G, acc, gauge, drop);
}
__global__ void __launch_bounds__(LAKE_LANES) k_catch_hist(const LakeMember* __restrict__ tab, CatchPlanes p, uint32_t* hist, uint32_t nbins, double bin_height) {
  __shared__ CatchHistTable<LAKE_SLOTS> t;
  const LakeMember m = tab[blockIdx.y];
  if ((uint64_t)blockIdx.x * lake_stats_cells(LAKE_SLOTS, LAKE_LANES) >= (uint64_t)m.dimx * (uint64_t)m.dimy) return;
  ObsGroup g;
  catch_hist_group<LAKE_SLOTS>(m, g, blockIdx.x, t, p.M, p.s.J, hist, nbins, bin_height);
}

// ---------------- the horizons (smx_horizons / smx_ensemble_horizons; bodies: soil_horizon.h) ----------------
// On planes of their own: no drainage chain in front. k_horizon_heights takes a workgroup per coarse tile (64 x 64 cells, a wavefront
// on 64 consecutive records of a column; 520 bytes of LDS), k_horizon_scan a workgroup per 256 consecutive cells and selected
// direction (blockIdx.z; 288 bytes of LDS), k_horizon_sky a lane per cell. The table holds every member twice: tab[y] as everywhere,
// tab[gridDim.y + y] the view of its tiles.
struct HorizonPlanes {   // what the three kernels work on: the scan's view, the planes of all directions (null: not kept) and the fold's tables
  double *H, *FM, *CM;
  uint64_t* MM;
  double* S; uint32_t* K;
  HorizonAcc* acc; uint32_t* lit_cells;
  const HorizonSun* suns; uint32_t nsuns;
  uint64_t words;
};
__global__ void __launch_bounds__(LAKE_LANES) k_horizon_heights(const LakeMember* __restrict__ tab, HorizonPlanes p) {
  __shared__ HorizonTileMax<HORIZON_FINE, HORIZON_COARSE> s;
  const LakeMember m = tab[blockIdx.y], t = tab[gridDim.y + blockIdx.y];
  if (blockIdx.x >= horizon_tiles(m, HORIZON_COARSE)) return;
  ObsGroup g;
  horizon_heights_group<HORIZON_FINE, HORIZON_COARSE>(m, t, g, blockIdx.x, s, p.H, p.FM, p.CM, p.MM);
}
__global__ void __launch_bounds__(LAKE_LANES) k_horizon_scan(const LakeMember* __restrict__ tab, HorizonPlanes p, uint32_t mask, uint32_t reach) {
  __shared__ HorizonFold f;
  const LakeMember m = tab[blockIdx.y], t = tab[gridDim.y + blockIdx.y];
  if ((uint64_t)blockIdx.x * LAKE_LANES >= (uint64_t)m.dimx * (uint64_t)m.dimy) return;
  ObsGroup g;
  const HorizonView v{p.H, p.FM, p.CM, p.MM};
  horizon_scan_group<HORIZON_FINE, HORIZON_COARSE>(m, t, g, blockIdx.x, f, v, horizon_nth(mask, blockIdx.z), blockIdx.z, reach, p.suns, p.nsuns, p.words, p.S, p.K, p.acc,
                                                   p.lit_cells);
}
__global__ void __launch_bounds__(LAKE_LANES) k_horizon_sky(const LakeMember* __restrict__ tab, HorizonPlanes p, uint32_t mask, double* sky, uint32_t* open, uint32_t* lit) {
  const LakeMember m = tab[blockIdx.y];
  if ((uint64_t)blockIdx.x * LAKE_LANES >= (uint64_t)m.dimx * (uint64_t)m.dimy) return;
  ObsGroup g;
  horizon_sky_group(m, g, blockIdx.x, mask, p.suns, p.nsuns, p.words, p.S, p.K, sky, open, lit);
}

// ---------------- proximity (smx_proximity / smx_ensemble_proximity; bodies: soil_prox.h) ----------------
// On planes of their own; in WATER mode behind the census's labelling and the rank scan. k_prox_mark takes a lane per list entry or,
// in WATER mode, per cell; k_prox_columns a workgroup per column (8 KB of LDS: the column's site mask); k_prox_envelope a lane per
// row and band (PROX_BANDS bands of columns) in workgroups of ONE wavefront, so that the serial pass spreads over as many compute
// units as the map has 64-row stretches times bands;
// k_prox_query's table holds 512 cells' worth of groups (26 KB of LDS), k_prox_hist's 512 cells' worth of (group, bin) keys (4 KB).
constexpr int PROX_ENV_LANES = 64;
struct ProxPlanes {   // what the kernels work on (soil_prox.h): the marks, the rank scan (WATER) and later the depths, the columns' candidates, the envelopes
  uint32_t *M, *BD, *P, *S, *T;
};
__global__ void __launch_bounds__(LAKE_LANES) k_prox_mark(const LakeMember* __restrict__ tab, ProxPlanes p, const uint32_t* __restrict__ list, uint32_t n, ProxAcc* acc,
                                                          uint32_t* nlakes) {
  const LakeMember m = tab[blockIdx.y];
  const uint32_t nb = prox_mark_blocks(m, list != nullptr, n, LAKE_LANES);
  if (blockIdx.x >= nb) return;
  ObsGroup g;
  prox_mark_group(m, g, blockIdx.x, nb, list, n, p.M, p.BD, acc, nlakes + blockIdx.y);
}
__global__ void __launch_bounds__(LAKE_LANES) k_prox_columns(const LakeMember* __restrict__ tab, ProxPlanes p) {
  __shared__ ProxColumn s;
  const LakeMember m = tab[blockIdx.y];
  if (blockIdx.x >= (uint32_t)m.dimx) return;
  ObsGroup g;
  prox_columns_group(m, g, blockIdx.x, s, p.M, p.P);
}
__global__ void __launch_bounds__(PROX_ENV_LANES) k_prox_envelope(const LakeMember* __restrict__ tab, ProxPlanes p, uint32_t bands) {
  const LakeMember m = tab[blockIdx.y];
  if ((uint64_t)blockIdx.x * PROX_ENV_LANES >= (uint64_t)m.dimy * prox_bands(m, bands)) return;
  ObsGroup g;
  prox_envelope_group(m, g, blockIdx.x, bands, p.P, p.S, p.T, p.BD);
}
__global__ void __launch_bounds__(LAKE_LANES) k_prox_query(const LakeMember* __restrict__ tab, ProxPlanes p, uint32_t bands, ProxAcc* acc, uint32_t* nearest, uint32_t* dist2,
                                                           uint32_t* group) {
  __shared__ ProxTable<LAKE_SLOTS> t;
  const LakeMember m = tab[blockIdx.y];
  if ((uint64_t)blockIdx.x * lake_stats_cells(LAKE_SLOTS, LAKE_LANES) >= (uint64_t)m.dimx * (uint64_t)m.dimy) return;
  ObsGroup g;
  prox_query_group<LAKE_SLOTS>(m, g, blockIdx.x, bands, t, p.M, p.P, p.S, p.T, p.BD, acc, nearest, dist2, group);
}
__global__ void __launch_bounds__(LAKE_LANES) k_prox_hist(const LakeMember* __restrict__ tab, const uint32_t* __restrict__ dist2, const uint32_t* __restrict__ group,
                                                          uint32_t* hist, uint32_t nbins, uint32_t bin_width) {
  __shared__ ProxHistTable<LAKE_SLOTS> t;
  const LakeMember m = tab[blockIdx.y];
  if ((uint64_t)blockIdx.x * lake_stats_cells(LAKE_SLOTS, LAKE_LANES) >= (uint64_t)m.dimx * (uint64_t)m.dimy) return;
  ObsGroup g;
  prox_hist_group<LAKE_SLOTS>(m, g, blockIdx.x, t, dist2, group, hist, nbins, bin_width);
}

// ---------------- dispersed flow (smx_dispersal / smx_ensemble_dispersal; bodies: soil_disp.h) ----------------
// Behind the drainage chain with its statistics, on its planes. k_disp_pending holds the height and dry-mark tiles with their halo of
// one and a slot per cell of the tile (18 KB of LDS); k_disp_flow strides over the round's part of the ready list with at most
// DISP_FLOW_BLOCKS workgroups: the list's length is read on the device. k_disp_fold's table holds 512 cells' worth of basins (14 KB).
struct DispPlanes {   // the planes of one call (soil_disp.h)
  uint32_t *T, *R, *P, *RC, *Q;
  uint64_t* AQ;
};
__global__ void __launch_bounds__(LAKE_LANES) k_disp_pending(const LakeMember* __restrict__ tab, DispPlanes p, DispAcc* acc, uint32_t* ring) {
  __shared__ double hs[(LAKE_TX + 2) * (LAKE_TY + 2)];
  __shared__ uint32_t ds[(LAKE_TX + 2) * (LAKE_TY + 2)];
  __shared__ uint32_t sl[LAKE_TX * LAKE_TY];
  __shared__ uint32_t wc[2];
  const LakeMember m = tab[blockIdx.y];
  const uint32_t nt = lake_tiles(m, LAKE_TX, LAKE_TY);
  if (blockIdx.x >= nt) return;
  ObsGroup g;
  disp_pending_group<LAKE_TX, LAKE_TY>(m, g, blockIdx.x, nt, hs, ds, sl, wc, p.P, p.RC, p.Q, p.AQ, acc, ring + DISP_RING * blockIdx.y);
}
__global__ void __launch_bounds__(LAKE_LANES) k_disp_flow(const LakeMember* __restrict__ tab, uint32_t round, uint32_t exponent, DispPlanes p, DispAcc* acc, uint32_t* ring,
                                                          uint32_t* busy, uint32_t bit) {
  const LakeMember m = tab[blockIdx.y];
  ObsGroup g;
  disp_flow_group(m, g, blockIdx.x, gridDim.x, round, exponent, p.T, p.R, p.P, p.RC, p.Q, p.AQ, acc, ring + DISP_RING * blockIdx.y, busy, bit);
}
__global__ void __launch_bounds__(LAKE_LANES) k_disp_fold(const LakeMember* __restrict__ tab, DispPlanes p, DispAcc* acc) {
  __shared__ DispTable<LAKE_SLOTS> t;
  const LakeMember m = tab[blockIdx.y];
  if ((uint64_t)blockIdx.x * lake_stats_cells(LAKE_SLOTS, LAKE_LANES) >= (uint64_t)m.dimx * (uint64_t)m.dimy) return;
  ObsGroup g;
  disp_fold_group<LAKE_SLOTS>(m, g, blockIdx.x, t, p.T, p.R, p.RC, p.AQ, acc);
}
__global__ void __launch_bounds__(LAKE_LANES) k_disp_peak(const LakeMember* __restrict__ tab, DispPlanes p, DispAcc* acc, uint32_t want_donors, uint32_t want_receivers) {
  const LakeMember m = tab[blockIdx.y];
  if ((uint64_t)blockIdx.x * LAKE_LANES >= (uint64_t)m.dimx * (uint64_t)m.dimy) return;
  ObsGroup g;
  disp_peak_group(m, g, blockIdx.x, p.T, p.P, p.RC, p.AQ, acc, want_donors, want_receivers);
}

// ---------------- spill analysis (smx_spill / smx_ensemble_spill; bodies: soil_spill.h) ----------------
// The census's tiles and lanes. k_spill_pass holds the height and rank tiles with their halo of one (18 x 66 doubles and words, 14 KB
// of LDS) and a table with a slot per cell of the tile (12 KB); k_spill_store's table holds 512 cells' worth of basins (14 KB).
// k_spill_relax strides over a member's boundary cells with at most SPILL_RELAX_BLOCKS workgroups: the list's length is read on the device.
constexpr int SPILL_PS = LAKE_TX * LAKE_TY;
constexpr unsigned SPILL_RELAX_BLOCKS = 2048;
struct SpillPlanes {   // the planes of one call (soil_spill.h)
  uint32_t *T, *B, *R, *Q;
  double* H;
};
__global__ void __launch_bounds__(LAKE_LANES) k_spill_init(const LakeMember* __restrict__ tab, SpillAcc* acc) {
  const LakeMember m = tab[blockIdx.y];
  if ((uint64_t)blockIdx.x * LAKE_LANES >= m.cap) return;
  ObsGroup g;
  spill_init_group(m, g, blockIdx.x, acc);
}
template <int PHASE>
__global__ void __launch_bounds__(LAKE_LANES) k_spill_pass(const LakeMember* __restrict__ tab, SpillPlanes p, SpillAcc* acc) {
  __shared__ double hs[(LAKE_TX + 2) * (LAKE_TY + 2)];
  __shared__ uint32_t ls[(LAKE_TX + 2) * (LAKE_TY + 2)];
  __shared__ SpillPassTable<SPILL_PS> t;
  const LakeMember m = tab[blockIdx.y];
  if (blockIdx.x >= lake_tiles(m, LAKE_TX, LAKE_TY)) return;
  ObsGroup g;
  spill_pass_group<LAKE_TX, LAKE_TY, SPILL_PS, PHASE>(m, g, blockIdx.x, hs, ls, t, p.T, p.B, p.R, p.H, acc);
}
__global__ void __launch_bounds__(LAKE_LANES) k_spill_list(const LakeMember* __restrict__ tab, SpillPlanes p) {
  const LakeMember m = tab[blockIdx.y];
  if ((uint64_t)blockIdx.x * LAKE_LANES >= (uint64_t)m.dimx * (uint64_t)m.dimy) return;
  ObsGroup g;
  spill_list_group(m, g, blockIdx.x, p.B, p.R, p.Q);
}
__global__ void __launch_bounds__(LAKE_LANES) k_spill_point(const LakeMember* __restrict__ tab, SpillPlanes p, SpillAcc* acc) {
  const LakeMember m = tab[blockIdx.y];
  if ((uint64_t)blockIdx.x * LAKE_LANES >= m.cap) return;
  ObsGroup g;
  spill_point_group(m, g, blockIdx.x, p.T, acc);
}
__global__ void __launch_bounds__(LAKE_LANES) k_spill_relax(const LakeMember* __restrict__ tab, uint32_t sweep, SpillPlanes p, SpillAcc* acc, uint32_t* changed) {
  const LakeMember m = tab[blockIdx.y];
  ObsGroup g;
  spill_relax_group(m, g, blockIdx.x, gridDim.x, sweep, p.T, p.B, p.R, p.Q, p.H, acc, changed);
}
__global__ void __launch_bounds__(LAKE_LANES) k_spill_store(const LakeMember* __restrict__ tab, SpillPlanes p, SpillAcc* acc, int filled) {
  __shared__ SpillStoreTable<LAKE_SLOTS> t;
  const LakeMember m = tab[blockIdx.y];
  if ((uint64_t)blockIdx.x * lake_stats_cells(LAKE_SLOTS, LAKE_LANES) >= (uint64_t)m.dimx * (uint64_t)m.dimy) return;
  ObsGroup g;
  spill_store_group<LAKE_SLOTS>(m, g, blockIdx.x, t, p.T, p.H, acc, filled != 0);
}

// ---------------- through-drainage (smx_through / smx_ensemble_through; bodies: soil_through.h) ----------------
// The spill chain's kernels run on the call's own planes (the boundary marks in a plane of their own: R stays the receivers); behind
// them, per basin or per boundary cell, the kernels below. k_through_count's table holds 512 cells' worth of basins (4 KB of LDS);
// k_through_hops and k_through_exit stride over the boundary cells as k_spill_relax does.
struct ThroughPlanes {   // the planes of one call (soil_through.h): M the boundary marks
  uint32_t *T, *B, *M, *Q;
  double* H;
};
__global__ void __launch_bounds__(LAKE_LANES) k_through_init(const LakeMember* __restrict__ tab, ThroughAcc* acc) {
  const LakeMember m = tab[blockIdx.y];
  if ((uint64_t)blockIdx.x * LAKE_LANES >= m.cap) return;
  ObsGroup g;
  through_init_group(m, g, blockIdx.x, acc);
}
__global__ void __launch_bounds__(LAKE_LANES) k_through_count(const LakeMember* __restrict__ tab, const uint32_t* __restrict__ T, ThroughAcc* acc) {
  __shared__ ThroughCountTable<LAKE_SLOTS> t;
  const LakeMember m = tab[blockIdx.y];
  if ((uint64_t)blockIdx.x * lake_stats_cells(LAKE_SLOTS, LAKE_LANES) >= (uint64_t)m.dimx * (uint64_t)m.dimy) return;
  ObsGroup g;
  through_count_group<LAKE_SLOTS>(m, g, blockIdx.x, t, T, acc);
}
__global__ void __launch_bounds__(LAKE_LANES) k_through_hops(const LakeMember* __restrict__ tab, ThroughPlanes p, const SpillAcc* sacc, ThroughAcc* acc, uint32_t* changed) {
  const LakeMember m = tab[blockIdx.y];
  ObsGroup g;
  through_hops_group(m, g, blockIdx.x, gridDim.x, p.T, p.B, p.M, p.Q, p.H, sacc, acc, changed);
}
__global__ void __launch_bounds__(LAKE_LANES) k_through_exit(const LakeMember* __restrict__ tab, ThroughPlanes p, const SpillAcc* sacc, ThroughAcc* acc) {
  const LakeMember m = tab[blockIdx.y];
  ObsGroup g;
  through_exit_group(m, g, blockIdx.x, gridDim.x, p.T, p.B, p.M, p.Q, p.H, sacc, acc);
}
template <int PHASE>
__global__ void __launch_bounds__(LAKE_LANES) k_through_link(const LakeMember* __restrict__ tab, ThroughPlanes p, const SpillAcc* sacc, ThroughAcc* acc) {
  const LakeMember m = tab[blockIdx.y];
  if ((uint64_t)blockIdx.x * LAKE_LANES >= m.cap) return;
  ObsGroup g;
  through_link_group<PHASE>(m, g, blockIdx.x, p.T, p.H, sacc, acc);
}
__global__ void __launch_bounds__(LAKE_LANES) k_through_accumulate(const LakeMember* __restrict__ tab, ThroughAcc* acc, uint32_t* AR) {
  const LakeMember m = tab[blockIdx.y];
  if ((uint64_t)blockIdx.x * LAKE_LANES >= m.cap) return;
  ObsGroup g;
  through_accumulate_group(m, g, blockIdx.x, acc, AR);
}
__global__ void __launch_bounds__(LAKE_LANES) k_through_outlet(const LakeMember* __restrict__ tab, const SpillAcc* sacc, ThroughAcc* acc) {
  const LakeMember m = tab[blockIdx.y];
  if ((uint64_t)blockIdx.x * LAKE_LANES >= m.cap) return;
  ObsGroup g;
  through_outlet_group(m, g, blockIdx.x, sacc, acc);
}
__global__ void __launch_bounds__(LAKE_LANES) k_through_plane(const LakeMember* __restrict__ tab, const uint32_t* __restrict__ T, const ThroughAcc* acc, uint32_t* O) {
  const LakeMember m = tab[blockIdx.y];
  if ((uint64_t)blockIdx.x * LAKE_LANES >= (uint64_t)m.dimx * (uint64_t)m.dimy) return;
  ObsGroup g;
  through_plane_group(m, g, blockIdx.x, T, acc, O);
}
__global__ void __launch_bounds__(LAKE_LANES) k_through_area(const LakeMember* __restrict__ tab, const uint32_t* __restrict__ R, uint32_t* P, uint32_t* AR) {
  const LakeMember m = tab[blockIdx.y];
  if ((uint64_t)blockIdx.x * LAKE_LANES >= (uint64_t)m.dimx * (uint64_t)m.dimy) return;
  ObsGroup g;
  through_area_group(m, g, blockIdx.x, R, P, AR);
}

// ---------------- reading the strata (smx_soil_totals / smx_soil_thickness / smx_cores; bodies: soil_strata.h) ----------------
// One lane per column, pointer chasing: a workgroup is ONE wavefront (a deep column holds up nothing else) and strides over the map.
// k_strata_totals: member blockIdx.y of the table, workgroup blockIdx.x of gridDim.x on ITS columns (the grid is sized for the largest).
__global__ void __launch_bounds__(STRATA_LANES) k_strata_totals(const StrataMap* __restrict__ tab, uint32_t ntypes, StrataRec* acc, uint64_t* other, uint64_t* bad) {
  __shared__ StrataTable t;
  const StrataMap m = tab[blockIdx.y];
  if ((uint64_t)blockIdx.x * STRATA_LANES >= m.ncells) return;   // (none of its columns exists)
  ObsGroup g;
  strata_totals_group(m, g, blockIdx.x, gridDim.x, ntypes, t, acc, other, bad);
}
__global__ void __launch_bounds__(STRATA_LANES) k_strata_thickness(StrataMap m, StrataTypes ty, double* __restrict__ thickness, double* __restrict__ cover,
                                                                   uint32_t* __restrict__ sections, uint64_t* bad) {
  ObsGroup g;
  strata_thickness_group(m, g, blockIdx.x, gridDim.x, ty, thickness, cover, sections, bad);
}
__global__ void __launch_bounds__(STRATA_LANES) k_core_count(StrataMap m, const uint32_t* __restrict__ list, uint64_t n, uint32_t* __restrict__ count, uint64_t* bad) {
  ObsGroup g;
  core_count_group(m, g, blockIdx.x, gridDim.x, list, n, count, bad);
}
// the sections the list holds, next to the error word (one lane, behind the scan)
__global__ void k_core_total(const uint32_t* __restrict__ count, const uint64_t* __restrict__ base, uint64_t n, uint64_t* total) {
  *total = base[n - 1] + count[n - 1];
}
__global__ void __launch_bounds__(STRATA_LANES) k_core_scatter(StrataMap m, const uint32_t* __restrict__ list, uint64_t n, const uint32_t* __restrict__ count,
                                                               const uint64_t* __restrict__ base, uint64_t room, uint32_t* __restrict__ type,
                                                               double* __restrict__ size, double* __restrict__ floor, double* __restrict__ sat) {
  ObsGroup g;
  core_scatter_group(m, g, blockIdx.x, gridDim.x, list, n, count, base, room, type, size, floor, sat);
}
struct CoreWidenFn {   // the scan's input: a count as a 64-bit word
  __host__ __device__ uint64_t operator()(uint32_t v) const { return (uint64_t)v; }
};

// ---------------- the sediment budget (smx_budget / smx_ensemble_budget; bodies: soil_budget.h) ----------------
// Behind the drainage chain on the BASE, on its rank plane. k_budget_fold: member blockIdx.y of the table, workgroup blockIdx.x a
// 16 x 16 tile of cells, one lane a cell (a compact tile meets few basins; sixteen consecutive 32-byte records a column); the basin
// table has a slot per cell and the soil table an entry per type (21 KB of LDS). k_budget_where: LAKE_LANES cells a workgroup.
constexpr int BUDGET_TX = 16, BUDGET_TY = 16, BUDGET_SLOTS = BUDGET_TX * BUDGET_TY;
static_assert(BUDGET_SLOTS == LAKE_LANES, "k_budget_fold: one lane a cell");
__global__ void __launch_bounds__(LAKE_LANES) k_budget_fold(BudgetBase b, const BudgetMap* __restrict__ tab, const uint32_t* __restrict__ T, BudgetAcc* acc,
                                                            BudgetSoilRec* soils, uint64_t* bad, BudgetPlanes pl) {
  __shared__ BudgetBasinTable<BUDGET_SLOTS> bt;
  __shared__ BudgetSoilTable st;
  const BudgetMap m = tab[blockIdx.y];
  ObsGroup g;
  budget_fold_group<BUDGET_TX, BUDGET_TY, BUDGET_SLOTS>(b, m, g, blockIdx.x, bt, st, T, acc, soils, bad, pl);
}
__global__ void __launch_bounds__(LAKE_LANES) k_budget_where(BudgetBase b, const BudgetMap* __restrict__ tab, const uint32_t* __restrict__ T, BudgetAcc* acc) {
  const BudgetMap m = tab[blockIdx.y];
  ObsGroup g;
  budget_where_group(b, m, g, blockIdx.x, T, acc);
}

// ---------------- speculative engine kernels (protocol: soil_spec.h) ----------------
// Particles per wave (env SMX_SPEC_LANES, default 1): a phase has only ~10^3 particles while the chip has 1024
// SIMDs, and one particle step is issue-bound (a few thousand dependent instructions), so one particle per wave
// is fastest (measured at 1024^2: 1 lane 349 ms, 8 lanes 429 ms, 32 lanes 537 ms per water phase).
static int spec_lanes() {
  static const int v = (int)std::min(64ll, std::max(1ll, env_int("SMX_SPEC_LANES")));
  return v;
}

__global__ void __launch_bounds__(256) k_spec_begin(DevState s, SpecShared sh, uint32_t n) {
  spec_begin_team(s, sh, n, threadIdx.x, blockDim.x);
}
template <bool WIND>
__global__ void __launch_bounds__(64) k_spec_scout(DevState s, SpecShared sh, uint32_t lanes) {
  SMX_LOAD_SOILS(soils_sh)
  const uint32_t n = sh.ctrl[SC_N] ? sh.ctrl[SC_N] + SPEC_SCOUT_MARGIN : 0u;
  const uint32_t pid = blockIdx.x * lanes + threadIdx.x;
  if (threadIdx.x >= lanes || pid >= n) return;
  spec_scout_one<WIND>(s, soils_sh, sh, pid);
}
template <bool WIND>
__global__ void __launch_bounds__(64) k_spec_scout_coop(DevState s, SpecShared sh) {
  SMX_LOAD_SOILS(soils_sh)
  if (sh.ctrl[SC_N] == 0 || blockIdx.x >= sh.ctrl[SC_N] + SPEC_SCOUT_MARGIN) return;
  spec_scout_one_coop<WIND>(s, soils_sh, sh, blockIdx.x);
}
// one wave per pending particle walks its predicted footprint: publish claims, then (next kernel) test them
__global__ void __launch_bounds__(64) k_spec_claim(SpecShared sh) {
  if (blockIdx.x >= sh.ctrl[SC_NPENDING]) return;
  spec_claim_one(sh, sh.pending[blockIdx.x], threadIdx.x, 64u);
}
__global__ void __launch_bounds__(64) k_spec_select(SpecShared sh) {
  if (blockIdx.x >= sh.ctrl[SC_NPENDING]) return;
  const uint32_t pid = sh.pending[blockIdx.x];
  const bool b = spec_blocked(sh, pid, threadIdx.x, 64u);
  const bool any = __any(b);
  if (threadIdx.x == 0) sh.part[pid].blocked = any ? 1u : 0u;
}
template <bool WIND>
__global__ void __launch_bounds__(64) k_spec_exec(DevState s, SpecShared sh, uint32_t lanes) {
  SMX_LOAD_SOILS(soils_sh)
  const uint32_t i = blockIdx.x * lanes + threadIdx.x;
  if (threadIdx.x >= lanes || i >= sh.ctrl[SC_NPENDING]) return;
  spec_exec_one<WIND>(s, soils_sh, sh, sh.pending[i]);
}
// one particle per WAVE: lanes 0..8 share the block fetch / acquisition of every step (soil_coop.h)
template <bool WIND>
__global__ void __launch_bounds__(64) k_spec_exec_coop(DevState s, SpecShared sh) {
  SMX_LOAD_SOILS(soils_sh)
  if (blockIdx.x >= sh.ctrl[SC_NPENDING]) return;
  spec_exec_one_coop<WIND>(s, soils_sh, sh, sh.pending[blockIdx.x]);
}
__global__ void __launch_bounds__(1024) k_spec_boundary(DevState s, SpecShared sh) {   // ONE workgroup: the round barrier
  __shared__ SpecWork w;
  spec_boundary_team(s, sh, w, threadIdx.x, blockDim.x, []() { __syncthreads(); });
}
__global__ void __launch_bounds__(64) k_spec_abandon(DevState s, SpecShared sh) {
  if (threadIdx.x == 0) spec_abandon(s, sh);
}
__global__ void __launch_bounds__(256) k_spec_end(DevState s, SpecShared sh, uint32_t whole_phase) {
  const uint32_t done = whole_phase ? sh.ctrl[SC_N] : sh.ctrl[SC_TOP];   // top-level particles executed
  spec_end_team(s, sh, done, sh.ctrl[SC_NESTED_COMMITTED], threadIdx.x, blockDim.x);
}


// ---------------- batched engine kernels (protocol: soil_batch.h) ----------------
// One particle per LANE. 64-thread workgroups: a phase has 10^3..10^6 particles and the chip has 1024 SIMDs, so
// single-wave workgroups spread the waves evenly over CUs and XCDs (workgroups go round-robin over the XCDs).
template <bool WIND>
__global__ void __launch_bounds__(64) k_batch_spawn(DevState s, BatchShared bs, uint32_t nslots, const BChild* kids, const uint32_t* contains) {
  SMX_LOAD_SOILS(sh)
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= nslots) return;
  BatchPolicy pol(s, bs);
  Sim<BatchPolicy> sim(s, sh, pol);
  if constexpr (WIND) batch_wind_spawn(sim, bs, i); else batch_water_spawn(sim, bs, i, kids ? kids + i : nullptr, kids ? contains : nullptr);
  sim.flush_counters(); pol.finish(s);
  // relaxed schedule: a record whose flood is what did not fit its parent's region waits on the flood list of epoch 0
  if constexpr (!WIND) { if (bs.relaxed && kids) relax_flood_later(bs, i, 0u, bs.water[i].state == B_ENDED); }
}
template <bool WIND>
__global__ void __launch_bounds__(64) k_batch_reclaim(DevState s, BatchShared bs, uint32_t nlive, uint32_t epoch) {
  SMX_LOAD_SOILS(sh)
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= nlive) return;
  BatchPolicy pol(s, bs);
  Sim<BatchPolicy> sim(s, sh, pol);
  if constexpr (WIND) batch_wind_reclaim(sim, bs, bs.live[i], epoch); else batch_water_reclaim(sim, bs, bs.live[i], epoch);
}
template <bool WIND>
__global__ void __launch_bounds__(64) k_batch_epoch(DevState s, BatchShared bs, uint32_t nlive, uint32_t epoch, uint32_t lpw) {
  SMX_LOAD_SOILS(sh)
  // `lpw` particles per wavefront (batch_lanes_per_wave): a wavefront costs the UNION of its lanes' paths, and the chip has
  // 1024 SIMDs -- a phase that is down to a few thousand particles runs them one per wavefront instead of 64.
  const uint32_t i = blockIdx.x * lpw + threadIdx.x;
  if (threadIdx.x >= lpw || i >= nlive) return;
  BatchPolicy pol(s, bs);
  Sim<BatchPolicy> sim(s, sh, pol);
  if constexpr (WIND) batch_wind_epoch(sim, bs, bs.live[i], epoch);
  else { Frame st[MAX_FRAMES]; batch_water_epoch(sim, bs, bs.live[i], epoch, st); }
  sim.flush_counters(); pol.finish(s);
}
// the same kernel held to 256 registers (a few spilled) = two wavefronts per SIMD: for phases with more wavefronts than SIMDs
template <bool WIND>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) k_batch_epoch2(DevState s, BatchShared bs, uint32_t nlive, uint32_t epoch, uint32_t lpw) {
  SMX_LOAD_SOILS(sh)
  // `lpw` particles per wavefront (batch_lanes_per_wave): a wavefront costs the UNION of its lanes' paths, and the chip has
  // 1024 SIMDs -- a phase that is down to a few thousand particles runs them one per wavefront instead of 64.
  const uint32_t i = blockIdx.x * lpw + threadIdx.x;
  if (threadIdx.x >= lpw || i >= nlive) return;
  BatchPolicy pol(s, bs);
  Sim<BatchPolicy> sim(s, sh, pol);
  if constexpr (WIND) batch_wind_epoch(sim, bs, bs.live[i], epoch);
  else { Frame st[MAX_FRAMES]; batch_water_epoch(sim, bs, bs.live[i], epoch, st); }
  sim.flush_counters(); pol.finish(s);
}
// ---------------- relaxed schedule (soil_relax.h): step -> apply -> nine cascade colours (-> floods), per epoch ----------------
template <bool WIND>
__global__ void __launch_bounds__(64) k_relax_step(DevState s, BatchShared bs, uint32_t nlive, uint32_t epoch, uint32_t lpw) {
  SMX_LOAD_SOILS(sh)
  const uint32_t i = blockIdx.x * lpw + threadIdx.x;
  if (threadIdx.x >= lpw || i >= nlive) return;
  BatchPolicy pol(s, bs);
  Sim<BatchPolicy> sim(s, sh, pol);
  if constexpr (WIND) relax_wind_step(sim, bs, bs.live[i], epoch); else relax_water_step(sim, bs, bs.live[i], epoch);
}
__global__ void __launch_bounds__(64) k_relax_apply(DevState s, BatchShared bs, uint32_t nlive, uint32_t epoch) {
  SMX_LOAD_SOILS(sh)
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i == 0u) {                                             // the lists of the NEXT epoch start empty (their last readers finished an epoch ago)
    relax_reset_lists(bs, (epoch + 1u) & 1u);
    bs.ctrl[BC_CASC_CURSOR] = 0u;                            // (this epoch's cascade dataflow starts at its first listed cell)
  }
  if (i >= nlive) return;
  BatchPolicy pol(s, bs);
  Sim<BatchPolicy> sim(s, sh, pol);
  relax_apply_slot(sim, bs, bs.live[i]);
  sim.flush_counters(); pol.finish(s);
}
// wave-reduced commit of the cascade counters of the relaxed kernels (one atomic per wavefront)
__device__ __forceinline__ void relax_commit_cascade_counters(const DevState& s, unsigned long long nc, unsigned long long nt) {
  for (int off = 32; off > 0; off >>= 1) { nc += (unsigned long long)__shfl_down((long long)nc, off); nt += (unsigned long long)__shfl_down((long long)nt, off); }
  if ((threadIdx.x & 63u) == 0) { if (nc) atomicAdd(&s.ctr[C_CASCADE_CALLS], nc); if (nt) atomicAdd(&s.ctr[C_CASCADE_TRANSFERS], nt); }
}
// steps of the nested particles that ran inside this launch's floods (C_FLOOD_NESTED_STEPS: what bench.py prices a flood launch with)
__device__ __forceinline__ void relax_commit_flood_steps(const DevState& s, unsigned long long n) {
  for (int off = 32; off > 0; off >>= 1) n += (unsigned long long)__shfl_down((long long)n, off);
  if ((threadIdx.x & 63u) == 0 && n) atomicAdd(&s.ctr[C_FLOOD_NESTED_STEPS], n);
}
// `lpw` flagged cells per wavefront (relax_settle_lanes): an isolated cell cascades right in its lane, a branchy path of ~13 us, and a wavefront
// costs the UNION of its lanes' paths -- the launch lasted as long as its slowest wavefront of 64 cells, not as long as its work (round 14).
__global__ void __launch_bounds__(64) k_relax_filter(DevState s, BatchShared bs, uint32_t epoch, uint32_t lpw) {
  const uint32_t par = epoch & 1u;
  uint32_t n = bs.ctrl[BC_NFLAG + par];
  if (n > bs.flag_cap) n = bs.flag_cap;
  if (blockIdx.x * lpw >= n) return;                         // (the launch is sized for the worst case: most blocks leave here)
  SMX_LOAD_SOILS(sh)
  const uint32_t i = blockIdx.x * lpw + threadIdx.x;
  const bool valid = threadIdx.x < lpw && i < n;
  BatchPolicy pol(s, bs);
  Sim<BatchPolicy> sim(s, sh, pol);
  relax_filter<BatchPolicy, true>(sim, bs, valid ? bs.flagl[par][i] : 0u, valid, epoch);   // (isolated cells cascade in here)
  sim.flush_counters(); pol.finish(s);
  relax_commit_cascade_counters(s, pol.a_casc, pol.a_tr);
}
// (a fixed, small grid with a grid-stride loop: the colour lists hold the residue of crowded cells -- a few hundred entries, often none --
//  and a launch sized for the worst case spends its ~13 us dispatching a thousand workgroups that read the count and leave; round 5)
__global__ void __launch_bounds__(64) k_relax_cascade(DevState s, BatchShared bs, uint32_t epoch, uint32_t colour) {
  const uint32_t par = epoch & 1u;
  uint32_t n = bs.ctrl[BC_NCASC + 9u * par + colour];
  if (n > bs.clist_cap) n = bs.clist_cap;
  if (blockIdx.x * 64u >= n) return;
  SMX_LOAD_SOILS(sh)
  unsigned long long nc = 0, nt = 0;
  for (uint32_t i = blockIdx.x * 64u + threadIdx.x; i < n; i += gridDim.x * 64u) {
    BatchPolicy pol(s, bs);
    Sim<BatchPolicy> sim(s, sh, pol);
    relax_cascade(sim, bs.clist[par][(size_t)colour * bs.clist_cap + i]);
    sim.flush_counters(); pol.finish(s);
    nc += pol.a_casc; nt += pol.a_tr;
  }
  relax_commit_cascade_counters(s, nc, nt);
}
// The nine colour lists of an epoch as ONE launch (round 5): a DATAFLOW over the listed cells in colour order -- a wavefront takes the
// next cell, waits until every listed cell of an earlier colour within two cells of it (3x3 blocks that overlap its own) is done, runs
// Particle::cascade there (lane 0) and publishes it (bs.cstate). Same order between conflicting cells as nine launches with a barrier
// each, so the same result -- without eight kernel boundaries of ~8 us in an epoch that lasts ~230 (2 300 epochs per tick: 19.8 % of it).
// Spin budget of the two dataflow kernels of the default schedule: a wavefront that polls a dependency longer than `budget` polls -- tens of seconds; the
// dynamic cursor guarantees that every dependency belongs to a wavefront that is already running, so only a fault gets there -- raises bs.ctrl[BC_STALLED], every other
// waiter sees the flag within 1 024 polls and stops waiting too, the kernel drains, and the host fails the call (-9) instead of hanging the stream.
// SMX_SPIN_BUDGET overrides the number of polls (tests/test_gpu_relaxed.py sets 1 to see the error).
static uint32_t spin_budget(uint32_t dflt) { static const long long v = env_int("SMX_SPIN_BUDGET"); return v >= 0 ? (uint32_t)v : dflt; }
__device__ __forceinline__ bool spin_wait_while(const uint32_t* f, uint32_t busy, uint32_t* stalled, uint32_t budget, uint32_t sleep_a, uint32_t naps) {
  uint32_t spins = 0;
  while (__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == busy) {
    if (sleep_a == 2u) __builtin_amdgcn_s_sleep(2); else __builtin_amdgcn_s_sleep(8);
    for (uint32_t r = 0; r < naps; r++) __builtin_amdgcn_s_sleep(127);
    if (++spins > budget) { __hip_atomic_store(stalled, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); return false; }
    if ((spins & 1023u) == 0u && __hip_atomic_load(stalled, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return false;
  }
  return true;
}
// Publish a cell's state to the wavefronts that poll it, on any XCD: write back what this wavefront stored, WAIT for it, then the flag (agent scope, sc1).
// Spelled out instead of a release store: where the compiler can prove the vector-memory counter empty on some path into the release, it drops the
// s_waitcnt vmcnt(0) behind buffer_wbl2 and the flag overtakes the cascade's stores (seen in k_relax_settle's code: the headline's digest moved, the
// 64 x 64 tests did not notice). The inline wait is invisible to that pass.
__device__ __forceinline__ void relax_publish(uint32_t* f, uint32_t v) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __hip_atomic_store(f, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// The dependencies of ONE cell `c` of colour `q`, polled by the whole wavefront (c and q are wavefront-uniform; every lane calls): lane k < 25 watches
// the k-th cell of the 5 x 5 square around c -- up to 24 independent words, where lane 0 used to poll them one round trip after the other.
//   SETTLE = false (k_relax_cascade_flow): wait while a cell of an EARLIER colour is listed and not done (cstate == 2T);
//   SETTLE = true  (k_relax_settle): every FLAGGED cell there must be classified (cstate >= 2T), those of an earlier colour done (2T + 1).
// Budget and stall flag as spin_wait_while: false = stalled (the caller stops waiting and lets the kernel drain; the host fails the call, -9).
template <bool SETTLE>
__device__ __forceinline__ bool relax_wait_block(const DevState& s, const BatchShared& bs, uint32_t c, uint32_t q, uint32_t budget) {
  const uint32_t lane = threadIdx.x & 63u, t2 = 2u * bs.rtag;
  const int x = (int)(c / (uint32_t)s.dimy), y = (int)(c - (uint32_t)x * (uint32_t)s.dimy);
  const int xx = x + (int)(lane / 5u) - 2, yy = y + (int)(lane % 5u) - 2;
  const bool inr = lane < 25u && lane != 12u && xx >= s.x_lo && xx < s.x_hi && yy >= 0 && yy < s.dimy;
  const size_t ci = inr ? (size_t)xx * (size_t)s.dimy + (size_t)yy : (size_t)c;     // (a lane with nothing to watch never loads)
  const bool earlier = inr && (uint32_t)((xx % 3) * 3 + (yy % 3)) < q;
  const bool watch = SETTLE ? (inr && bs.cflag[ci] == bs.rtag) : earlier;
  uint32_t* stalled = &bs.ctrl[BC_STALLED];
  uint32_t spins = 0;
  while (true) {
    bool ok = true;
    if (watch) {
      const uint32_t st = __hip_atomic_load(&bs.cstate[ci], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      ok = SETTLE ? (st >= t2 && (!earlier || st == t2 + 1u)) : st != t2;
    }
    if (__ballot(!ok) == 0ull) return true;
    __builtin_amdgcn_s_sleep(2);
    if (++spins > budget) { if (lane == 0u) __hip_atomic_store(stalled, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); return false; }
    if ((spins & 1023u) == 0u && __hip_atomic_load(stalled, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return false;   // (one word: uniform)
  }
}
__global__ void __launch_bounds__(64) k_relax_cascade_flow(DevState s, BatchShared bs, uint32_t epoch, uint32_t budget) {
  const uint32_t par = epoch & 1u;
  uint32_t cnt[9], total = 0;
#pragma unroll
  for (uint32_t q = 0; q < 9u; q++) { uint32_t n = bs.ctrl[BC_NCASC + 9u * par + q]; if (n > bs.clist_cap) n = bs.clist_cap; cnt[q] = n; total += n; }
  if (total == 0u) return;
  SMX_LOAD_SOILS(sh)
  __shared__ uint32_t s_i, s_c, s_q;
  unsigned long long nc = 0, nt = 0;
  const uint32_t pending = 2u * bs.rtag;
  bool live = true;
  while (true) {
    if (threadIdx.x == 0) {
      uint32_t i = atomicAdd(&bs.ctrl[BC_CASC_CURSOR], 1u), q = 0;
      s_i = i;
      if (i < total) {
#pragma unroll
        for (uint32_t k = 0; k < 9u; k++) { if (q == k && i >= cnt[k]) { i -= cnt[k]; q = k + 1u; } }
        s_c = bs.clist[par][(size_t)q * bs.clist_cap + i]; s_q = q;
      }
    }
    __syncthreads();
    const uint32_t i = s_i, c = s_c, q = s_q;
    __syncthreads();
    if (i >= total) break;
    if (live && !relax_wait_block<false>(s, bs, c, q, budget)) live = false;   // (stalled: the call fails; stop waiting, let the kernel drain)
    if (threadIdx.x == 0) {
      __atomic_thread_fence(__ATOMIC_ACQUIRE);
      BatchPolicy pol(s, bs);
      Sim<BatchPolicy> sim(s, sh, pol);
      relax_cascade(sim, c);
      sim.flush_counters(); pol.finish(s);
      nc += pol.a_casc; nt += pol.a_tr;
      relax_publish(&bs.cstate[c], pending + 1u);
    }
  }
  if (threadIdx.x == 0) { if (nc) atomicAdd(&s.ctr[C_CASCADE_CALLS], nc); if (nt) atomicAdd(&s.ctr[C_CASCADE_TRANSFERS], nt); }
}
// ONE launch after apply (round 14): what k_relax_filter and k_relax_cascade_flow do in two, without colour lists, cursor or tickets. A flagged cell
// (cflag == T, T = bs.rtag) goes through three states in bs.cstate: unclassified (anything below 2T), classified and waiting (2T), done (2T + 1).
//   classify  one flagged cell per lane, one pass per wavefront, exactly as relax_filter: load the 3x3 block, cascade_precheck (a cell that needs nothing
//             counts its call and is done), the isolation test (relax_crowded); publish 2T + 1 or 2T (relax_publish). Nothing here waits.
//   isolated  cells cascade in their own lane, as in the filter, and publish 2T + 1.
//   crowded   cells are served by their wavefront one at a time, in ascending colour: the lanes poll the up to 24 cells around it (relax_wait_block) until
//             every flagged one is classified and every one of an earlier colour is done; acquire fence; the owning lane runs relax_cascade and
//             publishes 2T + 1 (relax_publish).
// Why the first wait: relax_filter takes its `need` decision on the map after apply and BEFORE any crowded cascade (a cell that needs nothing then is never
// cascaded, whatever a neighbour's cascade does to its block later), and two cells' 3x3 blocks overlap exactly when the cells are within two of each other:
// a crowded cell must not write before all such neighbours have read. With both waits the order between conflicting cells is that of nine colour passes
// with a barrier each -- what the restatement and the host-thread build define.
// Forward progress (as for spin_wait_while: only a fault reaches the budget). The host launches at most as many wavefronts as are resident together
// (relax_settle_plan), so every wavefront of the launch runs. Classification precedes every wait in every wavefront, hence every flagged cell gets
// classified. Each wavefront holds at most one cell per lane and serves its crowded cells in ascending colour, one at a time; take the unfinished
// crowded cells of the lowest colour q: all they wait for -- classified neighbours, done neighbours of colours < q -- has happened, and in a wavefront that
// holds one of them the current cell has colour q too (nothing below q is unfinished), so it proceeds. By induction over the cells everything finishes.
// Every wait honours the spin budget and BC_STALLED.
// (The body of a settle block behind its early exit, for blocks [0, S) of k_relax_settle_floods: the text of k_relax_settle's own body below, which stays
//  spelled out there -- calling this function from it changes that kernel's register allocation and with it its machine code. Keep the two equal.)
__device__ __forceinline__ void relax_settle_block(const DevState& s, const BatchShared& bs, const SoilP* sh, uint32_t par, uint32_t n, uint32_t lpw, uint32_t budget, unsigned long long* ncrowded) {
  const uint32_t lane = threadIdx.x, i = blockIdx.x * lpw + lane, t2 = 2u * bs.rtag;
  const bool valid = lane < lpw && i < n;
  const uint32_t c = valid ? bs.flagl[par][i] : 0u;
  BatchPolicy pol(s, bs);
  Sim<BatchPolicy> sim(s, sh, pol);
  uint32_t kind = 0u, col = 0u;                              // 0: nothing to do, 1: isolated, 2: crowded
  if (valid) {                                               // ---- classify
    const int x = (int)(c / (uint32_t)s.dimy), y = (int)(c - (uint32_t)x * (uint32_t)s.dimy);
    Blk b;
    sim.template load_block<2>(x, y, b);
    if (!sim.cascade_precheck(b)) sim.n_casc++;              // (a listed cell counts in cascade_blk)
    else kind = relax_crowded(s, bs, x, y) ? 2u : 1u;
    col = (uint32_t)((x % 3) * 3 + (y % 3));
    relax_publish(&bs.cstate[c], kind ? t2 : t2 + 1u);       // (after the loads of the block: a crowded neighbour may write from here on)
  }
  const unsigned long long crowd = __ballot(kind == 2u);
  if (lane == 0u && crowd) atomicAdd(ncrowded, (unsigned long long)__popcll(crowd));
  bool live = true;
  for (int q = -1; q < 9; q++) {                             // ---- pass -1: the isolated cells, all lanes at once; passes 0..8: the crowded cells of that colour, one at a time
    unsigned long long m = __ballot(q < 0 ? kind == 1u : (kind == 2u && col == (uint32_t)q));
    while (m) {
      bool mine;
      if (q < 0) { mine = kind == 1u; m = 0ull; }
      else {
        const int owner = __ffsll((long long)m) - 1;
        m &= m - 1ull;
        const uint32_t cc = (uint32_t)__shfl((int)c, owner);
        if (live && !relax_wait_block<true>(s, bs, cc, (uint32_t)q, budget)) live = false;   // (stalled: the call fails; stop waiting, let the kernel drain)
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        mine = (int)lane == owner;
      }
      if (mine) {                                            // (one site for both kinds: the cascade's code once in the kernel)
        relax_cascade(sim, c);
        relax_publish(&bs.cstate[c], t2 + 1u);
      }
    }
  }
  sim.flush_counters(); pol.finish(s);
  relax_commit_cascade_counters(s, pol.a_casc, pol.a_tr);
}
__global__ void __launch_bounds__(64) k_relax_settle(DevState s, BatchShared bs, uint32_t epoch, uint32_t lpw, uint32_t budget, unsigned long long* ncrowded) {
  const uint32_t par = epoch & 1u;
  uint32_t n = bs.ctrl[BC_NFLAG + par];
  if (n > bs.flag_cap) n = bs.flag_cap;
  if (blockIdx.x * lpw >= n) return;                         // (the launch is sized for the worst case: most blocks leave here)
  SMX_LOAD_SOILS(sh)
  const uint32_t lane = threadIdx.x, i = blockIdx.x * lpw + lane, t2 = 2u * bs.rtag;
  const bool valid = lane < lpw && i < n;
  const uint32_t c = valid ? bs.flagl[par][i] : 0u;
  BatchPolicy pol(s, bs);
  Sim<BatchPolicy> sim(s, sh, pol);
  uint32_t kind = 0u, col = 0u;                              // 0: nothing to do, 1: isolated, 2: crowded
  if (valid) {                                               // ---- classify
    const int x = (int)(c / (uint32_t)s.dimy), y = (int)(c - (uint32_t)x * (uint32_t)s.dimy);
    Blk b;
    sim.template load_block<2>(x, y, b);
    if (!sim.cascade_precheck(b)) sim.n_casc++;              // (a listed cell counts in cascade_blk)
    else kind = relax_crowded(s, bs, x, y) ? 2u : 1u;
    col = (uint32_t)((x % 3) * 3 + (y % 3));
    relax_publish(&bs.cstate[c], kind ? t2 : t2 + 1u);       // (after the loads of the block: a crowded neighbour may write from here on)
  }
  const unsigned long long crowd = __ballot(kind == 2u);
  if (lane == 0u && crowd) atomicAdd(ncrowded, (unsigned long long)__popcll(crowd));
  bool live = true;
  for (int q = -1; q < 9; q++) {                             // ---- pass -1: the isolated cells, all lanes at once; passes 0..8: the crowded cells of that colour, one at a time
    unsigned long long m = __ballot(q < 0 ? kind == 1u : (kind == 2u && col == (uint32_t)q));
    while (m) {
      bool mine;
      if (q < 0) { mine = kind == 1u; m = 0ull; }
      else {
        const int owner = __ffsll((long long)m) - 1;
        m &= m - 1ull;
        const uint32_t cc = (uint32_t)__shfl((int)c, owner);
        if (live && !relax_wait_block<true>(s, bs, cc, (uint32_t)q, budget)) live = false;   // (stalled: the call fails; stop waiting, let the kernel drain)
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        mine = (int)lane == owner;
      }
      if (mine) {                                            // (one site for both kinds: the cascade's code once in the kernel)
        relax_cascade(sim, c);
        relax_publish(&bs.cstate[c], t2 + 1u);
      }
    }
  }
  sim.flush_counters(); pol.finish(s);
  relax_commit_cascade_counters(s, pol.a_casc, pol.a_tr);
}
// the floods of the relaxed schedule: batch_water_epoch over this epoch's list of ended particles; who is not done joins the next
// list. The launch has a fixed number of wavefronts; the floods are spread over them as thinly as the list allows (a wavefront costs
// the union of its lanes' paths, and a flood is a long, branchy path).
// (Round 6, measured and dropped -- profiles/r06_floods.md: the 63 idle lanes fetching a flood's whole rectangle -- cells, flag bytes,
//  frequency / track words, one load per 128-byte line -- before lane 0 starts, and the same for a grid tile's 24 x 24-cell region: no
//  change within 0.5 % although the kernel spends 80 % of its wave cycles waiting (rocprofv3 --pmc): the chain's ~100 dependent accesses
//  are L2 / Infinity-Cache hits already, 0.3-0.5 us each; what a flood costs is their NUMBER. 256 ... 16 384 wavefronts for the list: no
//  change either -- a launch lasts as long as its longest flood.)
// (experiments, SMX_FLOOD_PROF=1: how long does ONE flood take, and how many steps of nested particles run inside it? [0..31] floods by log2 of
//  their duration in 100 MHz ticks, [32..63] the nested steps of those floods, [64] floods that acted, [65] their ticks, [66] listed floods that
//  did not hold their tiles; printed by smx_destroy)
__device__ unsigned long long g_flood_prof[72];
__global__ void __launch_bounds__(64) k_relax_floods(DevState s, BatchShared bs, uint32_t epoch, uint32_t prof) {
  const uint32_t par = epoch & 1u;
  uint32_t n = bs.ctrl[BC_NFLOOD + par];
  if (n > bs.list_cap) n = bs.list_cap;
  uint32_t lpw = (n + gridDim.x - 1u) / gridDim.x;
  if (lpw > 64u) lpw = 64u;
  if (blockIdx.x * lpw >= n) return;
  SMX_LOAD_SOILS(sh)
  // (n > 64 * gridDim.x cannot happen: the host sizes the launch for the generation's slots)
  const uint32_t i = blockIdx.x * lpw + threadIdx.x;
  const bool act = threadIdx.x < lpw && i < n;
  bool again = false; uint32_t slot = 0u;
  if (!relax_floods_due(bs, epoch, n, bs.ctrl[BC_NRUN + par])) {  // not this epoch: the whole list moves on
    if (act) slot = bs.flist[par][i];
    relax_flood_later(bs, slot, par ^ 1u, act);
    return;
  }
  unsigned long long nst = 0;
  if (act) slot = bs.flist[par][i];
  if (act) {
    BatchPolicy pol(s, bs);
    Sim<BatchPolicy> sim(s, sh, pol);
    Frame st[MAX_FRAMES];
    const unsigned long long t0 = prof ? wall_clock64() : 0ull;
    batch_water_epoch(sim, bs, slot, epoch, st);
    sim.flush_counters(); nst = pol.a_nsteps; pol.finish(s);
    again = bs.water[slot].state == B_ENDED;
    if (prof) {
      const unsigned long long dt = wall_clock64() - t0;
      if (again) atomicAdd(&g_flood_prof[66], 1ull);
      else { const int b = 63 - __clzll((long long)(dt | 1ull)); atomicAdd(&g_flood_prof[b > 31 ? 31 : b], 1ull); atomicAdd(&g_flood_prof[32 + (b > 31 ? 31 : b)], nst); atomicAdd(&g_flood_prof[64], 1ull); atomicAdd(&g_flood_prof[65], dt); }
    }
  }
  relax_flood_later(bs, slot, par ^ 1u, again);
  relax_commit_flood_steps(s, nst);
}
// The gate of ONE flood in k_relax_settle_floods, run by the whole wavefront (the rectangle is wavefront-uniform; every lane calls): the flood holds the
// tiles `r` and will write map cells inside them. The lanes scan bs.cflag over the tiles' cells widened by one cell (clamped to the held columns and the
// map, as relax_wait_block clamps), 256 cells per round with the four flag loads of a lane in flight together -- a flood of spill 3 holds at most 3 x 3
// tiles of 4 x 4 cells: 14 x 14 = 196 words, one round -- and the lanes that found a cell flagged in this epoch poll its bs.cstate until it reads done
// (2T + 1). Budget and stall flag as relax_wait_block: false = stalled. `any`: was a flagged cell found at all (a function of the input, not of timing).
__device__ __forceinline__ bool relax_flood_gate(const DevState& s, const BatchShared& bs, const BRect& r, uint32_t budget, bool& any) {
  const uint32_t lane = threadIdx.x & 63u, done = 2u * bs.rtag + 1u;
  int cx0 = (r.tx0 << bs.tshift) - 1, cx1 = (r.tx1 + 1) << bs.tshift, cy0 = (r.ty0 << bs.tshift) - 1, cy1 = (r.ty1 + 1) << bs.tshift;
  if (cx0 < s.x_lo) cx0 = s.x_lo;
  if (cx1 > s.x_hi - 1) cx1 = s.x_hi - 1;
  if (cy0 < 0) cy0 = 0;
  if (cy1 > s.dimy - 1) cy1 = s.dimy - 1;
  any = false;
  if (cx1 < cx0 || cy1 < cy0) return true;
  const uint32_t h = (uint32_t)(cy1 - cy0 + 1), total = (uint32_t)(cx1 - cx0 + 1) * h;
  uint32_t* stalled = &bs.ctrl[BC_STALLED];
  uint32_t spins = 0;
  for (uint32_t k0 = 0; k0 < total; k0 += 256u) {
    size_t ci[4]; uint32_t f[4];
#pragma unroll
    for (uint32_t j = 0; j < 4u; j++) {                        // (consecutive lanes along y: consecutive words)
      const uint32_t k = k0 + 64u * j + lane, kc = k < total ? k : 0u;
      ci[j] = (size_t)(cx0 + (int)(kc / h)) * (size_t)s.dimy + (size_t)(cy0 + (int)(kc % h));
      f[j] = bs.cflag[ci[j]];
      if (k >= total) f[j] = bs.rtag - 1u;                     // (nothing to watch)
    }
    uint32_t watch = 0u;
#pragma unroll
    for (uint32_t j = 0; j < 4u; j++) if (f[j] == bs.rtag) watch |= 1u << j;
    if (__ballot(watch != 0u) == 0ull) continue;
    any = true;
    while (true) {
#pragma unroll
      for (uint32_t j = 0; j < 4u; j++)
        if ((watch >> j) & 1u) { if (__hip_atomic_load(&bs.cstate[ci[j]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == done) watch &= ~(1u << j); }
      if (__ballot(watch != 0u) == 0ull) break;
      __builtin_amdgcn_s_sleep(2);
      if (++spins > budget) { if (lane == 0u) __hip_atomic_store(stalled, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); return false; }
      if ((spins & 1023u) == 0u && __hip_atomic_load(stalled, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return false;   // (one word: uniform)
    }
  }
  return true;
}
// Settle and floods of a dense water epoch as ONE launch (round 15; smx_set_relax_settle mode 2). After k_relax_settle the floods of the epoch waited for the
// whole settle launch to drain -- the longest chain of crowded cells anywhere on the map, plus a kernel boundary -- where a flood needs only the few flagged
// cells next to its own tiles settled. Here the floods join the dataflow over bs.cstate:
//   blocks [0, S)      are the blocks of k_relax_settle (relax_settle_block): classification, isolated pass, crowded passes, waits, publishes;
//   blocks [S, S + F)  take the epoch's flood list as k_relax_floods does, with the same due test; a list that is not due moves on (relax_flood_later).
//                      A listed flood that will not act (it does not hold its tiles, or what it needs next lies outside them) re-claims for the next
//                      epoch as today: it touches no map cell and waits for nothing. A flood that WILL act passes relax_flood_gate first; a wavefront
//                      with several of them gates them one after the other, then an agent-scope acquire fence, then batch_water_epoch for all its lanes.
// Why the state after the launch is the one the two launches leave:
//   * a flood reads and writes no map cell outside the claim tiles it holds (batch_water_epoch: pol.region = held; run_nested and flood_fits suspend
//     whatever would leave them), a settle cascade touches the 3x3 block of its flagged cell and nothing else (Particle::cascade(.., 0)): a cell's block
//     overlaps the flood's tiles exactly when the cell lies within one cell of the tiles' rectangle -- what the gate scans;
//   * every flag of the epoch is set before the launch starts (k_relax_step), and the claim plane and the slot's record that decide whether a flood acts are
//     written by nobody in this launch but the flood's own lane (floods claim in the NEXT epoch's plane);
//   * every flagged cell ends at 2T + 1 -- at classification if it needs nothing, otherwise after its cascade (relax_publish: the cascade's stores first);
//   * so after the wait and the acquire the cells the flood can see are exactly as k_relax_settle leaves them, and no later cascade can reach them;
//   * floods write nothing settle reads: flist of the next parity, the claim plane of the next epoch, map cells inside their tiles after the wait.
// Forward progress: flood wavefronts wait for settle wavefronts, never the other way round, and settle wavefronts among themselves as in k_relax_settle, so
// that kernel's argument carries over once all S + F wavefronts are resident together -- relax_settle_floods_plan sizes the grid from THIS kernel's
// occupancy. Every wait honours the spin budget and BC_STALLED.
// nflow: [0] floods that acted, [1] those of them whose gate found a flagged cell (smx_get_relax_flood_flow). prof: SMX_FLOOD_PROF as in k_relax_floods.
__global__ void __launch_bounds__(64) k_relax_settle_floods(DevState s, BatchShared bs, uint32_t epoch, uint32_t lpw, uint32_t nsettle, uint32_t budget, uint32_t prof,
                                                            unsigned long long* ncrowded, unsigned long long* nflow) {
  const uint32_t par = epoch & 1u;
  const bool settle = blockIdx.x < nsettle;
  const uint32_t fb = blockIdx.x - nsettle, nfb = gridDim.x - nsettle;
  uint32_t n = bs.ctrl[(settle ? BC_NFLAG : BC_NFLOOD) + par];
  if (n > (settle ? bs.flag_cap : bs.list_cap)) n = settle ? bs.flag_cap : bs.list_cap;
  uint32_t flpw = (n + nfb - 1u) / nfb;                       // floods per wavefront: as thin as the list allows
  if (flpw > 64u) flpw = 64u;                                 // (n > 64 * nfb cannot happen: the host sizes F for the generation's slots)
  if ((settle ? blockIdx.x * lpw : fb * flpw) >= n) return;   // (sized for the worst case: most blocks leave here)
  SMX_LOAD_SOILS(sh)
  if (settle) { relax_settle_block(s, bs, sh, par, n, lpw, budget, ncrowded); return; }
  const uint32_t i = fb * flpw + threadIdx.x;
  const bool act = threadIdx.x < flpw && i < n;
  bool again = false;
  const uint32_t slot = act ? bs.flist[par][i] : 0u;
  if (!relax_floods_due(bs, epoch, n, bs.ctrl[BC_NRUN + par])) {  // not this epoch: the whole list moves on
    relax_flood_later(bs, slot, par ^ 1u, act);
    return;
  }
  BRect rect = BRect{0, -1, 0, -1};
  bool acts = false;                                          // will batch_water_epoch flood? (its own tests, on words nobody else writes in this launch)
  if (act) {
    const BWater& q = bs.water[slot];
    rect = q.rect;
    acts = q.state == B_ENDED && bs.maxsteps > 0 && water_floods(q.w) && brect_contains(rect, water_intent_flood(s, bs, q.w))
           && rect.tx0 >= bs.txb && rect.tx1 < bs.txe && bholds(bs, (int)par, rect, btag(epoch, slot));
  }
  bool live = true; uint32_t gated = 0u;
  const unsigned long long acting = __ballot(acts);
  for (unsigned long long m = acting; m; m &= m - 1ull) {
    const int owner = __ffsll((long long)m) - 1;
    const BRect r = BRect{__shfl(rect.tx0, owner), __shfl(rect.tx1, owner), __shfl(rect.ty0, owner), __shfl(rect.ty1, owner)};
    bool any = false;
    if (live && !relax_flood_gate(s, bs, r, budget, any)) live = false;   // (stalled: the call fails; stop waiting, let the kernel drain)
    gated += any ? 1u : 0u;
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  if (threadIdx.x == 0u && acting) { atomicAdd(&nflow[0], (unsigned long long)__popcll(acting)); if (gated) atomicAdd(&nflow[1], (unsigned long long)gated); }
  unsigned long long nst = 0;
  if (act) {
    BatchPolicy pol(s, bs);
    Sim<BatchPolicy> sim(s, sh, pol);
    Frame st[MAX_FRAMES];
    const unsigned long long t0 = prof ? wall_clock64() : 0ull;
    batch_water_epoch(sim, bs, slot, epoch, st);
    sim.flush_counters(); nst = pol.a_nsteps; pol.finish(s);
    again = bs.water[slot].state == B_ENDED;
    if (prof) {
      const unsigned long long dt = wall_clock64() - t0;
      if (again) atomicAdd(&g_flood_prof[66], 1ull);
      else { const int b = 63 - __clzll((long long)(dt | 1ull)); atomicAdd(&g_flood_prof[b > 31 ? 31 : b], 1ull); atomicAdd(&g_flood_prof[32 + (b > 31 ? 31 : b)], nst); atomicAdd(&g_flood_prof[64], 1ull); atomicAdd(&g_flood_prof[65], dt); }
    }
  }
  relax_flood_later(bs, slot, par ^ 1u, again);
  relax_commit_flood_steps(s, nst);
}
// The tail of a relaxed water generation (a few hundred particles left, for hundreds of epochs; and every nested generation after
// its first steps): ONE workgroup runs whole epochs back to back -- step, apply, filter, nine cascade colours, floods -- with
// workgroup barriers where the dense schedule has kernel boundaries. Same phases, same order, same results; no launch per phase.
constexpr uint32_t RELAX_TAIL = 256;                          // running particles up to which the tail kernel takes over (one per thread of its
                                                              // workgroup; round 3: 1 024 = four per thread -- 2.6 % slower on the headline, r04 sweep)
static_assert(RELAX_TAIL == 256, "the default of SMX_RELAX_TAIL_AT in ENV_SWITCHES is RELAX_TAIL");
__global__ void __launch_bounds__(256) k_relax_tail(DevState s, BatchShared bs, uint32_t nlive, uint32_t epoch0, uint32_t nepochs, uint32_t tag0) {
  SMX_LOAD_SOILS(sh)
  __shared__ uint32_t busy;
  for (uint32_t k = 0; k < nepochs; k++) {
    const uint32_t epoch = epoch0 + k, par = epoch & 1u;
    bs.rtag = tag0 + k;
    if (threadIdx.x == 0) busy = 0u;
    __syncthreads();
    uint32_t mine = 0u;
    for (uint32_t i = threadIdx.x; i < nlive; i += 256u) {                                       // step
      BatchPolicy pol(s, bs);
      Sim<BatchPolicy> sim(s, sh, pol);
      const uint32_t slot = bs.live[i];
      relax_water_step(sim, bs, slot, epoch);
      mine |= (bs.water[slot].state != B_DONE || bs.rcount[slot] != 0u) ? 1u : 0u;   // (a particle's last step still has edits to apply)
    }
    if (mine) busy = 1u;
    if (threadIdx.x == 0) {                                                                      // the lists of the next epoch start empty
      // (relax_reset_lists spelled out: through the function the compiler also reorders code elsewhere in this kernel -- profiles/r08_refactor_kernel_diff.md)
      bs.ctrl[BC_NFLOOD + (par ^ 1u)] = 0u; bs.ctrl[BC_NFLAG + (par ^ 1u)] = 0u; bs.ctrl[BC_NRUN + (par ^ 1u)] = 0u;
      for (uint32_t q = 0; q < 9u; q++) bs.ctrl[BC_NCASC + 9u * (par ^ 1u) + q] = 0u;
    }
    __syncthreads();
    if (!busy) break;                                                                            // every particle of the generation is done
    for (uint32_t i = threadIdx.x; i < nlive; i += 256u) {                                       // apply
      BatchPolicy pol(s, bs);
      Sim<BatchPolicy> sim(s, sh, pol);
      relax_apply_slot(sim, bs, bs.live[i]);
      sim.flush_counters(); pol.finish(s);
    }
    __syncthreads();
    unsigned long long nc = 0, nt = 0;
    {                                                                                            // filter
      uint32_t n = SMX_A_LOAD(&bs.ctrl[BC_NFLAG + par]);
      if (n > bs.flag_cap) n = bs.flag_cap;
      for (uint32_t i0 = 0; i0 < n; i0 += 256u) {
        const uint32_t i = i0 + threadIdx.x;
        BatchPolicy pol(s, bs);
        Sim<BatchPolicy> sim(s, sh, pol);
        relax_filter(sim, bs, i < n ? bs.flagl[par][i] : 0u, i < n, epoch);
        sim.flush_counters(); pol.finish(s);
        nc += pol.a_casc; nt += pol.a_tr;
      }
    }
    __syncthreads();
    for (uint32_t q = 0; q < 9u; q++) {                                                          // the nine cascade colours
      uint32_t n = SMX_A_LOAD(&bs.ctrl[BC_NCASC + 9u * par + q]);
      if (n > bs.clist_cap) n = bs.clist_cap;
      if (n == 0u) continue;                                                                     // (uniform: every thread reads the same count)
      for (uint32_t i = threadIdx.x; i < n; i += 256u) {
        BatchPolicy pol(s, bs);
        Sim<BatchPolicy> sim(s, sh, pol);
        relax_cascade(sim, bs.clist[par][(size_t)q * bs.clist_cap + i]);
        sim.flush_counters(); pol.finish(s);
        nc += pol.a_casc; nt += pol.a_tr;
      }
      __syncthreads();
    }
    relax_commit_cascade_counters(s, nc, nt);
    {                                                                                            // floods
      uint32_t n = SMX_A_LOAD(&bs.ctrl[BC_NFLOOD + par]);
      if (n > bs.list_cap) n = bs.list_cap;
      const bool due = relax_floods_due(bs, epoch, n, SMX_A_LOAD(&bs.ctrl[BC_NRUN + par]));
      unsigned long long nst = 0;
      for (uint32_t i0 = 0; i0 < n; i0 += 256u) {
        const uint32_t i = i0 + threadIdx.x;
        bool again = false; uint32_t slot = 0u;
        if (i < n && !due) { slot = bs.flist[par][i]; again = true; }                            // not this epoch: the list moves on
        else if (i < n) {
          slot = bs.flist[par][i];
          BatchPolicy pol(s, bs);
          Sim<BatchPolicy> sim(s, sh, pol);
          Frame st[MAX_FRAMES];
          batch_water_epoch(sim, bs, slot, epoch, st);
          sim.flush_counters(); nst += pol.a_nsteps; pol.finish(s);
          again = bs.water[slot].state == B_ENDED;
        }
        relax_flood_later(bs, slot, par ^ 1u, again);
      }
      relax_commit_flood_steps(s, nst);
    }
    __syncthreads();
  }
}
// The DENSE epochs of a relaxed water generation as ONE persistent launch (round 6; OFF by default -- smx_set_relax_launch(1, ..) /
// SMX_RELAX_MEGA=1 turn it on): the same five phases in the same order -- step, apply, filter (isolated cells cascade there), the colour
// lists as a dataflow, floods -- run by a grid of co-resident workgroups (hipLaunchCooperativeKernel) with a device-wide barrier where the
// per-phase launches have kernel boundaries; phases whose list is empty are skipped together with their barrier (the count is read by
// everybody after a barrier, so the decision is uniform). Which lane runs a slot / a cell has no influence on any result (soil_relax.h): the
// state after the launch is the one the per-phase launches leave, bit for bit (tests/test_gpu_relaxed.py runs every launch shape against the
// same host-thread states and against the restatement).
// MEASURED, and why it is not the default (profiles/r06_persistent_epochs.md): the idea was that 5 launches per epoch x 4 352 dense epochs per
// tick are launch-bound. They are not. The barrier itself is cheap -- 6-7 us for 256 workgroups with thread 0 fencing, 2.4 us for 64
// (tools/barrier_bench.hip; no fence: stale reads, counted) -- but an epoch inside this kernel takes 183 us against 143 us as five launches
// (headline workload, k = 8, ticks 4-7: water phase 904 ms against 623; 64 workgroups: 714): workgroup 0's clock puts the step phase at
// 23 + 15 us (its own work + waiting for the slowest workgroup) where k_relax_step takes 9.7 us as a launch of its own, apply at 9 + 18
// (13), and the flood phase at 20 + 48. One kernel holds all five phases' code (240 KB against a 64 KB instruction cache that every
// wavefront walks through once per epoch), is register-allocated for its worst phase (256 VGPR + 96 AGPR, 1.1 KB of scratch per lane: one
// wavefront per SIMD, where the step / apply / filter kernels run at 64-144 registers), and every barrier's acquire invalidates the L2 the
// next phase's first loads -- instructions included -- then miss. Kernel boundaries do the same flushes in hardware, overlapped with the
// dispatch of a kernel compiled for that phase alone. What bounds an epoch is the slowest flood and the slowest cascade, not the launches.
struct GridBar { uint32_t count, gen, busy[2], abort, pad[3]; unsigned long long prof[16]; };   // prof: (flags & 2) ticks of the 100 MHz clock per phase, workgroup 0's view
constexpr uint32_t GB_SPIN_LIMIT = 1u << 22;                  // ~ seconds: a barrier nobody releases sets `abort`, everybody leaves, the host reports it
// The fences are thread 0's alone: a workgroup's stores are acknowledged by its XCD's L2 when __syncthreads() lets it through (the per-CU
// cache writes through), thread 0's release then writes that L2 back, and its acquire after the wait invalidates the CU's cache and the
// L2's stale lines for everybody behind the second __syncthreads(). (Every thread fencing -- 1 024 wavefronts x write-back + invalidate per
// barrier -- cost 65 us per barrier: the first build of this kernel ran the water phase three times slower than five launches per epoch.)
__device__ __forceinline__ bool grid_sync(GridBar* b, uint32_t nblocks, uint32_t& gen, bool every_thread_fences) {
  if (every_thread_fences) __threadfence();
  __syncthreads();
  gen++;
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    if (__hip_atomic_fetch_add(&b->count, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nblocks - 1u) {
      __hip_atomic_store(&b->count, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&b->gen, gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      uint32_t spins = 0;
      while (__hip_atomic_load(&b->gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != gen) {
        __builtin_amdgcn_s_sleep(1);
        if (++spins > GB_SPIN_LIMIT) { __hip_atomic_store(&b->abort, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break; }
        if ((spins & 0x3FFu) == 0u && __hip_atomic_load(&b->abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  }
  __syncthreads();
  if (every_thread_fences) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  return __hip_atomic_load(&b->abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u;   // (the host reads it through bs.ctrl[BC_STALLED], k_relax_epochs)
}
__global__ void __launch_bounds__(256) k_relax_epochs(DevState s, BatchShared bs, uint32_t nlive, uint32_t epoch0, uint32_t nepochs, uint32_t tag0, GridBar* bar, uint32_t dense_waves, uint32_t flags) {
  SMX_LOAD_SOILS(sh)
  // entry i of a list -> lane (i / W) % 64 of wavefront i % W, W wavefronts dealt round robin over the workgroups (wavefront w of the deal =
  // wave w / nblocks of workgroup w % nblocks: the first `nblocks` wavefronts sit on different CUs). Steps, applies and the filter use
  // `dense_waves` wavefronts (one per CU by default, as batch_lanes_per_wave: their paths are uniform, and wavefronts of one CU compete for the
  // instruction cache); floods -- long, branchy, one lane each -- are dealt over ALL wavefronts.
  const uint32_t NW = gridDim.x * 4u, lane = threadIdx.x & 63u, gw = (threadIdx.x >> 6) * gridDim.x + blockIdx.x;
  const bool fence_all = (flags & 1u) != 0u, prof = (flags & 2u) != 0u && blockIdx.x == 0 && threadIdx.x == 0;
  unsigned long long t_prev = prof ? wall_clock64() : 0ull;
#define SMX_PROF(slot) if (prof) { const unsigned long long t_now = wall_clock64(); bar->prof[slot] += t_now - t_prev; t_prev = t_now; }
  uint32_t DW = dense_waves < 1u ? 1u : (dense_waves > NW ? NW : dense_waves);
  { const uint32_t need = (nlive + 63u) / 64u; if (need > DW) DW = need > NW ? NW : need; }
  const uint32_t first = lane * DW + gw, stride = 64u * DW;    // (gw >= DW: this wavefront sits the dense phases out)
  uint32_t gen = __hip_atomic_load(&bar->gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (uint32_t k = 0; k < nepochs; k++) {
    const uint32_t epoch = epoch0 + k, par = epoch & 1u;
    bs.rtag = tag0 + k;
    unsigned long long nc = 0, nt = 0;
    {                                                                                            // ---- step
      uint32_t mine = 0u;
      for (uint32_t i = first; gw < DW && i < nlive; i += stride) {
        BatchPolicy pol(s, bs);
        Sim<BatchPolicy> sim(s, sh, pol);
        const uint32_t slot = bs.live[i];
        relax_water_step(sim, bs, slot, epoch);
        mine |= (bs.water[slot].state != B_DONE || bs.rcount[slot] != 0u) ? 1u : 0u;            // (a particle's last step still has edits to apply)
      }
      if (mine) __hip_atomic_store(&bar->busy[k & 1u], bs.rtag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (tags are unique and never 0: nothing to reset)
      if (blockIdx.x == 0 && threadIdx.x == 0) {                                                 // the lists of the next epoch start empty
        // (relax_reset_lists spelled out, as in k_relax_tail)
        bs.ctrl[BC_NFLOOD + (par ^ 1u)] = 0u; bs.ctrl[BC_NFLAG + (par ^ 1u)] = 0u; bs.ctrl[BC_NRUN + (par ^ 1u)] = 0u;
        for (uint32_t q = 0; q < 9u; q++) bs.ctrl[BC_NCASC + 9u * (par ^ 1u) + q] = 0u;
        bs.ctrl[BC_CASC_CURSOR] = 0u;
      }
    }
    SMX_PROF(0)
    if (!grid_sync(bar, gridDim.x, gen, fence_all)) { bs.ctrl[BC_STALLED] = 1u; return; }
    SMX_PROF(1)
    if (__hip_atomic_load(&bar->busy[k & 1u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != bs.rtag) break;   // every particle of the generation is done
    for (uint32_t i = first; gw < DW && i < nlive; i += stride) {                                // ---- apply
      BatchPolicy pol(s, bs);
      Sim<BatchPolicy> sim(s, sh, pol);
      relax_apply_slot(sim, bs, bs.live[i]);
      sim.flush_counters(); pol.finish(s);
    }
    SMX_PROF(2)
    if (!grid_sync(bar, gridDim.x, gen, fence_all)) { bs.ctrl[BC_STALLED] = 1u; return; }
    SMX_PROF(3)
    {                                                                                            // ---- filter (isolated cells cascade in here)
      uint32_t n = __hip_atomic_load(&bs.ctrl[BC_NFLAG + par], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (n > bs.flag_cap) n = bs.flag_cap;
      if (n) {
        uint32_t FW = DW; { const uint32_t need = (n + 63u) / 64u; if (need > FW) FW = need > NW ? NW : need; }
        for (uint32_t i0 = gw; gw < FW && i0 < n; i0 += 64u * FW) {                              // (wavefront-uniform trip count: relax_filter appends with ballots)
          const uint32_t i = i0 + lane * FW;
          BatchPolicy pol(s, bs);
          Sim<BatchPolicy> sim(s, sh, pol);
          relax_filter(sim, bs, i < n ? bs.flagl[par][i] : 0u, i < n, epoch);
          sim.flush_counters(); pol.finish(s);
          nc += pol.a_casc; nt += pol.a_tr;
        }
        SMX_PROF(4)
        if (!grid_sync(bar, gridDim.x, gen, fence_all)) { bs.ctrl[BC_STALLED] = 1u; return; }
        SMX_PROF(5)
      }
    }
    {                                                                                            // ---- the colour lists: the dataflow of k_relax_cascade_flow, a cell per wavefront
      uint32_t cnt[9], total = 0;
#pragma unroll
      for (uint32_t q = 0; q < 9u; q++) {
        uint32_t n = __hip_atomic_load(&bs.ctrl[BC_NCASC + 9u * par + q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (n > bs.clist_cap) n = bs.clist_cap;
        cnt[q] = n; total += n;
      }
      if (total) {
        const uint32_t pending = 2u * bs.rtag;
        while (true) {
          uint32_t i = 0u;
          if (lane == 0u) i = atomicAdd(&bs.ctrl[BC_CASC_CURSOR], 1u);
          i = (uint32_t)__shfl((int)i, 0);
          if (i >= total) break;
          if (lane == 0u) {
            uint32_t q = 0;
#pragma unroll
            for (uint32_t c9 = 0; c9 < 9u; c9++) { if (q == c9 && i >= cnt[c9]) { i -= cnt[c9]; q = c9 + 1u; } }
            const uint32_t c = bs.clist[par][(size_t)q * bs.clist_cap + i];
            const int x = (int)(c / (uint32_t)s.dimy), y = (int)(c - (uint32_t)x * (uint32_t)s.dimy);
            const int xa = x - 2 < s.x_lo ? s.x_lo : x - 2, xb = x + 2 >= s.x_hi ? s.x_hi - 1 : x + 2;
            const int ya = y - 2 < 0 ? 0 : y - 2, yb = y + 2 >= s.dimy ? s.dimy - 1 : y + 2;
            uint32_t spins = 0;
            for (int xx = xa; xx <= xb; xx++)
              for (int yy = ya; yy <= yb; yy++) {
                if ((uint32_t)((xx % 3) * 3 + (yy % 3)) >= q) continue;                          // (only cells of an earlier colour; the cell itself has colour q)
                uint32_t* f = &bs.cstate[(size_t)xx * (size_t)s.dimy + (size_t)yy];
                while (__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == pending) {
                  __builtin_amdgcn_s_sleep(2);
                  if (++spins > GB_SPIN_LIMIT) { __hip_atomic_store(&bar->abort, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break; }
                }
              }
            __atomic_thread_fence(__ATOMIC_ACQUIRE);
            BatchPolicy pol(s, bs);
            Sim<BatchPolicy> sim(s, sh, pol);
            relax_cascade(sim, c);
            sim.flush_counters(); pol.finish(s);
            nc += pol.a_casc; nt += pol.a_tr;
            __hip_atomic_store(&bs.cstate[c], pending + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
          }
        }
        SMX_PROF(6)
        if (!grid_sync(bar, gridDim.x, gen, fence_all)) { bs.ctrl[BC_STALLED] = 1u; return; }
        SMX_PROF(7)
      }
    }
    relax_commit_cascade_counters(s, nc, nt);
    {                                                                                            // ---- floods (and their nested particles), one per wavefront while the list allows
      uint32_t n = __hip_atomic_load(&bs.ctrl[BC_NFLOOD + par], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (n > bs.list_cap) n = bs.list_cap;
      if (n) {
        const bool due = relax_floods_due(bs, epoch, n, __hip_atomic_load(&bs.ctrl[BC_NRUN + par], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        unsigned long long nst = 0;
        for (uint32_t i0 = gw; i0 < n; i0 += 64u * NW) {
          const uint32_t i = i0 + lane * NW;
          bool again = false; uint32_t slot = 0u;
          if (i < n && !due) { slot = bs.flist[par][i]; again = true; }                          // not this epoch: the list moves on
          else if (i < n) {
            slot = bs.flist[par][i];
            BatchPolicy pol(s, bs);
            Sim<BatchPolicy> sim(s, sh, pol);
            Frame st[MAX_FRAMES];
            batch_water_epoch(sim, bs, slot, epoch, st);
            sim.flush_counters(); nst += pol.a_nsteps; pol.finish(s);
            again = bs.water[slot].state == B_ENDED;
          }
          relax_flood_later(bs, slot, par ^ 1u, again);
        }
        relax_commit_flood_steps(s, nst);
        SMX_PROF(8)
        if (!grid_sync(bar, gridDim.x, gen, fence_all)) { bs.ctrl[BC_STALLED] = 1u; return; }
        SMX_PROF(9)
      }
    }
    if (prof) bar->prof[10] += 1ull;
  }
#undef SMX_PROF
}
// how many particles share a wavefront: as few as fill `SMX_BATCH_WAVES` wavefronts (default 256 = one per CU; 0 = always 64;
// measured in profiles/r02_batched_schedules.md, sweep 5). Which lane runs a slot has no influence on results.
static uint32_t batch_lanes_per_wave(uint32_t nlive) {
  static const uint32_t waves = (uint32_t)env_int("SMX_BATCH_WAVES");
  if (!waves) return 64u;
  const uint32_t l = (nlive + waves - 1u) / waves;
  return l < 1u ? 1u : (l > 64u ? 64u : l);
}
// rebuild the list of slots that still run (order is irrelevant: a slot's identity is its index, not its lane)
template <bool WIND>
__global__ void __launch_bounds__(256) k_batch_compact(BatchShared bs, uint32_t nslots) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const uint32_t st_ = i < nslots ? (WIND ? bs.wind[i].state : bs.water[i].state) : B_DONE;
  const bool alive = st_ != B_DONE && st_ != B_AWAY;
  const unsigned long long m = __ballot(alive);
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t base = 0;
  if (lane == 0 && m) base = atomicAdd(&bs.ctrl[BC_NLIVE], (uint32_t)__popcll(m));
  base = (uint32_t)__shfl((int)base, 0);
  if (alive) bs.live[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = i;
}
__global__ void __launch_bounds__(256) k_batch_iota(uint32_t* live, uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) live[i] = i;
}
// between kernels: nodes released during the last kernel go back on the free stack
__global__ void __launch_bounds__(256) k_batch_merge_freed(DevState s, BatchShared bs) {
  uint32_t nf = bs.ctrl[BC_NFREED];
  if (nf > bs.freed_cap) nf = bs.freed_cap;
  const uint32_t base = *s.free_count;
  for (uint32_t i = threadIdx.x; i < nf; i += 256u) s.freelist[base + i] = bs.freed[i];
  __syncthreads();
  if (threadIdx.x == 0) { *s.free_count = base + nf; bs.ctrl[BC_NFREED] = 0; }
}
template <bool WIND>
__global__ void __launch_bounds__(256) k_batch_counters(DevState s, BatchShared bs, uint32_t nslots) {
  unsigned long long acc[4] = {0, 0, 0, 0};
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < nslots; i += gridDim.x * 256u) batch_slot_counters(bs, WIND, i, acc);
#pragma unroll
  for (int k = 0; k < 4; k++)
    for (int off = 32; off > 0; off >>= 1) acc[k] += (unsigned long long)__shfl_down((long long)acc[k], off);
  if ((threadIdx.x & 63u) == 0) batch_commit_counters(s, WIND, acc);
}
// ---------------- grid pass (water.h:335-343) over the 8x8-cell tiles (soil_batch.h GRID_SHIFT) ----------------
// A tile's seep + cascade(.., 3) -- and the nested particles that run inside it -- stay in the tile and the ring of tiles around it (its
// REGION). Regions of tiles two or less apart overlap; such tiles have different colours (tx mod 3, ty mod 3) and are swept in colour
// order. The sweep is a DATAFLOW over the tiles that have work, sorted by (colour, tile): a wavefront takes the next entry, waits until
// every tile of a smaller colour within two tiles of its own that has work is done, sweeps its tile (lane 0) and publishes it. A tile only
// waits for entries before its own, taken by wavefronts that are running: no deadlock; chains of waiting tiles are at most nine long, and
// a tile in a quiet corner never waits for the slowest tile of a colour somewhere else (nine launches with a barrier each: 9 x 5 ms in
// round 4, with 16-cell tiles and no nested particles inside). One tile per wavefront: a tile is a long, branchy path, and lanes of one
// wavefront cannot wait for each other. The order of conflicting tiles is fixed, so the result is the colour-by-colour sweep's.
constexpr uint32_t GT_PENDING = 0xFFFFFFFFu;
struct GridTiles {
  uint32_t* tdone;                            // [held tile columns][gty]: 0 = nothing to do here, GT_PENDING, 1 = swept
  uint32_t* pend[2];                          // entries colour * (gtx * gty) + tile (tile = tx * gty + ty): as appended / sorted
  uint32_t* count;                            // [0] entries, [1] the dataflow kernel's cursor
  int gtx, gty, txb, txe;                     // tiles of the map; tile columns [txb, txe) held by tdone
  int tx_lo, tx_hi;                           // tile columns of this sweep
  unsigned long long keybase;                 // key prefix of a tile's children: keybase + entry
};
__global__ void __launch_bounds__(256) k_grid_tiles_init(DevState s, BatchShared bs, GridTiles g) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const uint32_t ncol = (uint32_t)(g.tx_hi - g.tx_lo);
  bool act = false; uint32_t entry = 0;
  if (i < ncol * (uint32_t)g.gty) {
    const int tx = g.tx_lo + (int)(i / (uint32_t)g.gty), ty = (int)(i % (uint32_t)g.gty);
    entry = (uint32_t)((tx % 3) * 3 + (ty % 3)) * ((uint32_t)g.gtx * (uint32_t)g.gty) + (uint32_t)tx * (uint32_t)g.gty + (uint32_t)ty;
    if (batch_grid_tile_phase(s, bs, tx)) {
      const int x0 = tx << GRID_SHIFT, y0 = ty << GRID_SHIFT;
      for (int x = x0; x < x0 + (1 << GRID_SHIFT) && x < s.dimx; x++) {   // (a tile row = 8 consecutive bits of the bitmap)
        const size_t c = (size_t)x * s.dimy + y0;
        int len = s.dimy - y0; if (len > (1 << GRID_SHIFT)) len = 1 << GRID_SHIFT;
        for (int y = 0; y < len; y++) act |= ((s.active[(c + y) >> 6] >> ((c + y) & 63)) & 1ull) != 0ull;
      }
    }
    g.tdone[(size_t)(tx - g.txb) * g.gty + ty] = act ? GT_PENDING : 0u;
  }
  const uint32_t k = relax_append(&g.count[0], act);
  if (act) g.pend[0][k] = entry;
}
// (experiments, SMX_FLOOD_PROF=1: where does a sweep go? [0..31] tiles by log2 of their sweep time in 100 MHz ticks, [32..63] their active cells, [72..103] the steps of
//  their nested particles, [64] tiles, [65] ticks sweeping, [66] ticks waiting for tiles of earlier colours, [67] the longest sweep; printed by smx_destroy)
__device__ unsigned long long g_tile_prof[104];
__global__ void __launch_bounds__(64) k_grid_tiles_flow(DevState s, BatchShared bs, GridTiles g, const uint32_t* __restrict__ order, uint32_t n, uint32_t poll_naps_prof, uint32_t budget) {
  const uint32_t poll_naps = poll_naps_prof & 0x7FFFFFFFu; const bool prof = (poll_naps_prof >> 31) != 0u;
  SMX_LOAD_SOILS(sh)
  __shared__ uint32_t s_i;
  unsigned long long vis = 0, gns = 0;
  const uint32_t nt = (uint32_t)g.gtx * (uint32_t)g.gty;
  bool live = true;
  while (true) {
    if (threadIdx.x == 0) s_i = atomicAdd(&g.count[1], 1u);
    __syncthreads();
    const uint32_t i = s_i;
    __syncthreads();
    if (i >= n) break;
    if (threadIdx.x == 0) {
      const uint32_t entry = order[i], col = entry / nt, tile = entry - col * nt;
      const int tx = (int)(tile / (uint32_t)g.gty), ty = (int)(tile % (uint32_t)g.gty);
      const unsigned long long tw0 = prof ? wall_clock64() : 0ull;
      for (int dx = -2; dx <= 2; dx++)                         // the tiles whose region overlaps this one's and whose colour comes first
        for (int dy = -2; dy <= 2; dy++) {
          const int ax = tx + dx, ay = ty + dy;
          if ((!dx && !dy) || ax < g.tx_lo || ax >= g.tx_hi || ax < g.txb || ax >= g.txe || ay < 0 || ay >= g.gty) continue;
          if ((uint32_t)((ax % 3) * 3 + (ay % 3)) >= col) continue;
          uint32_t* f = &g.tdone[(size_t)(ax - g.txb) * g.gty + ay];
          // (a tile takes milliseconds: its dependants poll every few microseconds -- rocprofv3 counted 122 M polling loads per launch at one poll per 0.2 us, profiles/r06_pmc.json)
          if (live && !spin_wait_while(f, GT_PENDING, &bs.ctrl[BC_STALLED], budget, 8u, poll_naps)) live = false;   // (stalled: the call fails; stop waiting, let the kernel drain)
        }
      __atomic_thread_fence(__ATOMIC_ACQUIRE);                 // what the tiles before wrote to the map is visible from here on
      BatchPolicy pol(s, bs);
      Sim<BatchPolicy> sim(s, sh, pol);
      Frame st[MAX_FRAMES];
      const unsigned long long ts0 = prof ? wall_clock64() : 0ull;
      const unsigned long long vt = batch_grid_tile(sim, tx, ty, g.keybase + (unsigned long long)entry, st);
      vis += vt;
      sim.flush_counters(); gns += pol.a_nsteps;
      if (prof) {
        const unsigned long long dt = wall_clock64() - ts0;
        int b = 63 - __clzll((long long)(dt | 1ull)); if (b > 31) b = 31;
        atomicAdd(&g_tile_prof[b], 1ull); atomicAdd(&g_tile_prof[32 + b], vt); atomicAdd(&g_tile_prof[72 + b], (unsigned long long)pol.a_nsteps);
        atomicAdd(&g_tile_prof[64], 1ull); atomicAdd(&g_tile_prof[65], dt); atomicAdd(&g_tile_prof[66], ts0 - tw0); atomicMax(&g_tile_prof[67], dt);
      }
      pol.finish(s);
      __hip_atomic_store(&g.tdone[(size_t)(tx - g.txb) * g.gty + ty], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  if (threadIdx.x == 0 && vis) atomicAdd(&s.ctr[C_GRID_ACTIVE], vis);
  if (threadIdx.x == 0 && gns) atomicAdd(&s.ctr[C_GRID_NESTED_STEPS], gns);
}
__global__ void k_batch_grid_finish(DevState s, unsigned long long visited0) {   // counter parity: every other cell "calls" cascade once
  const unsigned long long n = (unsigned long long)s.dimx * s.dimy, v = s.ctr[C_GRID_ACTIVE] - visited0;
  s.ctr[C_WCASCADE_CALLS] += n - v;
}

// ---------------- column strips on several devices: halo columns, migrating particles (library driver: soil_strips_host.h; Python restatement: tests/strips_ref.py) ----------------
__global__ void __launch_bounds__(64) k_batch_child_contains(const BChild* kids, uint32_t nslots, uint32_t* out) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i < nslots) out[i] = batch_child_contains(kids, i);
}
struct XCursor { unsigned long long bytes; uint32_t nrec, lost; };
// every column of the DIRTY 4x4 grid tiles whose x lies in [gx0, gx1) tiles: one thread per tile walks its 16 columns twice
// (size, then content); space comes from two atomic cursors, so records land in any order (they are independent)
__global__ void __launch_bounds__(64) k_strip_pack_columns(DevState s, BatchShared bs, int gx0, int gx1, uint8_t* data, unsigned long long cap,
                                                            uint32_t* offs, uint32_t offs_cap, XCursor* cur) {
  const int gty = (s.dimy + 3) >> 2;
  const long long t = (long long)blockIdx.x * 64 + threadIdx.x;
  if (t >= (long long)(gx1 - gx0) * gty) return;
  const int gx = gx0 + (int)(t / gty), gy = (int)(t % gty);
  uint8_t& dflag = bs.dirty[(size_t)gx * gty + gy];
  if (!dflag) return;
  dflag = 0;
  uint32_t ncol = 0; unsigned long long need = 0;
  for (int x = gx << 2; x < (gx << 2) + 4 && x < s.dimx; x++)
    for (int y = gy << 2; y < (gy << 2) + 4 && y < s.dimy; y++) {
      const Sec& c = s.cells[(size_t)x * s.dimy + y];
      uint32_t k = 0;
      if (c.type != EMPTY) { k = 1; for (uint32_t pv = c.prev; pv != NIL; pv = s.pool[pv].prev) k++; }
      need += 24ull + 32ull * k; ncol++;
    }
  const unsigned long long base = atomicAdd(&cur->bytes, need);
  const uint32_t rbase = atomicAdd(&cur->nrec, ncol);
  if (base + need > cap || rbase + ncol > offs_cap) { atomicAdd(&cur->lost, 1u); return; }
  unsigned long long o = base; uint32_t r = rbase;
  for (int x = gx << 2; x < (gx << 2) + 4 && x < s.dimx; x++)
    for (int y = gy << 2; y < (gy << 2) + 4 && y < s.dimy; y++) {
      const size_t cc = (size_t)x * s.dimy + y, fi = (size_t)y * s.dimx + x;
      const Sec& c = s.cells[cc];
      uint32_t k = 0;
      if (c.type != EMPTY) { k = 1; for (uint32_t pv = c.prev; pv != NIL; pv = s.pool[pv].prev) k++; }
      offs[r++] = (uint32_t)(o - base) + (uint32_t)base;       // (offsets are relative to the start of the data area; < 4 GiB)
      uint32_t* h = reinterpret_cast<uint32_t*>(data + o);
      h[0] = (uint32_t)cc; h[1] = k; h[2] = __float_as_uint(s.wtrack[fi]); h[3] = __float_as_uint(s.windfreq[fi]); h[4] = s.flags[cc]; h[5] = 0;
      // sections bottom -> top: the chain is top -> bottom, so fill from the back
      const Sec* t2 = &c;
      for (uint32_t j = k; j-- > 0;) {
        double* q = reinterpret_cast<double*>(data + o + 24 + 32ull * j);
        q[0] = t2->size; q[1] = t2->floor; q[2] = t2->sat;
        reinterpret_cast<uint32_t*>(q + 3)[0] = t2->type; reinterpret_cast<uint32_t*>(q + 3)[1] = 0;
        if (t2->prev != NIL) t2 = &s.pool[t2->prev];
      }
      o += 24ull + 32ull * k;
    }
}
// one thread per received column: give the old chain back (deferred, like every free of a batched kernel), build the new one
__global__ void __launch_bounds__(64) k_strip_unpack_columns(DevState s, BatchShared bs, const uint8_t* data, const uint32_t* offs, uint32_t nrec, uint32_t nbytes) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= nrec) return;
  if ((unsigned long long)offs[i] + 24ull > nbytes) return;  // (records must lie inside the message)
  const uint8_t* r = data + offs[i];
  const uint32_t* h = reinterpret_cast<const uint32_t*>(r);
  const uint32_t cc = h[0], count = h[1];
  if (cc >= (unsigned long long)s.dimx * s.dimy || (unsigned long long)offs[i] + 24ull + 32ull * count > nbytes) return;
  if (cc < (unsigned long long)s.x_lo * s.dimy || cc >= (unsigned long long)s.x_hi * s.dimy) return;   // (a strip context holds [x_lo, x_hi) only: cells / flags are biased pointers)
  const size_t x = cc / (size_t)s.dimy, y = cc % (size_t)s.dimy, fi = y * (size_t)s.dimx + x;
  s.wtrack[fi] = __uint_as_float(h[2]); s.windfreq[fi] = __uint_as_float(h[3]);
  BatchPolicy pol(s, bs);
  long long live = 0;
  Sec& c = s.cells[cc];
  if (c.type != EMPTY) { live--; uint32_t pv = c.prev; while (pv != NIL) { const uint32_t nx = s.pool[pv].prev; pol.node_free(s, pv); pv = nx; live--; } }
  Sec cell; cell.size = 0.0; cell.floor = 0.0; cell.sat = 0.0; cell.type = EMPTY; cell.prev = NIL;
  uint32_t pv = NIL;
  for (uint32_t k = 0; k < count; k++) {
    const double* q = reinterpret_cast<const double*>(r + 24 + 32ull * k);
    Sec t; t.size = q[0]; t.floor = q[1]; t.sat = q[2]; t.type = reinterpret_cast<const uint32_t*>(q + 3)[0]; t.prev = pv;
    live++;
    if (k + 1 == count) cell = t;
    else {
      const uint32_t nd = pol.node_alloc(s);
      if (nd == NIL) { atomicAdd(&s.ctr[C_POOL_OVERFLOW], 1ull); cell = t; break; }   // out of nodes: the column keeps what fits (reported, not silent)
      s.pool[nd] = t; pv = nd;
    }
  }
  c = cell; s.flags[cc] = (uint8_t)h[4];
  if (live) atomicAdd(&s.ctr[C_LIVE_SECTIONS], (unsigned long long)live);
}
template <bool WIND>
__global__ void __launch_bounds__(256) k_strip_pack_particles(BatchShared bs, uint32_t nslots, int x0, int x1, uint8_t* data, unsigned long long cap, XCursor* cur) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= nslots) return;
  uint32_t& st = WIND ? bs.wind[i].state : bs.water[i].state;
  if (st == B_DONE || st == B_AWAY) return;
  const int ix = WIND ? bs.wind[i].d.ix : bs.water[i].w.ix;
  if (ix < x0 || ix >= x1) return;
  constexpr unsigned long long rs = 4 + (WIND ? sizeof(BWind) : sizeof(BWater));
  const uint32_t k = atomicAdd(&cur->nrec, 1u);
  if ((k + 1ull) * rs > cap) { atomicAdd(&cur->lost, 1u); return; }
  uint8_t* o = data + k * rs;
  memcpy(o, &i, 4);
  if constexpr (WIND) memcpy(o + 4, &bs.wind[i], sizeof(BWind)); else memcpy(o + 4, &bs.water[i], sizeof(BWater));
  st = B_AWAY;
}
template <bool WIND>
__global__ void __launch_bounds__(256) k_strip_unpack_particles(BatchShared bs, const uint8_t* data, uint32_t n) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n) return;
  constexpr unsigned long long rs = 4 + (WIND ? sizeof(BWind) : sizeof(BWater));
  const uint8_t* o = data + k * rs;
  uint32_t i; memcpy(&i, o, 4);
  if constexpr (WIND) memcpy(&bs.wind[i], o + 4, sizeof(BWind)); else memcpy(&bs.water[i], o + 4, sizeof(BWater));
}
SMX_D float map_frequency1(float f, float t) {   // water.h:358-365
  const float lrate = 0.01f, K = 50.0f;      // water.h:359-360
  return (1.0f - lrate) * f + lrate * K * t / (1.0f + K * t);
}
__global__ void __launch_bounds__(256) k_map_frequency(float* __restrict__ freq, const float* __restrict__ track, size_t n4, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t k = i; k < n4; k += stride) {
    float4 f = reinterpret_cast<float4*>(freq)[k];
    const float4 t = reinterpret_cast<const float4*>(track)[k];
    f.x = map_frequency1(f.x, t.x);
    f.y = map_frequency1(f.y, t.y);
    f.z = map_frequency1(f.z, t.z);
    f.w = map_frequency1(f.w, t.w);
    reinterpret_cast<float4*>(freq)[k] = f;
  }
  for (size_t k = n4 * 4 + i; k < n; k += stride)
    freq[k] = map_frequency1(freq[k], track[k]);
}
// ensembles: k_map_frequency followed by the reset of the water track (smx_map_frequency + smx_reset_frequency, water.h:353-365) in
// one pass, member blockIdx.y; a cell's track is read before it is cleared, as in the two steps
__global__ void __launch_bounds__(256) k_ens_frequency(const EnsEntry* __restrict__ tab_) {
  EnsTab* tab = ens_tab(tab_);
  if (!tab[blockIdx.y].on) return;
  const DevState s = tab[blockIdx.y].s;
  const size_t n = (size_t)s.dimx * s.dimy, n4 = n / 4;
  float* __restrict__ freq = s.wfreq;
  float* __restrict__ track = s.wtrack;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t k = i; k < n4; k += stride) {
    float4 f = reinterpret_cast<float4*>(freq)[k];
    const float4 t = reinterpret_cast<const float4*>(track)[k];
    f.x = map_frequency1(f.x, t.x);
    f.y = map_frequency1(f.y, t.y);
    f.z = map_frequency1(f.z, t.z);
    f.w = map_frequency1(f.w, t.w);
    reinterpret_cast<float4*>(freq)[k] = f;
    reinterpret_cast<float4*>(track)[k] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  for (size_t k = n4 * 4 + i; k < n; k += stride) {
    freq[k] = map_frequency1(freq[k], track[k]);
    track[k] = 0.f;
  }
}

// Layermap::initialize (layermap.h:163-216). One thread per cell builds its whole column: the layers are
// added in file order with the rules of Layermap::add (merge same type, water swap, push). Pool nodes for
// buried sections come from an atomic bump on the free stack (node identity is unobservable).
struct LayerDev { uint32_t type; float min, bias, scale; NoiseCfg noise; float z; };
constexpr int MAX_LAYERS = 16;
struct LayersDev { int n; LayerDev l[MAX_LAYERS]; };

__global__ void __launch_bounds__(256) k_init_terrain(DevState s, LayersDev L) {
  const size_t n = (size_t)s.x_hi * s.dimy;
  const size_t c = (size_t)s.x_lo * s.dimy + (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  const int i = (int)(c / s.dimy), j = (int)(c % s.dimy);
  double csize[MAX_LAYERS]; uint32_t ctype[MAX_LAYERS];
  int ns = 0;
  const float px = (float)i / (float)s.dimx, py = (float)j / (float)s.dimy;
  for (int l = 0; l < L.n; l++) {
    float val = L.l[l].bias + L.l[l].scale * noise_fbm(L.l[l].noise, px, py, L.l[l].z);   // SurfLayer::get surface.h:95-99
    if (val < L.l[l].min) val = L.l[l].min;
    const double h = val;
    const uint32_t t = L.l[l].type;
    if (h <= 0) continue;                                        // layermap.h:237-240
    if (ns == 0) { csize[0] = h; ctype[0] = t; ns = 1; continue; }
    if (ctype[ns - 1] == t) { csize[ns - 1] += h; continue; }    // :249-253
    if (ctype[ns - 1] == AIR) {                                  // :258-275 water swap
      const double wsize = csize[ns - 1];
      ns--;
      if (ns > 0 && ctype[ns - 1] == t) csize[ns - 1] += h;
      else { csize[ns] = h; ctype[ns] = t; ns++; }
      csize[ns] = wsize; ctype[ns] = AIR; ns++;
      continue;
    }
    csize[ns] = h; ctype[ns] = t; ns++;
  }
  Sec cell;
  cell.size = 0.0; cell.floor = 0.0; cell.sat = 0.0; cell.type = EMPTY; cell.prev = NIL;
  uint8_t flag = 0;
  if (ns > 0) {
    uint32_t base = 0;
    if (ns > 1) {
      base = atomicSub(s.free_count, (uint32_t)(ns - 1));             // old count: our nodes are freelist[base-ns+1 .. base-1]
      if (base < (uint32_t)(ns - 1) || base > (uint32_t)s.pool_capacity) {   // out of nodes (smx_initialize rules this out: guard only)
        atomicAdd(&s.ctr[C_POOL_OVERFLOW], 1ull);
        ns = 1;                                                       // keep the bottom section only, touch nothing out of bounds
      }
    }
    double fl = 0.0;
    uint32_t pv = NIL;
    for (int k = 0; k < ns; k++) {
      Sec r; r.size = csize[k]; r.floor = fl; r.sat = 0.0; r.type = ctype[k]; r.prev = pv;
      if (k == ns - 1) cell = r;
      else { const uint32_t nd = s.freelist[base - 1 - k]; s.pool[nd] = r; pv = nd; }
      fl = r.floor + r.size;                                     // E->floor = height(pos) (:304)
    }
    if (cell.type == AIR) flag |= F_AIR;
    atomicAdd(&s.ctr[C_LIVE_SECTIONS], (unsigned long long)ns);
  }
  s.cells[c] = cell;
  s.flags[c] = flag;
}

__global__ void __launch_bounds__(256) k_heights(DevState s, double* __restrict__ out) {   // (out: the held range, first cell at out[0])
  const size_t n = (size_t)s.x_hi * s.dimy, c_lo = (size_t)s.x_lo * s.dimy;
  const size_t c = c_lo + (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c < n) out[c - c_lo] = s.cells[c].floor + s.cells[c].size;
}
__global__ void __launch_bounds__(256) k_surface(DevState s, uint32_t* __restrict__ out) {
  const size_t n = (size_t)s.x_hi * s.dimy, c_lo = (size_t)s.x_lo * s.dimy;
  const size_t c = c_lo + (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c < n) { uint32_t t = s.cells[c].type; out[c - c_lo] = (t == EMPTY) ? 0u : t; }
}
__global__ void __launch_bounds__(256) k_normals(DevState s, float* __restrict__ out) {
  const size_t n = (size_t)s.dimx * s.dimy;
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  SerialPolicy pol(s);
  Sim<SerialPolicy> sim(s, s.soils, pol);
  f3 v = sim.normal((int)(c / s.dimy), (int)(c % s.dimy));
  out[3 * c] = v.x; out[3 * c + 1] = v.y; out[3 * c + 2] = v.z;
}
// Layermap::update(Vertexpool&) for the whole map (layermap.h:475-555): one 44-byte vertex per column. A thread
// builds its vertex in LDS, the block then streams its 256 x 11 floats out as one contiguous run (a 44-byte
// stride per thread would scatter every store over two lines).
// mode -1: no cut (the top section). mode 0: Layermap::update's SLICE cut (layermap.h:477-510). mode 1: Layermap::slice(s)
// (layermap.h:557-613). thr = the cut height in map units, ycut = the y written for a cut column.
struct VCut { int mode; double thr; float ycut; unsigned block0 = 0, rel = 0; };   // block0: first 256-cell block of the launch; rel: `out` holds that block only (one column: smx_fill_vertex_cut)
__global__ void __launch_bounds__(256) k_fill_vertices(DevState s, const float* __restrict__ colors4, uint32_t ncolors,
                                                       float* __restrict__ out, VCut cut) {
  __shared__ float stage[256 * 11];
  const size_t n = (size_t)s.dimx * s.dimy;
  const size_t c0 = ((size_t)blockIdx.x + cut.block0) * 256, c = c0 + threadIdx.x;
  if (c < n) {
    const int x = (int)(c / s.dimy), y = (int)(c % s.dimy);
    Sec r = s.cells[c];
    bool have = r.type != EMPTY;
    if (cut.mode >= 0)                                        // the first section that starts at or below the cut
      while (have && r.floor > cut.thr) { if (r.prev == NIL) have = false; else r = s.pool[r.prev]; }
    const uint32_t ty = have ? r.type : 0u;
    const double h = have ? r.floor + r.size : 0.0;
    float* v = stage + threadIdx.x * 11;
    f3 nrm = {0.f, 1.f, 0.f};
    float py = 0.f;
    uint32_t ci = 0;
    float col[4];
    bool plain = true;                                        // colour = colors4[ci]
    if (cut.mode >= 0 && have && h > cut.thr) {               // the section is cut: flat top at the cut height
      py = cut.ycut;
      const bool wet = r.floor + r.size * r.sat > cut.thr;
      ci = (cut.mode == 0 && wet) ? 0u : ty;
      if (wet) {                                              // mix(a, colour, 0.6) in double (glm), a = Air's colour / red
        plain = false;
        const uint32_t ct = ty < ncolors ? ty : 0u;
        const float a[4] = {cut.mode == 0 ? colors4[0] : 1.f, cut.mode == 0 ? colors4[1] : 0.f, cut.mode == 0 ? colors4[2] : 0.f, cut.mode == 0 ? colors4[3] : 1.f};
        for (int k = 0; k < 4; k++) col[k] = (float)((double)a[k] * (1.0 - 0.6) + (double)colors4[4 * ct + k] * 0.6);
      }
    } else if (cut.mode >= 0 ? have : !(h == 0.0 && ty == 0u)) {
      SerialPolicy pol(s);
      Sim<SerialPolicy> sim(s, s.soils, pol);
      nrm = sim.normal(x, y);
      py = (float)(s.scale * h);
      ci = ty;
      if (cut.mode == 1 && r.sat == 0.0) { plain = false; col[0] = 1.f; col[1] = 0.f; col[2] = 0.f; col[3] = 1.f; }   // :598-604
    }
    const uint32_t cc = ci < ncolors ? ci : 0u;
    if (plain) { col[0] = colors4[4 * cc]; col[1] = colors4[4 * cc + 1]; col[2] = colors4[4 * cc + 2]; col[3] = colors4[4 * cc + 3]; }
    v[0] = (float)x; v[1] = py; v[2] = (float)y;
    v[3] = nrm.x; v[4] = nrm.y; v[5] = nrm.z;
    v[6] = col[0]; v[7] = col[1]; v[8] = col[2]; v[9] = col[3];
    v[10] = (float)(int)ci;
  }
  __syncthreads();
  const size_t left = n - c0, cells = left < 256 ? left : 256, nf = cells * 11;
  for (size_t i = threadIdx.x; i < nf; i += 256) out[(cut.rel ? (size_t)blockIdx.x * 256 : c0) * 11 + i] = stage[i];
}
__global__ void __launch_bounds__(256) k_bilinear(DevState s, const float* __restrict__ pos, int n, double* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  SerialPolicy pol(s);
  Sim<SerialPolicy> sim(s, s.soils, pol);
  out[i] = sim.height_bilinear(f2{pos[2 * i], pos[2 * i + 1]});
}

// single-operation kernels behind the point API (host-driven Layermap::add/remove etc.)
struct PointOp { int op; int x, y; double a; uint32_t type; float px, py; int k; };
__global__ void __launch_bounds__(64) k_point_op(DevState s, PointOp o, double* out) {
  SMX_LOAD_SOILS(sh)
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  SerialPolicy pol(s);
  Sim<SerialPolicy> sim(s, sh, pol);
  Frame st[MAX_FRAMES];
  int depth = 0;
  Water dummy;
  dummy.pos = {0.f, 0.f}; dummy.speed = {0.f, 0.f}; dummy.volume = 0.0; dummy.sediment = 0.0; dummy.evaprate = 0.0;
  dummy.spill = 0; dummy.ix = dummy.iy = 0; dummy.friction = 0.f; dummy.surface = dummy.contains = 0;
  switch (o.op) {
    case 0: sim.add(o.x, o.y, o.a, o.type); break;
    case 1: *out = sim.remove(o.x, o.y, o.a); break;
    case 2: if (o.k > 0) sim.template particle_cascade<1>(f2{o.px, o.py}); else sim.template particle_cascade<0>(f2{o.px, o.py}); break;
    case 3: sim.push_frame(st, depth, o.x, o.y, o.k); sim.water_drive(dummy, false, false, st, depth); break;
    case 4: sim.seep(o.x, o.y); break;
    case 5: *out = (double)pol.rand1(s); break;
  }
  sim.flush_counters();
  pol.finish(s);
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// roctx ranges per phase: resolved at run time, so the library does not depend on the profiler's marker library
struct RoctxApi {
  int (*push)(const char*) = nullptr; int (*pop)() = nullptr; bool tried = false;
  void load() {
    if (tried) return;
    tried = true;
    // only a marker library that is ALREADY in the process (a profiler preloads it; PyTorch links libroctx64): nothing is loaded for ranges
    for (const char* name : {"librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "libroctx64.so", "libroctx64.so.4"}) {
      if (void* h = dlopen(name, RTLD_NOW | RTLD_NOLOAD)) {
        push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA")); pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
        if (push && pop) return;
      }
    }
    push = nullptr; pop = nullptr;
  }
};
static RoctxApi g_roctx;
struct roctx_range {
  bool on;
  explicit roctx_range(const char* name) { g_roctx.load(); on = g_roctx.push != nullptr; if (on) g_roctx.push(name); }
  ~roctx_range() { if (on) g_roctx.pop(); }
};
// what a pair of HIP events brackets (smx_timing): a phase of the tick, or kernels inside one
enum Phase { PH_WATER = 0, PH_GRID, PH_WIND, PH_FREQ, PH_K_WATER, PH_K_WIND, PH_K_CLASSIFY, PH_K_GRIDTILES, PH_K_MAPFREQ, PH_K_TAIL, PH_K_EPOCHS, PH_K_GRID_CHILDREN, PH_K_FLOODS };
struct EvPair { hipEvent_t a, b; Phase phase; uint32_t launches; };
// the stream a context (or an ensemble) queues its work on, and the HIP-event brackets of its phases (smx_timing)
struct EventTimer {
  hipStream_t stream = nullptr;
  std::vector<EvPair> pending;
  std::vector<hipEvent_t> evpool;
  smx_timing timing{};
};

// smx_copy_state / smx_ensemble_fork: per-cell counts, their scan, the derived flag bytes, the totals, rocPRIM's temporary storage and
// the destination table (grown on demand, kept with the destination context or the ensemble)
struct ForkScratch {
  uint32_t* buried = nullptr; uint32_t* base = nullptr; uint8_t* flag = nullptr; size_t cells = 0;
  ForkTotals* tot = nullptr;
  void* temp = nullptr; size_t temp_bytes = 0;
  ForkDst* tab = nullptr; uint32_t tab_cap = 0;
};

// (the scratch of the terrain analyses -- smx_lakes, smx_drainage, smx_streams, smx_spill, smx_through, smx_hillslopes -- is
// AnalysisScratch, soil_scratch.h: one instance per analysis and owner)
using AnalysisScratch = AnalysisScratchOf<LakeMember>;

// smx_soil_totals / smx_ensemble_soil_totals / smx_soil_thickness / smx_cores: the member table, the error words, the records, the core
// lists with their counts and bases and rocPRIM's temporary storage (d_buf); the thickness planes or the section arrays (d_sec); the
// pinned source of the table and landing place of the small results (h_buf). Allocated at first use, grown on demand, kept.
struct StrataScratch {
  char* d_buf = nullptr; size_t buf_cap = 0;
  char* d_sec = nullptr; size_t sec_cap = 0;
  char* h_buf = nullptr; size_t h_cap = 0;
};

// smx_budget / smx_ensemble_budget: the analysis scratch of the chain on the base and of the records, and the 64-bit planes of the
// cells' changes (smx_budget only, allocated once a plane is asked for)
struct BudgetScratch {
  AnalysisScratch a;
  char* d_planes = nullptr; size_t planes_cap = 0;
};

// smx_set_analysis_launch: the most workgroups (grid.x) of the three families of launches that stride -- k_disp_flow; k_spill_relax,
// k_through_hops and k_through_exit; the strata readers -- and the grid.x the owner's last call gave each. A launch shape, never a result.
constexpr size_t STRATA_GRID = 8192;   // workgroups of one strata launch at most: 32 wavefronts per compute unit, the rest is strided
enum { LAUNCH_FLOW, LAUNCH_RELAX, LAUNCH_STRATA };
struct AnalysisLaunch {
  int32_t set[3] = {0, 0, 0};     // 0: the default
  uint32_t grid[3] = {0, 0, 0};   // 0: no launch of the family yet
  static uint32_t most(int which) { return which == LAUNCH_FLOW ? (uint32_t)DISP_FLOW_BLOCKS : which == LAUNCH_RELAX ? (uint32_t)SPILL_RELAX_BLOCKS : (uint32_t)STRATA_GRID; }
  uint32_t cap(int which) const { return set[which] ? (uint32_t)set[which] : most(which); }
};

struct smx_ctx : EventTimer {
  smx_config cfg;
  DevState d;
  DevMem mem;                         // owns every device and pinned buffer below, the views' included (soil_devmem.h); smx_destroy lists none of them
  bool own_stream = true;             // false: the stream is an ensemble's (smx_ensemble_add), which destroys it
  smx_ensemble* ensemble = nullptr;   // the ensemble that owns this context (smx_destroy refuses it), or null
  std::string err;
  size_t ncells = 0, nw0 = 0, nw1 = 0, nw2 = 0;
  size_t c_lo = 0, c_hi = 0, lcells = 0;   // cells HELD by this context: [c_lo, c_hi) = columns [x_lo, x_hi) (the whole map unless smx_create_strip)
  Sec* cells_alloc = nullptr; uint8_t* flags_alloc = nullptr; uint32_t* rhead_alloc = nullptr; uint32_t* cflag_alloc = nullptr; uint32_t* cstate_alloc = nullptr;   // unbiased allocations
  bool partial() const { return lcells != ncells; }
  SoilP* d_soils = nullptr;
  int nsoils = 0;
  double* d_scratch = nullptr;        // 1 double for point ops
  float* d_vtx = nullptr; float* d_vcol = nullptr; float* d_vtx1 = nullptr;   // smx_fill_vertices scratch (kept); d_vtx1: one 256-cell block (smx_fill_vertex_cut)
  float vcol_host[256 * 4]; int vcol_n = -1;          // the colour table on the device
  void* d_plane = nullptr; size_t plane_cap = 0;     // smx_read_heights / _surface / smx_normals scratch (kept)
  uint32_t spec_sub = 0, spec_maxnest = 0; bool spec_realloc = false;   // smx_set_spec_limits (0 = defaults)
  int water_generations = SMX_WATER_GENERATIONS;             // smx_set_water_generations (throughput engines: 8)
  int water_stagger = SMX_WATER_STAGGER;                     // smx_set_water_stagger: > 0 = the k generations of a water phase are BORN this many epochs apart inside ONE phase (relaxed engine)
  uint32_t stagger_phase_n = 0;                              // ... the top-level particle count of the phase that is running staggered (0: none)
  uint64_t spec_rounds = 0, spec_aborts = 0, spec_kills = 0, spec_fallbacks = 0, spec_executed = 0, spec_subphases_cut = 0, spec_serial_particles = 0;
  SpecShared sh{};                    // speculative engine buffers (allocated on first use)
  uint32_t spec_cap = 0;              // particles the buffers are sized for
  uint32_t* h_ctrl = nullptr;         // pinned host copy of the control block
  // batched engine (allocated on first use)
  BatchShared bs{};
  uint32_t batch_cap = 0;             // slots the particle buffers are sized for
  bool batch_wind_buf = false;
  uint32_t* d_draws = nullptr; uint32_t* h_draws = nullptr; uint32_t draws_cap = 0;
  BChild* d_kids = nullptr; uint32_t kids_cap = 0;
  unsigned long long* d_skeys[2] = {nullptr, nullptr}; uint32_t* d_sidx[2] = {nullptr, nullptr}; void* d_stemp = nullptr; size_t stemp_bytes = 0; uint32_t sort_cap = 0;   // children sort (device)
  uint32_t* h_bctrl = nullptr;
  int batch_dilate = 0;
  uint32_t relax_wind_min = 0xFFFFFFFFu;   // relaxed schedule: wind runs relaxed while more particles than this are running (default: never --
                                      // measured, profiles/r03_relaxed.md: the exclusive schedule's 8-32 steps per launch serve wind better)
  int relax_wind_steps = 4;           // ... taking up to this many steps per epoch (<= R_MAXSTEPS)
  int relax_water_steps = 1;          // relaxed water: steps per epoch (1 = an edit is visible to everybody's next step)
  uint32_t relax_tag = 0;             // epoch tags of the cascade flags (unique over the context's life)
  struct GridBar* d_gbar = nullptr;   // k_relax_epochs: the device-wide barrier of the persistent launch
  int mega_blocks = 0;                // ... its grid (0: not sized yet): co-resident workgroups, hipLaunchCooperativeKernel
  bool mega_off = false;              // ... the device refused a cooperative launch: the per-phase launches run instead (said once on stderr)
  int relax_persistent = -1, relax_tail_at = -1;   // smx_set_relax_launch (-1: the defaults / the environment's)
  uint32_t flood_launch_no = 0;       // k_relax_floods launches so far (every 7th is bracketed by HIP events)
  int relax_settle = -1;              // smx_set_relax_settle: -1 default, 0 k_relax_filter + k_relax_cascade_flow, 1 k_relax_settle where residency allows,
                                      // 2 k_relax_settle_floods (water epochs: settle and floods in one launch) where its residency allows, else as 1
  int settle_max_waves = 0, settle_lanes = 0;   // ... a cap on the resident wavefronts it may count on / cells per wavefront (0: the device's / the rule's)
  int settle_resident = 0;            // wavefronts of k_relax_settle the device holds at once (0: not asked yet, < 0: the occupancy query failed)
  int joined_resident = 0;            // ... and of k_relax_settle_floods
  unsigned long long* d_settle_crowded = nullptr;   // device counters: [0] cells that went through the waiting path of k_relax_settle(_floods),
                                                    // [1] floods that acted in k_relax_settle_floods, [2] those whose gate found a flagged cell
  uint64_t settle_epochs_fused = 0, settle_epochs_split = 0;   // dense per-phase epochs through k_relax_settle(_floods) / through the two launches
  uint64_t settle_epochs_joined = 0;  // ... of the fused ones: water epochs through k_relax_settle_floods
  uint32_t relax_cap = 0;             // slots the relaxed schedule's buffers are sized for
  int strips_n = 1, strips_a = 16, strips_b = 48;
  int own_x0 = 0, own_x1 = -1;        // strips on several devices: the columns this context owns (-1: to the map's edge)
  // step-wise generation state (smx_d_*)
  bool d_wind = false, d_first = true; uint32_t d_nslots = 0, d_epoch = 0, d_chunk = 0;
  uint32_t* d_contains = nullptr; uint32_t contains_cap = 0;
  uint8_t* d_xdata = nullptr; uint32_t* d_xoffs = nullptr; XCursor* d_xcur = nullptr;
  unsigned long long xdata_cap = 0; uint32_t xoffs_cap = 0;
  uint8_t* d_rdata = nullptr; uint32_t* d_roffs = nullptr; uint8_t* d_xpart = nullptr; uint8_t* d_rpart = nullptr; unsigned long long xpart_cap = 0;   // strips in the library
  struct StripState* strip = nullptr;
  uint32_t* d_tdone = nullptr; uint32_t* d_tpend[2] = {nullptr, nullptr}; uint32_t* d_tcount = nullptr; uint32_t* h_tcount = nullptr; void* d_tsort = nullptr; size_t tsort_bytes = 0; uint32_t tsort_cap = 0;   // grid pass: tile states, pending lists
  uint64_t batch_epochs = 0, batch_generations = 0, batch_children_lost = 0, grid_passes = 0;
  ForkScratch fork;                   // smx_copy_state into this context
  AnalysisScratch lakes, drain, streams, spill, through, hills, paths;   // smx_lakes, smx_drainage, smx_streams, smx_spill, smx_through, smx_hillslopes, smx_flowpaths: one each
  AnalysisScratch disp;                                                  // smx_dispersal
  AnalysisScratch catchments;                                            // smx_catchments
  AnalysisScratch horizons;                                              // smx_horizons
  AnalysisScratch proximity;                                             // smx_proximity
  StrataScratch strata;               // smx_soil_totals, smx_soil_thickness, smx_cores
  BudgetScratch budget;               // smx_budget of this context against a base
  AnalysisLaunch launch;              // smx_set_analysis_launch
};

// a failed HIP call: its text and the runtime's message go to the `err` of `obj` (a context, an ensemble, a lattice), the function returns -1
#define HIPCHK(obj, call)                                                                             \
  do {                                                                                                \
    hipError_t e_ = (call);                                                                           \
    if (e_ != hipSuccess) {                                                                           \
      (obj)->err = std::string(#call) + ": " + hipGetErrorString(e_);                                 \
      return -1;                                                                                      \
    }                                                                                                 \
  } while (0)

// a kernel template over the kind of particle: k<true> for wind, k<false> for water, same launch shape, same arguments
#define LAUNCH_WIND_WATER(wind, k, grid, block, st, ...)                                              \
  do {                                                                                                \
    if (wind) hipLaunchKernelGGL(k<true>, grid, block, 0, st, __VA_ARGS__);                           \
    else hipLaunchKernelGGL(k<false>, grid, block, 0, st, __VA_ARGS__);                               \
  } while (0)

static hipEvent_t ev_get(EventTimer* ctx) {
  if (!ctx->evpool.empty()) { hipEvent_t e = ctx->evpool.back(); ctx->evpool.pop_back(); return e; }
  hipEvent_t e; hipEventCreate(&e); return e;
}
static void drain_events(EventTimer* ctx) {
  for (EvPair& p : ctx->pending) {
    hipEventSynchronize(p.b);
    float ms = 0; hipEventElapsedTime(&ms, p.a, p.b);
    switch (p.phase) {
      case PH_WATER: ctx->timing.ms_water += ms; ctx->timing.launches_water++; break;
      case PH_GRID: ctx->timing.ms_grid += ms; ctx->timing.launches_grid++; break;
      case PH_WIND: ctx->timing.ms_wind += ms; ctx->timing.launches_wind++; break;
      case PH_FREQ: ctx->timing.ms_freq += ms; ctx->timing.launches_freq++; break;
      case PH_K_WATER: ctx->timing.ms_kernel_water += ms; ctx->timing.launches_kernel_water += p.launches; break;
      case PH_K_WIND: ctx->timing.ms_kernel_wind += ms; ctx->timing.launches_kernel_wind += p.launches; break;
      case PH_K_CLASSIFY: ctx->timing.ms_kernel_classify += ms; ctx->timing.launches_kernel_classify += p.launches; break;
      case PH_K_GRIDTILES: ctx->timing.ms_kernel_gridtiles += ms; ctx->timing.launches_kernel_gridtiles += p.launches; break;
      case PH_K_MAPFREQ: ctx->timing.ms_kernel_mapfreq += ms; ctx->timing.launches_kernel_mapfreq += p.launches; break;
      case PH_K_TAIL: ctx->timing.ms_kernel_tail += ms; ctx->timing.launches_kernel_tail++; ctx->timing.epochs_kernel_tail += p.launches; break;          // k_relax_tail (p.launches = its epochs)
      case PH_K_EPOCHS: ctx->timing.ms_kernel_epochs += ms; ctx->timing.launches_kernel_epochs++; ctx->timing.epochs_kernel_epochs += p.launches; break;   // k_relax_epochs
      case PH_K_GRID_CHILDREN: ctx->timing.ms_kernel_grid_children += ms; ctx->timing.launches_kernel_grid_children += p.launches; break;
      case PH_K_FLOODS: ctx->timing.ms_kernel_floods += ms; ctx->timing.launches_kernel_floods += p.launches; break;       // k_relax_floods (k_relax_settle_floods where it replaces it), the bracketed launches
    }
    ctx->evpool.push_back(p.a); ctx->evpool.push_back(p.b);
  }
  ctx->pending.clear();
}
struct PhaseTimer {
  EventTimer* ctx; EvPair p;
  PhaseTimer(EventTimer* c, Phase phase, uint32_t launches = 1) : ctx(c) { p.a = ev_get(c); p.b = ev_get(c); p.phase = phase; p.launches = launches; hipEventRecord(p.a, c->stream); }
  ~PhaseTimer() { hipEventRecord(p.b, ctx->stream); ctx->pending.push_back(p); if (ctx->pending.size() > 512) drain_events(ctx); }
};

static int reset_pool(smx_ctx* ctx) {
  // free stack holds every node index; cells empty; counters zero
  const uint64_t cap = ctx->cfg.pool_capacity;
  std::vector<uint32_t> fl(cap);
  for (uint64_t i = 0; i < cap; i++) fl[i] = (uint32_t)(cap - 1 - i);
  HIPCHK(ctx, hipMemcpyAsync(ctx->d.freelist, fl.data(), cap * 4, hipMemcpyHostToDevice, ctx->stream));
  uint32_t fc = (uint32_t)cap;
  HIPCHK(ctx, hipMemcpyAsync(ctx->d.free_count, &fc, 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return 0;
}

extern "C" {

const char* smx_last_error(smx_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

// stream: queue the context's work on this stream, which the caller owns (smx_ensemble_add); null = a stream of its own
// bare: leave cells, pool, free list, soil table and generator unwritten -- smx_ensemble_fork fills every one of them on the device
static int create_range(const smx_config* cfg, int x_lo, int x_hi, hipStream_t stream, smx_ctx** out, bool bare = false) {
  if (!cfg || !out || cfg->dimx <= 0 || cfg->dimy <= 0 || cfg->pool_capacity == 0 || cfg->pool_capacity >= 0x7FFFFFFFull) return -2;
  if (x_lo < 0 || x_hi > cfg->dimx || x_lo >= x_hi) return -2;
  smx_ctx* ctx = new smx_ctx();
  ctx->cfg = *cfg;
  *out = ctx;   // handed out even on failure so the caller can read smx_last_error(); smx_destroy() is safe
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { ctx->err = "no HIP device visible (the soilmx product path has no CPU fallback)"; return -3; }
  HIPCHK(ctx, hipSetDevice(cfg->device));
  if (stream) { ctx->stream = stream; ctx->own_stream = false; }
  else HIPCHK(ctx, hipStreamCreate(&ctx->stream));
  hipDeviceSetLimit(hipLimitStackSize, 16384);   // recursion depth of cascade<->nested particles is bounded by spill (water.h:34)
  const size_t n = (size_t)cfg->dimx * cfg->dimy;
  ctx->ncells = n;
  ctx->nw0 = (n + 63) >> 6; ctx->nw1 = (ctx->nw0 + 63) >> 6; ctx->nw2 = (ctx->nw1 + 63) >> 6;
  DevState& d = ctx->d;
  memset(&d, 0, sizeof(d));
  d.dimx = cfg->dimx; d.dimy = cfg->dimy; d.scale = cfg->scale; d.pool_capacity = cfg->pool_capacity;
  d.x_lo = x_lo; d.x_hi = x_hi;
  ctx->c_lo = (size_t)x_lo * cfg->dimy; ctx->c_hi = (size_t)x_hi * cfg->dimy; ctx->lcells = ctx->c_hi - ctx->c_lo;
  const size_t ln = ctx->lcells;
  DevMem& m = ctx->mem;
  HIPCHK(ctx, m.dev(ctx->cells_alloc, ln));
  d.cells = ctx->cells_alloc - ctx->c_lo;                     // global cell index, held range only (DevState::x_lo)
  HIPCHK(ctx, m.dev(d.pool, cfg->pool_capacity)); HIPCHK(ctx, m.dev(d.freelist, cfg->pool_capacity)); HIPCHK(ctx, m.dev(d.free_count, 16));
  HIPCHK(ctx, m.dev(ctx->flags_alloc, ln + 8));   // (whole 32-bit words: SerialPolicy::set_flag; c_lo is a multiple of 4 or the context holds everything)
  d.flags = ctx->flags_alloc - ctx->c_lo;
  HIPCHK(ctx, m.dev(d.wfreq, n)); HIPCHK(ctx, m.dev(d.wtrack, n)); HIPCHK(ctx, m.dev(d.windfreq, n));
  HIPCHK(ctx, m.dev(d.rnd, 1)); HIPCHK(ctx, m.dev(d.ctr, C_COUNT));
  HIPCHK(ctx, m.dev(d.active, ctx->nw0 + 64)); HIPCHK(ctx, m.dev(d.active1, ctx->nw1 + 64)); HIPCHK(ctx, m.dev(d.active2, ctx->nw2 + 64));
  HIPCHK(ctx, m.dev(ctx->d_scratch, 8)); HIPCHK(ctx, m.dev(ctx->d_soils, 256));
  d.soils = ctx->d_soils;
  HIPCHK(ctx, hipMemsetAsync(d.wfreq, 0, n * 4, ctx->stream)); HIPCHK(ctx, hipMemsetAsync(d.wtrack, 0, n * 4, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(d.windfreq, 0, n * 4, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(ctx->flags_alloc, 0, ln + 8, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(d.ctr, 0, C_COUNT * 8, ctx->stream));
  if (!bare) {   // all columns empty
    std::vector<Sec> empty(ln);
    for (size_t i = 0; i < ln; i++) { empty[i].size = 0; empty[i].floor = 0; empty[i].sat = 0; empty[i].type = EMPTY; empty[i].prev = NIL; }
    HIPCHK(ctx, hipMemcpyAsync(ctx->cells_alloc, empty.data(), ln * sizeof(Sec), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  }
  if (!bare) {
    if (reset_pool(ctx)) return -1;
    const smx_soil air = {0, 0, 0, 0, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};   // surface.h:43-49
    if (smx_set_soils(ctx, &air, 1)) return -1;
    if (smx_srand(ctx, 1)) return -1;
  }
  // (experiments; only a variable that is set overrides)
  if (env_str("SMX_RELAX_WIND_MIN")) ctx->relax_wind_min = (uint32_t)env_int("SMX_RELAX_WIND_MIN");
  if (const int v = (int)env_int("SMX_RELAX_WATER_STEPS"); v >= 1 && v <= R_MAXSTEPS) ctx->relax_water_steps = v;
  if (const int v = (int)env_int("SMX_RELAX_WIND_STEPS"); v >= 1 && v <= R_MAXSTEPS) ctx->relax_wind_steps = v;
  return 0;
}
// The switch table as text, one line per switch: "NAME=value default class" (value: what this process read; an unset switch without a
// default shows "-"). Needs neither a context nor a device.
int smx_switches(char* buf, uint64_t cap, uint64_t* needed) {
  static const char* const cls[] = {"neutral", "changes_results", "diagnostic"};
  std::string t;
  const EnvValues& ev = env_values();
  for (int i = 0; i < N_ENV_SWITCHES; i++) {
    const EnvSwitch& w = ENV_SWITCHES[i];
    t += w.name; t += '='; t += ev.v[i] ? ev.v[i] : "-"; t += ' '; t += w.dflt ? w.dflt : "-"; t += ' '; t += cls[w.cls]; t += '\n';
  }
  if (needed) *needed = (uint64_t)t.size() + 1u;
  if (!buf || cap < t.size() + 1u) return -2;
  memcpy(buf, t.c_str(), t.size() + 1u);
  return 0;
}
int smx_create(const smx_config* cfg, smx_ctx** out) { return create_range(cfg, 0, cfg ? cfg->dimx : 0, nullptr, out); }
// A context that HOLDS only the columns [x_lo, x_hi) of a dimx x dimy map -- a column strip and its halo (smx_strips_*): cells, flags
// and the engines' per-cell planes are allocated for that range, per-rank memory follows the strip. x_lo*dimy must be a multiple of 64.
int smx_create_strip(const smx_config* cfg, int32_t x_lo, int32_t x_hi, smx_ctx** out) {
  if (cfg && ((size_t)x_lo * (size_t)cfg->dimy) % 64 != 0) return -2;
  return create_range(cfg, x_lo, x_hi, nullptr, out);
}
#define FULLMAP(what)                                                                                                 \
  if (ctx->partial()) { ctx->err = what ": not available on a strip context (smx_create_strip): it holds only a part of the map"; return -2; }

static void strips_free(smx_ctx* ctx);
void smx_destroy(smx_ctx* ctx) {
  if (!ctx) return;
  if (ctx->ensemble) { ctx->err = "smx_destroy: this context is a member of an ensemble; smx_ensemble_destroy frees it (nothing was freed)"; return; }
  strips_free(ctx);
  if (ctx->stream) hipStreamSynchronize(ctx->stream);
  if (flood_prof()) {
    unsigned long long h[72];
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_flood_prof), sizeof(h)) == hipSuccess && h[64]) {
      fprintf(stderr, "[soilmx] k_relax_floods: %llu floods acted, mean %.1f us; %llu listed floods waited (did not hold their tiles). duration bucket (us): floods, nested steps per flood\n", h[64], 0.01 * (double)h[65] / (double)h[64], h[66]);
      for (int b = 0; b < 32; b++) if (h[b]) fprintf(stderr, "   [%8.1f, %8.1f) %9llu  %7.1f\n", 0.01 * (double)(1ull << b), 0.01 * (double)(2ull << b), h[b], (double)h[32 + b] / (double)h[b]);
    }
  }
  if (flood_prof()) {
    unsigned long long h[104];
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_tile_prof), sizeof(h)) == hipSuccess && h[64]) {
      fprintf(stderr, "[soilmx] k_grid_tiles_flow: %llu tiles swept, mean %.1f us, longest %.1f us; waiting for earlier colours: mean %.1f us per tile. sweep time bucket (us): tiles, active cells per tile, nested steps per tile, us per active cell\n",
              h[64], 0.01 * (double)h[65] / (double)h[64], 0.01 * (double)h[67], 0.01 * (double)h[66] / (double)h[64]);
      for (int b = 0; b < 32; b++) if (h[b]) fprintf(stderr, "   [%8.1f, %8.1f) %9llu  %6.1f  %7.1f  %7.1f\n", 0.01 * (double)(1ull << b), 0.01 * (double)(2ull << b), h[b], (double)h[32 + b] / (double)h[b],
                                                     (double)h[72 + b] / (double)h[b], h[32 + b] ? 0.01 * 1.5 * (double)(1ull << b) * (double)h[b] / (double)h[32 + b] : 0.0);
    }
  }
#ifdef SMX_PROF_FLOOD
  {
    unsigned long long h[32];
    static const char* nm[10] = {"prelude: add sediment", "prelude: Particle::cascade", "prelude: add water", "prelude: seep", "push_frame (9 views, sort, mask)", "neighbour: nothing to move",
                                 "neighbour: partial transfer", "neighbour: nested particle spawned", "run_nested (a nested particle's steps)", "grid tile: seep of an active cell"};
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_sect), sizeof(h)) == hipSuccess)
      for (int k = 0; k < 10; k++) if (h[2 * k + 1]) fprintf(stderr, "[soilmx] section %-40s %10llu x %7.2f us = %9.1f ms\n", nm[k], h[2 * k + 1], 0.01 * (double)h[2 * k] / (double)h[2 * k + 1], 1e-5 * (double)h[2 * k]);
  }
#endif
  if (ctx->d_gbar && (relax_mega_flags() & 2u)) {   // (experiments: where an epoch of k_relax_epochs goes, workgroup 0's clock)
    GridBar hb; if (hipMemcpy(&hb, ctx->d_gbar, sizeof(hb), hipMemcpyDeviceToHost) == hipSuccess && hb.prof[10]) {
      static const char* nm[10] = {"step", "sync", "apply", "sync", "filter", "sync", "colours", "sync", "floods", "sync"};
      fprintf(stderr, "[soilmx] k_relax_epochs, %llu epochs, microseconds per epoch (100 MHz clock):", hb.prof[10]);
      for (int k = 0; k < 10; k++) fprintf(stderr, " %s %.1f", nm[k], 0.01 * (double)hb.prof[k] / (double)hb.prof[10]);
      fprintf(stderr, "\n");
    }
  }
  drain_events(ctx);
  for (hipEvent_t e : ctx->evpool) hipEventDestroy(e);
  ctx->mem.clear();
  if (ctx->stream && ctx->own_stream) hipStreamDestroy(ctx->stream);
  delete ctx;
}

int smx_set_soils(smx_ctx* ctx, const smx_soil* soils, int32_t n) {
  if (n <= 0 || n > 256) { ctx->err = "smx_set_soils: 1..256 soils"; return -2; }
  for (int i = 0; i < n; i++)
    if (soils[i].transports >= (uint32_t)n || soils[i].erodes >= (uint32_t)n || soils[i].cascades >= (uint32_t)n || soils[i].abrades >= (uint32_t)n) {
      ctx->err = "smx_set_soils: soil index out of range"; return -2;
    }
  HIPCHK(ctx, hipMemcpyAsync(ctx->d_soils, soils, n * sizeof(SoilP), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  ctx->nsoils = n; ctx->d.nsoils = n;
  return 0;
}
int smx_set_scale(smx_ctx* ctx, int32_t scale) { ctx->d.scale = scale; ctx->cfg.scale = scale; return 0; }
int smx_set_engine(smx_ctx* ctx, int32_t engine) { ctx->cfg.engine = engine; return 0; }
// speculative engine: top-level particles per sub-phase / nested-particle slots of a sub-phase (0 = default: 4096 / 8192). Tests use
// small values to drive the sub-phase hand-over; results never depend on them.
int smx_set_spec_limits(smx_ctx* ctx, uint32_t particles_per_subphase, uint32_t nested_slots) {
  if (nested_slots && (nested_slots < 128u || nested_slots > 60000u)) { ctx->err = "smx_set_spec_limits: nested_slots must lie in [128, 60000]"; return -2; }
  ctx->spec_sub = particles_per_subphase ? std::max(64u, particles_per_subphase) : 0u; ctx->spec_maxnest = nested_slots; ctx->spec_realloc = true;
  return 0;
}
// Column strips need every reservation to fit between the inset and the seam half-width (soil_batch.h BStrips), or a particle
// near a boundary is eligible in neither kind of chunk and the phase never ends. Widest reservations of batch_schedule:
// water 3 tiles of 4 cells, wind 3 tiles of 4 / 2 tiles of 8, each plus the margin on both sides.
static bool batch_strips_fit(int dilate, int inset, int seam_halfwidth) {
  const int dw = dilate > 0 ? dilate : 0, dd = dilate > 1 ? dilate : 1;
  const int w_water = (3 + 2 * dw) * 4, w_wind = (3 + 2 * dd) * 4, w_tail = (2 + 2 * dd) * 8;
  return std::max(w_water, std::max(w_wind, w_tail)) <= seam_halfwidth - inset;
}
int smx_set_batch_dilate(smx_ctx* ctx, int32_t tiles) {
  if (tiles < 0) tiles = 0;
  if (ctx->strips_n > 1 && !batch_strips_fit(tiles, ctx->strips_a, ctx->strips_b)) {
    ctx->err = "smx_set_batch_dilate: reservations with this margin do not fit the seam zones of the column strips"; return -2;
  }
  ctx->batch_dilate = tiles;
  return 0;
}
int smx_get_water_generations(smx_ctx* ctx, int32_t* k) { if (!k) return -2; *k = ctx->water_generations; return 0; }
int smx_set_water_stagger(smx_ctx* ctx, int32_t gap_epochs) {
  if (gap_epochs < 0 || gap_epochs > 65536) { ctx->err = "smx_set_water_stagger: 0 (consecutive generations) .. 65536 epochs"; return -2; }
  ctx->water_stagger = gap_epochs;
  return 0;
}
int smx_get_water_stagger(smx_ctx* ctx, int32_t* gap_epochs) { if (!gap_epochs) return -2; *gap_epochs = ctx->water_stagger; return 0; }
int smx_set_water_generations(smx_ctx* ctx, int32_t k) {
  if (k < 1 || k > 64) { ctx->err = "smx_set_water_generations: 1..64"; return -2; }
  ctx->water_generations = k;
  return 0;
}
int smx_set_grid_interleave(smx_ctx* ctx, int32_t) {
  ctx->err = "smx_set_grid_interleave: removed in round 5 (nested particles run inside their parent's region; the grid pass has no interleave any more)";
  return -2;
}
int smx_set_relax_launch(smx_ctx* ctx, int32_t persistent, int32_t tail_at) {
  if (tail_at > 256) { ctx->err = "smx_set_relax_launch: the tail kernel holds at most 256 particles (one per thread of its workgroup)"; return -2; }
  ctx->relax_persistent = persistent < 0 ? -1 : (persistent ? 1 : 0); ctx->relax_tail_at = tail_at < 0 ? -1 : tail_at;
  return 0;
}
int smx_set_relax_settle(smx_ctx* ctx, int32_t mode, int32_t max_waves, int32_t lanes) {
  if (mode > 2 || lanes > 64) { ctx->err = "smx_set_relax_settle: mode -1, 0, 1 or 2; at most 64 cells per wavefront"; return -2; }
  ctx->relax_settle = mode < 0 ? -1 : mode; ctx->settle_max_waves = max_waves < 0 ? 0 : max_waves; ctx->settle_lanes = lanes < 0 ? 0 : lanes;
  return 0;
}
int smx_get_relax_settle(smx_ctx* ctx, uint64_t* crowded_cells, uint64_t* epochs_fused, uint64_t* epochs_split) {
  unsigned long long nc = 0;
  if (ctx->d_settle_crowded) {
    HIPCHK(ctx, hipMemcpyAsync(&nc, ctx->d_settle_crowded, sizeof(nc), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  }
  if (crowded_cells) *crowded_cells = nc;
  if (epochs_fused) *epochs_fused = ctx->settle_epochs_fused;
  if (epochs_split) *epochs_split = ctx->settle_epochs_split;
  return 0;
}
int smx_get_relax_flood_flow(smx_ctx* ctx, uint64_t* epochs_joined, uint64_t* floods_acted, uint64_t* floods_gated) {
  unsigned long long nf[2] = {0, 0};
  if (ctx->d_settle_crowded) {
    HIPCHK(ctx, hipMemcpyAsync(nf, ctx->d_settle_crowded + 1, sizeof(nf), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  }
  if (epochs_joined) *epochs_joined = ctx->settle_epochs_joined;
  if (floods_acted) *floods_acted = nf[0];
  if (floods_gated) *floods_gated = nf[1];
  return 0;
}
int smx_set_relax_wind(smx_ctx* ctx, uint32_t min_running, int32_t steps_per_epoch) {
  if (steps_per_epoch < 1 || steps_per_epoch > R_MAXSTEPS) { ctx->err = "smx_set_relax_wind: 1..8 steps per epoch"; return -2; }
  ctx->relax_wind_min = min_running; ctx->relax_wind_steps = steps_per_epoch;
  return 0;
}
int smx_set_batch_strips(smx_ctx* ctx, int32_t nstrips, int32_t inset, int32_t seam_halfwidth) {
  if (nstrips < 1 || nstrips > 8 || inset < 0 || seam_halfwidth - inset < 32) { ctx->err = "smx_set_batch_strips: 1..8 strips, seam_halfwidth - inset >= 32"; return -2; }
  if (nstrips > 1 && ctx->cfg.dimx / nstrips < 2 * seam_halfwidth + 16) { ctx->err = "smx_set_batch_strips: strips narrower than two seam zones"; return -2; }
  if (nstrips > 1 && !batch_strips_fit(ctx->batch_dilate, inset, seam_halfwidth)) {
    ctx->err = "smx_set_batch_strips: the reservations of the current margin (smx_set_batch_dilate) do not fit seam_halfwidth - inset"; return -2;
  }
  ctx->strips_n = nstrips; ctx->strips_a = inset; ctx->strips_b = seam_halfwidth;
  return 0;
}
int smx_get_batch_stats(smx_ctx* ctx, uint64_t* epochs, uint64_t* generations, uint64_t* children_lost) {
  if (epochs) *epochs = ctx->batch_epochs;
  if (generations) *generations = ctx->batch_generations;
  if (children_lost) *children_lost = ctx->batch_children_lost;
  return 0;
}
void* smx_stream(smx_ctx* ctx) { return (void*)ctx->stream; }

int smx_srand(smx_ctx* ctx, uint32_t seed) {   // glibc srandom_r, TYPE_3 (stdlib/random_r.c)
  RandState r;
  rand_seed(r, seed);
  HIPCHK(ctx, hipMemcpyAsync(ctx->d.rnd, &r, sizeof(r), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return 0;
}
int smx_rand(smx_ctx* ctx, int32_t* out) {
  PointOp o{}; o.op = 5;
  hipLaunchKernelGGL(k_point_op, dim3(1), dim3(64), 0, ctx->stream, ctx->d, o, ctx->d_scratch);
  double v = 0;
  HIPCHK(ctx, hipMemcpyAsync(&v, ctx->d_scratch, 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  *out = (int32_t)v;
  return 0;
}

int smx_get_rand_state(smx_ctx* ctx, uint32_t ring31[31], uint32_t* idx, uint64_t* calls) {
  RandState r;
  HIPCHK(ctx, hipMemcpyAsync(&r, ctx->d.rnd, sizeof(r), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  memcpy(ring31, r.ring, sizeof(r.ring)); if (idx) *idx = r.idx; if (calls) *calls = r.calls;
  return 0;
}
int smx_set_rand_state(smx_ctx* ctx, const uint32_t ring31[31], uint32_t idx, uint64_t calls) {
  RandState r; memcpy(r.ring, ring31, sizeof(r.ring)); r.idx = idx; r.calls = calls;
  HIPCHK(ctx, hipMemcpyAsync(ctx->d.rnd, &r, sizeof(r), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return 0;
}
int smx_rand_advance(smx_ctx* ctx, uint64_t ndraws) {
  RandState r;
  HIPCHK(ctx, hipMemcpyAsync(&r, ctx->d.rnd, sizeof(r), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  rand_skip(r, ndraws);
  r.calls += ndraws;
  HIPCHK(ctx, hipMemcpyAsync(ctx->d.rnd, &r, sizeof(r), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return 0;
}

int smx_initialize(smx_ctx* ctx, int32_t seed, const smx_layer* layers, int32_t nlayers) {
  if (nlayers < 0 || nlayers > MAX_LAYERS) { ctx->err = "smx_initialize: too many layers"; return -2; }
  // Every (cell, layer) pair can become a section. The reference prints "Memory Pool Out-Of-Elements" and silently
  // drops the rest of the terrain (layermap.h:92-95,233); a device-parallel build cannot reproduce WHICH sections it
  // drops, so a pool that cannot hold the worst case is refused up front instead of producing a different map.
  if ((uint64_t)ctx->lcells * (uint64_t)(nlayers > 0 ? nlayers : 1) > ctx->cfg.pool_capacity) {
    ctx->err = "smx_initialize: pool_capacity < cells * layers (the reference's POOLSIZE would overflow during Layermap::initialize)";
    return -4;
  }
  if (reset_pool(ctx)) return -1;
  HIPCHK(ctx, hipMemsetAsync(ctx->d.ctr + C_LIVE_SECTIONS, 0, 8, ctx->stream));
  LayersDev L; L.n = nlayers;
  const int MAXSEED = 10000;
  for (int l = 0; l < nlayers; l++) {
    const float f = (float)l / (float)nlayers;                    // layermap.h:183-184
    const int Z = (int)((float)seed + f * (float)MAXSEED);
    LayerDev& d = L.l[l];
    d.type = layers[l].type; d.min = layers[l].min; d.bias = layers[l].bias; d.scale = layers[l].scale;
    d.noise.seed = 1337; d.noise.octaves = (int)layers[l].octaves; d.noise.frequency = layers[l].frequency;
    d.noise.lacunarity = layers[l].lacunarity; d.noise.gain = layers[l].gain;
    float g = d.noise.gain < 0 ? -d.noise.gain : d.noise.gain;    // CalculateFractalBounding (FastNoiseLite.h:473-484)
    float amp = g, ampFractal = 1.0f;
    for (int i = 1; i < d.noise.octaves; i++) { ampFractal += amp; amp *= g; }
    d.noise.bounding = 1 / ampFractal;
    d.z = (float)(Z % MAXSEED) / 1.0f;                            // vec3(i,j,Z%MAXSEED)/vec3(dim.x,dim.y,1) (:191)
  }
  const unsigned nb = (unsigned)((ctx->lcells + 255) / 256);
  hipLaunchKernelGGL(k_init_terrain, dim3(nb), dim3(256), 0, ctx->stream, ctx->d, L);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return 0;
}

int smx_import_columns(smx_ctx* ctx, const uint32_t* count, const uint32_t* type, const double* size,
                       const double* floor, const double* sat) {
  const size_t n = ctx->ncells, lo = ctx->c_lo, hi = ctx->c_hi, ln = ctx->lcells;   // (the arrays describe the WHOLE map; a strip context keeps its range)
  const uint64_t cap = ctx->cfg.pool_capacity;
  std::vector<Sec> cells(ln);
  std::vector<uint8_t> flags(ln + 8, 0);
  std::vector<Sec> pool;
  size_t off = 0, total = 0;
  for (size_t c = lo; c < hi; c++) total += count[c];
  if (total > cap) { ctx->err = "smx_import_columns: more sections than pool_capacity"; return -4; }
  pool.reserve(total > ln ? total - ln + 1 : 1);
  for (size_t c = 0; c < n; c++) {
    const uint32_t k = count[c];
    if (c < lo || c >= hi) { off += k; continue; }
    Sec cell; cell.size = 0; cell.floor = 0; cell.sat = 0; cell.type = EMPTY; cell.prev = NIL;
    uint32_t pv = NIL;
    for (uint32_t j = 0; j < k; j++, off++) {
      Sec r; r.size = size[off]; r.floor = floor[off]; r.sat = sat[off]; r.type = type[off]; r.prev = pv;
      if (r.sat != 0.0) flags[c - lo] |= F_SAT;
      if (j == k - 1) cell = r;
      else { pv = (uint32_t)pool.size(); pool.push_back(r); }
    }
    if (cell.type == AIR) flags[c - lo] |= F_AIR;
    cells[c - lo] = cell;
  }
  // node i of `pool` lives at pool index i; the free stack holds the remaining indices
  const uint64_t used = pool.size();
  std::vector<uint32_t> fl(cap);
  uint64_t nf = 0;
  for (uint64_t i = cap; i-- > used;) fl[nf++] = (uint32_t)i;
  uint32_t fc = (uint32_t)nf;
  unsigned long long live = total;
  HIPCHK(ctx, hipMemcpyAsync(ctx->cells_alloc, cells.data(), ln * sizeof(Sec), hipMemcpyHostToDevice, ctx->stream));
  if (used) HIPCHK(ctx, hipMemcpyAsync(ctx->d.pool, pool.data(), used * sizeof(Sec), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ctx->d.freelist, fl.data(), cap * 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ctx->d.free_count, &fc, 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ctx->flags_alloc, flags.data(), ln, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ctx->d.ctr + C_LIVE_SECTIONS, &live, 8, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return 0;
}

int smx_import_frequency(smx_ctx* ctx, const float* wfreq, const float* wtrack, const float* windfreq) {
  const size_t n = ctx->ncells;
  if (wfreq) HIPCHK(ctx, hipMemcpyAsync(ctx->d.wfreq, wfreq, n * 4, hipMemcpyHostToDevice, ctx->stream));
  if (wtrack) HIPCHK(ctx, hipMemcpyAsync(ctx->d.wtrack, wtrack, n * 4, hipMemcpyHostToDevice, ctx->stream));
  if (windfreq) HIPCHK(ctx, hipMemcpyAsync(ctx->d.windfreq, windfreq, n * 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return 0;
}

int smx_num_sections(smx_ctx* ctx, uint64_t* out) {
  unsigned long long live = 0;
  HIPCHK(ctx, hipMemcpyAsync(&live, ctx->d.ctr + C_LIVE_SECTIONS, 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  *out = live;
  return 0;
}

int smx_export_columns(smx_ctx* ctx, uint32_t* count, uint32_t* type, double* size, double* floor, double* sat) {
  const size_t n = ctx->ncells, lo = ctx->c_lo, hi = ctx->c_hi, ln = ctx->lcells;   // (a strip context reports empty columns outside its range)
  const uint64_t cap = ctx->cfg.pool_capacity;
  std::vector<Sec> cells(ln), pool(cap);
  HIPCHK(ctx, hipMemcpyAsync(cells.data(), ctx->cells_alloc, ln * sizeof(Sec), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(pool.data(), ctx->d.pool, cap * sizeof(Sec), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  size_t off = 0;
  std::vector<const Sec*> col;
  for (size_t c = 0; c < n; c++) {
    col.clear();
    if (c < lo || c >= hi) { count[c] = 0; continue; }
    if (cells[c - lo].type != EMPTY) {
      const Sec* t = &cells[c - lo];
      while (true) {
        col.push_back(t);
        if (t->prev == NIL) break;
        if (t->prev >= cap || col.size() > cap) { ctx->err = "smx_export_columns: corrupt section chain"; return -5; }
        t = &pool[t->prev];
      }
    }
    count[c] = (uint32_t)col.size();
    for (size_t k = col.size(); k-- > 0; off++) {
      type[off] = col[k]->type; size[off] = col[k]->size; floor[off] = col[k]->floor; sat[off] = col[k]->sat;
    }
  }
  return 0;
}

struct SnapHdr { char magic[8]; int32_t dimx, dimy, scale, nsoils; uint64_t ncells, nsec, rand_calls, pool_free, reserved; };
static_assert(sizeof(SnapHdr) == 64, "snapshot header");
struct RandTrailer { char magic[8]; uint32_t ring[31]; uint32_t idx; uint64_t calls; };
int smx_save(smx_ctx* ctx, const char* path) {
  FULLMAP("smx_save")
  const size_t n = ctx->ncells;
  uint64_t ns = 0;
  if (smx_num_sections(ctx, &ns)) return -1;
  std::vector<uint32_t> count(n), type(ns);
  std::vector<double> size(ns), floor(ns), sat(ns);
  std::vector<float> wf(n), wt(n), wi(n);
  if (smx_export_columns(ctx, count.data(), type.data(), size.data(), floor.data(), sat.data())) return -1;
  if (smx_read_frequency(ctx, wf.data(), wt.data(), wi.data())) return -1;
  // the per-column flag plane (bit1 = "this column has held a saturation", sticky): context state the column records do not
  // carry; the throughput engines fix the active set of their grid pass from it, so a resume without it can differ
  std::vector<uint8_t> fl(n);
  HIPCHK(ctx, hipMemcpyAsync(fl.data(), ctx->d.flags, n, hipMemcpyDeviceToHost, ctx->stream));
  RandTrailer tr; memcpy(tr.magic, "SMXRAND1", 8);
  RandState r;
  HIPCHK(ctx, hipMemcpyAsync(&r, ctx->d.rnd, sizeof(r), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  memcpy(tr.ring, r.ring, sizeof(tr.ring)); tr.idx = r.idx; tr.calls = r.calls;
  SnapHdr h; memset(&h, 0, sizeof(h)); memcpy(h.magic, "SMXSNAP1", 8);
  h.dimx = ctx->cfg.dimx; h.dimy = ctx->cfg.dimy; h.scale = ctx->d.scale; h.nsoils = ctx->nsoils; h.ncells = n; h.nsec = ns;
  h.rand_calls = r.calls; h.pool_free = ctx->cfg.pool_capacity - ns;
  FILE* f = fopen(path, "wb");
  if (!f) { ctx->err = std::string("smx_save: cannot open ") + path; return -7; }
  bool ok = fwrite(&h, sizeof(h), 1, f) == 1;
  ok = ok && fwrite(count.data(), 4, n, f) == n && fwrite(type.data(), 4, ns, f) == ns && fwrite(size.data(), 8, ns, f) == ns &&
       fwrite(floor.data(), 8, ns, f) == ns && fwrite(sat.data(), 8, ns, f) == ns && fwrite(wf.data(), 4, n, f) == n &&
       fwrite(wt.data(), 4, n, f) == n && fwrite(wi.data(), 4, n, f) == n && fwrite(&tr, sizeof(tr), 1, f) == 1 &&
       fwrite("SMXFLAG1", 1, 8, f) == 8 && fwrite(fl.data(), 1, n, f) == n;
  ok = (fclose(f) == 0) && ok;
  if (!ok) { ctx->err = std::string("smx_save: short write to ") + path; return -7; }
  return 0;
}
int smx_load(smx_ctx* ctx, const char* path) {
  FULLMAP("smx_load")
  FILE* f = fopen(path, "rb");
  if (!f) { ctx->err = std::string("smx_load: cannot open ") + path; return -7; }
  SnapHdr h;
  if (fread(&h, sizeof(h), 1, f) != 1 || memcmp(h.magic, "SMXSNAP1", 8) != 0) { fclose(f); ctx->err = "smx_load: not a soilmx snapshot"; return -7; }
  if (h.dimx != ctx->cfg.dimx || h.dimy != ctx->cfg.dimy || h.ncells != ctx->ncells) { fclose(f); ctx->err = "smx_load: snapshot dimensions differ from the context's"; return -2; }
  const size_t n = ctx->ncells; const uint64_t ns = h.nsec;
  // the header is untrusted input: the section count sizes five arrays below and every later index
  {
    struct stat sb;
    const uint64_t need = sizeof(SnapHdr) + 4ull * n + 28ull * ns + 12ull * n;
    if (ns > ctx->cfg.pool_capacity) { fclose(f); ctx->err = "smx_load: the snapshot holds more sections than pool_capacity"; return -4; }
    if (fstat(fileno(f), &sb) != 0 || (uint64_t)sb.st_size < need) { fclose(f); ctx->err = "smx_load: truncated snapshot (shorter than its header promises)"; return -7; }
  }
  std::vector<uint32_t> count(n), type(ns);
  std::vector<double> size(ns), floor(ns), sat(ns);
  std::vector<float> wf(n), wt(n), wi(n);
  bool ok = fread(count.data(), 4, n, f) == n && fread(type.data(), 4, ns, f) == ns && fread(size.data(), 8, ns, f) == ns &&
            fread(floor.data(), 8, ns, f) == ns && fread(sat.data(), 8, ns, f) == ns && fread(wf.data(), 4, n, f) == n &&
            fread(wt.data(), 4, n, f) == n && fread(wi.data(), 4, n, f) == n;
  RandTrailer tr; const bool have_rand = ok && fread(&tr, sizeof(tr), 1, f) == 1 && memcmp(tr.magic, "SMXRAND1", 8) == 0;
  std::vector<uint8_t> fl; char fmagic[8];
  if (have_rand && fread(fmagic, 1, 8, f) == 8 && memcmp(fmagic, "SMXFLAG1", 8) == 0) { fl.resize(n); if (fread(fl.data(), 1, n, f) != n) fl.clear(); }
  fclose(f);
  if (!ok) { ctx->err = "smx_load: truncated snapshot"; return -7; }
  {
    uint64_t total = 0;
    for (size_t c = 0; c < n; c++) total += count[c];
    if (total != ns) { ctx->err = "smx_load: per-cell section counts do not add up to the header's section count"; return -2; }
    for (uint64_t i = 0; i < ns; i++)
      if (type[i] >= (uint32_t)ctx->nsoils) { ctx->err = "smx_load: a section's soil type is outside the context's soil table (smx_set_soils first)"; return -2; }
  }
  if (smx_import_columns(ctx, count.data(), type.data(), size.data(), floor.data(), sat.data())) return -1;
  if (smx_import_frequency(ctx, wf.data(), wt.data(), wi.data())) return -1;
  if (!fl.empty()) {                                         // the sticky bit on top of what the import derived from the columns
    std::vector<uint8_t> cur(n);
    HIPCHK(ctx, hipMemcpyAsync(cur.data(), ctx->d.flags, n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t c = 0; c < n; c++) cur[c] |= (uint8_t)(fl[c] & F_SAT);
    HIPCHK(ctx, hipMemcpyAsync(ctx->d.flags, cur.data(), n, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  }
  if (have_rand) {
    RandState r; memcpy(r.ring, tr.ring, sizeof(r.ring)); r.idx = tr.idx; r.calls = tr.calls;
    HIPCHK(ctx, hipMemcpyAsync(ctx->d.rnd, &r, sizeof(r), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  }
  ctx->d.scale = h.scale; ctx->cfg.scale = h.scale;
  return have_rand ? 0 : 1;   /* 1: state restored, but the file carries no generator state (a bare snapshot): re-seed it yourself */
}

int smx_read_frequency(smx_ctx* ctx, float* wfreq, float* wtrack, float* windfreq) {
  const size_t n = ctx->ncells;
  if (wfreq) HIPCHK(ctx, hipMemcpyAsync(wfreq, ctx->d.wfreq, n * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (wtrack) HIPCHK(ctx, hipMemcpyAsync(wtrack, ctx->d.wtrack, n * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (windfreq) HIPCHK(ctx, hipMemcpyAsync(windfreq, ctx->d.windfreq, n * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return 0;
}

static int read_plane(smx_ctx* ctx, void* host, size_t bytes, int which) {   // (a strip context fills its range; the rest of `host` reads 0)
  if (which == 2) { FULLMAP("smx_normals") }
  HIPCHK(ctx, ctx->mem.grow(ctx->d_plane, ctx->plane_cap, bytes, bytes));
  void* tmp = ctx->d_plane;
  const unsigned nb = (unsigned)((ctx->lcells + 255) / 256);
  const size_t el = which == 0 ? 8 : (which == 1 ? 4 : 12);
  if (which == 0) hipLaunchKernelGGL(k_heights, dim3(nb), dim3(256), 0, ctx->stream, ctx->d, (double*)tmp);
  else if (which == 1) hipLaunchKernelGGL(k_surface, dim3(nb), dim3(256), 0, ctx->stream, ctx->d, (uint32_t*)tmp);
  else hipLaunchKernelGGL(k_normals, dim3(nb), dim3(256), 0, ctx->stream, ctx->d, (float*)tmp);
  if (ctx->partial()) memset(host, 0, bytes);
  hipError_t e = hipMemcpyAsync((char*)host + ctx->c_lo * el, tmp, ctx->lcells * el, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) { ctx->err = hipGetErrorString(e); return -1; }
  return 0;
}
int smx_read_heights(smx_ctx* ctx, double* out) { return read_plane(ctx, out, ctx->ncells * 8, 0); }
int smx_read_surface(smx_ctx* ctx, uint32_t* out) { return read_plane(ctx, out, ctx->ncells * 4, 1); }
int smx_normals(smx_ctx* ctx, float* out3) { return read_plane(ctx, out3, ctx->ncells * 12, 2); }

static int fill_vertices(smx_ctx* ctx, const float* colors4, int32_t ncolors, void* out_vertices44, VCut cut, long long one_cell = -1) {
  FULLMAP("smx_fill_vertices")
  if (!colors4 || ncolors <= 0 || !out_vertices44) { ctx->err = "smx_fill_vertices: colors4/out must be given"; return -2; }
  const size_t bytes = ctx->ncells * 44;
  if (!ctx->d_vcol) { HIPCHK(ctx, ctx->mem.dev(ctx->d_vcol, 256 * 4)); ctx->vcol_n = -1; }
  if (ncolors > 256) ncolors = 256;
  if (ctx->vcol_n != ncolors || memcmp(ctx->vcol_host, colors4, (size_t)ncolors * 16) != 0) {   // (the colour table rarely changes: one upload, not one per call)
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_vcol, colors4, (size_t)ncolors * 16, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(ctx->vcol_host, colors4, (size_t)ncolors * 16); ctx->vcol_n = ncolors;
  }
  if (one_cell >= 0) {                                        // one column (Layermap::update(ivec2, ...)): the 256-cell block that holds it, into a block-sized scratch
    if (!ctx->d_vtx1) HIPCHK(ctx, ctx->mem.dev(ctx->d_vtx1, 256 * 11));
    cut.block0 = (unsigned)((size_t)one_cell / 256); cut.rel = 1u;
    hipLaunchKernelGGL(k_fill_vertices, dim3(1), dim3(256), 0, ctx->stream, ctx->d, ctx->d_vcol, (uint32_t)ncolors, ctx->d_vtx1, cut);
    HIPCHK(ctx, hipMemcpyAsync(out_vertices44, reinterpret_cast<const char*>(ctx->d_vtx1) + ((size_t)one_cell % 256) * 44, 44, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
  }
  if (!ctx->d_vtx) {                                        // whole-map scratch kept for the context's lifetime (738 MB at 4096^2)
    if (ctx->mem.dev(ctx->d_vtx, ctx->ncells * 11) != hipSuccess) { ctx->err = "smx_fill_vertices: out of device memory"; return -1; }
  }
  hipLaunchKernelGGL(k_fill_vertices, dim3((unsigned)((ctx->ncells + 255) / 256)), dim3(256), 0, ctx->stream, ctx->d, ctx->d_vcol,
                     (uint32_t)ncolors, ctx->d_vtx, cut);
  HIPCHK(ctx, hipMemcpyAsync(out_vertices44, ctx->d_vtx, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return 0;
}
int smx_fill_vertices(smx_ctx* ctx, const float* colors4, int32_t ncolors, void* out_vertices44) {
  return fill_vertices(ctx, colors4, ncolors, out_vertices44, VCut{-1, 0.0, 0.f});
}
int smx_fill_vertices_cut(smx_ctx* ctx, const float* colors4, int32_t ncolors, int32_t mode, double cut, void* out_vertices44) {
  VCut c;
  c.mode = mode ? 1 : 0;
  if (mode == 0) { const int sl = (int)cut; c.thr = (double)((float)sl / (float)ctx->d.scale); c.ycut = (float)sl; }   // (float)SLICE/(float)SCALE, vec3(p.x, SLICE, p.y)
  else { c.thr = cut / (double)ctx->d.scale; c.ycut = (float)cut; }                                                    // s/SCALE, vec3(p.x, s, p.y)
  return fill_vertices(ctx, colors4, ncolors, out_vertices44, c);
}
int smx_fill_vertex_cut(smx_ctx* ctx, const float* colors4, int32_t ncolors, int32_t mode, double cut, int32_t x, int32_t y, void* out_vertex44) {
  if (x < 0 || y < 0 || x >= ctx->cfg.dimx || y >= ctx->cfg.dimy) { ctx->err = "smx_fill_vertex_cut: position outside the map"; return -2; }
  VCut c;
  c.mode = mode < 0 ? -1 : (mode ? 1 : 0); c.thr = 0.0; c.ycut = 0.f;
  if (mode == 0) { const int sl = (int)cut; c.thr = (double)((float)sl / (float)ctx->d.scale); c.ycut = (float)sl; }
  else if (mode > 0) { c.thr = cut / (double)ctx->d.scale; c.ycut = (float)cut; }
  return fill_vertices(ctx, colors4, ncolors, out_vertex44, c, (long long)x * ctx->cfg.dimy + y);
}

int smx_heights_bilinear(smx_ctx* ctx, const float* pos2, int32_t n, double* out) {
  FULLMAP("smx_heights_bilinear")
  if (n < 0 || (n > 0 && (!pos2 || !out))) { ctx->err = "smx_heights_bilinear: n < 0 or a null array"; return -2; }
  if (n == 0) return 0;
  // Layermap::height(vec2) reads the cells (px, py), (px + 1, py), (px, py + 1), (px + 1, py + 1) without a check (layermap.h:427-439): a position
  // is defined only in [0, dimx - 1) x [0, dimy - 1) -- none on a map one cell wide. Anything else (NaN included) is refused before a lane reads.
  for (int32_t i = 0; i < n; i++) {
    const float fx = floorf(pos2[2 * i]), fy = floorf(pos2[2 * i + 1]);
    if (!(fx >= 0.f && fx <= (float)(ctx->cfg.dimx - 2) && fy >= 0.f && fy <= (float)(ctx->cfg.dimy - 2))) {
      ctx->err = "smx_heights_bilinear: position " + std::to_string(i) + " outside [0, dimx - 1) x [0, dimy - 1)"; return -2;
    }
  }
  float* dpos = nullptr; double* dout = nullptr;
  HIPCHK(ctx, ctx->mem.dev(dpos, (size_t)n * 2)); HIPCHK(ctx, ctx->mem.dev(dout, (size_t)n));
  HIPCHK(ctx, hipMemcpyAsync(dpos, pos2, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(k_bilinear, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, ctx->d, dpos, n, dout);
  hipError_t e = hipMemcpyAsync(out, dout, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  ctx->mem.drop(dpos); ctx->mem.drop(dout);
  if (e != hipSuccess) { ctx->err = hipGetErrorString(e); return -1; }
  return 0;
}

// ---------------- speculative engine: host driver ----------------
static int spec_alloc(smx_ctx* ctx, uint32_t n) {          // n = particles of a sub-phase; it owns n + SPEC_MAXNEST slots
  FULLMAP("the speculative engine")
  if (ctx->spec_cap >= n && !ctx->spec_realloc) return 0;
  ctx->spec_realloc = false;
  SpecShared& sh = ctx->sh;
  DevMem& m = ctx->mem;
  if (ctx->spec_cap) {                                        // the per-slot buffers go before the larger ones are asked for
    m.drop(sh.part); m.drop(sh.chunk_tab); m.drop(sh.arena); m.drop(sh.alloc_log); m.drop(sh.free_log);
    m.drop(sh.pending); m.drop(sh.draws); m.drop(sh.scout_cells); m.drop(sh.scout_len); m.drop(sh.ckpt);
    ctx->spec_cap = 0;
  } else {
    HIPCHK(ctx, m.dev(sh.stamp, ctx->ncells)); HIPCHK(ctx, m.dev(sh.claim, ctx->ncells));
    HIPCHK(ctx, m.dev(sh.ctrl, SC_COUNT));
    sh.reclaim_cap = 1u << 22; HIPCHK(ctx, m.dev(sh.reclaim, sh.reclaim_cap));
    HIPCHK(ctx, m.pinned(ctx->h_ctrl, SC_COUNT));
  }
  const uint32_t cap = n < 1024 ? 1024 : n;                 // particles
  // nested-particle slots of a sub-phase: 8192 on the device (21 KB of per-slot records each: 170 MB). With the 1 024 of round 3 a
  // sub-phase of 4 096 particles at the headline's density was cut -- everything in flight rolled back on one lane and run again --
  // after ~650 committed particles (profiles/r04_exact_subphases.md)
  static const uint32_t maxnest = (uint32_t)std::min(60000ll, std::max(128ll, env_int("SMX_SPEC_MAXNEST")));
  sh.maxnest = ctx->spec_maxnest ? ctx->spec_maxnest : maxnest;
  const uint32_t slots = cap + sh.maxnest;                  // per-slot records (soil_spec.h "rand() SLOTS")
  HIPCHK(ctx, m.dev(sh.part, slots)); HIPCHK(ctx, m.dev(sh.chunk_tab, (size_t)slots * MAX_CHUNKS));
  sh.arena_chunks = cap * 32u < 16384u ? 16384u : cap * 32u;
  HIPCHK(ctx, m.dev(sh.arena, (size_t)sh.arena_chunks * LOG_CHUNK));
  HIPCHK(ctx, m.dev(sh.alloc_log, (size_t)slots * MAX_NODELOG)); HIPCHK(ctx, m.dev(sh.free_log, (size_t)slots * MAX_NODELOG));
  HIPCHK(ctx, m.dev(sh.pending, slots)); sh.ndraws = 2 * slots; HIPCHK(ctx, m.dev(sh.draws, sh.ndraws));
  // scouted footprints (the first n + SPEC_SCOUT_MARGIN slots only): water paths are a few thousand cells, wind paths up to ~10^5
  sh.scout_cap = cap <= 2048 ? 131072u : 16384u;
  HIPCHK(ctx, m.dev(sh.scout_cells, (size_t)(cap + SPEC_SCOUT_MARGIN) * sh.scout_cap)); HIPCHK(ctx, m.dev(sh.scout_len, slots));
  HIPCHK(ctx, m.dev(sh.ckpt, slots));
  sh.mode = 3u;
  ctx->spec_cap = cap;
  return 0;
}

// One SUB-PHASE of a particle phase with the speculative engine: the next `n` top-level particles of the phase, from the generator
// state and the map as they stand. It ends when all n are committed (outcome 0), when the nested particles it has committed use up
// the slots a sub-phase owns (outcome 1: everything committed so far stays, the caller goes on with a fresh sub-phase from the
// continued rand() stream -- water.h:246-264 draws nested particles from the one stream, which is why the slots are finite), or
// when the speculation cannot go on (outcome 2: no pool headroom, stalled prefix -- the caller hands the rest to the serial walker).
// Results are bit-identical whichever way a phase is cut (tests/test_gpu_parity.py, tests/test_hostsim.py).
static int spec_subphase(smx_ctx* ctx, int32_t n, bool wind, uint32_t* committed, int* outcome) {
  // engine mode per phase: water = blocked-filter + suspend/resume, wind = suspend/resume only (long wind particles
  // are nearly always "blocked somewhere": better to let them run up to the contested cell) -- host-sim measurements
  static const uint32_t mode_water = (uint32_t)env_int("SMX_SPEC_MODE");
  static const uint32_t mode_wind = (uint32_t)env_int("SMX_SPEC_MODE_WIND");
  ctx->sh.mode = wind ? mode_wind : mode_water;
  const SpecShared& sh = ctx->sh;
  hipStream_t st = ctx->stream;
  HIPCHK(ctx, hipMemsetAsync(sh.stamp, 0, ctx->ncells * 4, st));
  hipLaunchKernelGGL(k_spec_begin, dim3(1), dim3(256), 0, st, ctx->d, sh, (uint32_t)n);
  const uint32_t L = (uint32_t)spec_lanes();
  static const bool wind_scout = env_flag("SMX_WIND_SCOUT");
  const uint32_t ns = (uint32_t)n + SPEC_SCOUT_MARGIN;       // scouted slots
  if (!wind || wind_scout) {
    if (coop_on()) LAUNCH_WIND_WATER(wind, k_spec_scout_coop, dim3(ns), dim3(64), st, ctx->d, sh);
    else LAUNCH_WIND_WATER(wind, k_spec_scout, dim3((ns + L - 1) / L), dim3(64), st, ctx->d, sh, L);
  }
  uint32_t np = (uint32_t)n > SPEC_WINDOW ? SPEC_WINDOW : (uint32_t)n, last_base = 0, stall = 0;
  *outcome = 0;
  static const bool trace_rounds = env_flag("SMX_TRACE_ROUNDS");
  uint32_t prev_exec = 0, prev_sum = 0;
  if (trace_rounds) HIPCHK(ctx, hipStreamSynchronize(st));
  auto t_round = std::chrono::steady_clock::now();
  for (int round = 0;; round++) {
    HIPCHK(ctx, hipMemsetAsync(sh.claim, 0xFF, ctx->ncells * 4, st));
    hipLaunchKernelGGL(k_spec_claim, dim3(np), dim3(64), 0, st, sh);
    if (sh.mode & 1u) hipLaunchKernelGGL(k_spec_select, dim3(np), dim3(64), 0, st, sh);
    {
      PhaseTimer tk(ctx, wind ? PH_K_WIND : PH_K_WATER);
      if (coop_on()) LAUNCH_WIND_WATER(wind, k_spec_exec_coop, dim3(np), dim3(64), st, ctx->d, sh);
      else LAUNCH_WIND_WATER(wind, k_spec_exec, dim3((np + L - 1) / L), dim3(64), st, ctx->d, sh, L);
    }
    hipLaunchKernelGGL(k_spec_boundary, dim3(1), dim3(1024), 0, st, ctx->d, sh);
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_ctrl, sh.ctrl, SC_COUNT * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    const uint32_t* c = ctx->h_ctrl;
    if (trace_rounds) {                                                   // SMX_TRACE_ROUNDS=1: one line per round on stderr
      const auto now = std::chrono::steady_clock::now();
      fprintf(stderr, "[soilmx] %s round %3d: %7.3f ms  pending-in %4u  base %4u  executed %5u  longest %6u steps  aborts %u kills %u suspends %u\n",
              wind ? "wind " : "water", round, std::chrono::duration<double, std::milli>(now - t_round).count(), np, c[SC_BASE],
              c[SC_EXECUTED] - prev_exec, c[SC_SUM_MAXSTEPS] - prev_sum, c[SC_ABORTS], c[SC_KILLS], c[SC_SUSPENDS]);
      prev_exec = c[SC_EXECUTED]; prev_sum = c[SC_SUM_MAXSTEPS]; t_round = now;
    }
    if (c[SC_N] == 0) { *outcome = 2; break; }                          // no pool headroom: nothing was executed
    if (c[SC_TOP] == (uint32_t)n) break;                                // n top-level particles committed
    np = c[SC_NPENDING];
    if (c[SC_BASE] == last_base) stall++; else { stall = 0; last_base = c[SC_BASE]; }
    if (c[SC_NESTED_COMMITTED] + 64 > sh.maxnest) { *outcome = 1; break; }   // the sub-phase's nested slots are used up: commit, re-arm
    if (np == 0 || stall >= SPEC_STALL_LIMIT || round > 100000) { *outcome = 2; break; }
  }
  const uint32_t* c = ctx->h_ctrl;
  ctx->spec_rounds += c[SC_ROUNDS]; ctx->spec_aborts += c[SC_ABORTS]; ctx->spec_kills += c[SC_KILLS]; ctx->spec_executed += c[SC_EXECUTED];
  *committed = (c[SC_N] == 0) ? 0u : c[SC_TOP];                        // top-level particles the speculation committed
  if (*outcome != 0) {
    if (c[SC_N] != 0) {
      hipLaunchKernelGGL(k_spec_abandon, dim3(1), dim3(64), 0, st, ctx->d, sh);
      hipLaunchKernelGGL(k_spec_end, dim3(1), dim3(256), 0, st, ctx->d, sh, 0u);
    }
  } else {
    hipLaunchKernelGGL(k_spec_end, dim3(1), dim3(256), 0, st, ctx->d, sh, 1u);
  }
  HIPCHK(ctx, hipGetLastError());
  {
    uint32_t crossed = 0;
    HIPCHK(ctx, hipMemcpyAsync(&crossed, sh.ctrl + SC_POOL_CROSSED, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (crossed) { ctx->err = "speculative phase ran past pool_capacity (pool.get() would have failed inside it): raise pool_capacity"; return -6; }
  }
  if (c[SC_RECLAIM_LOST] != 0) { ctx->err = "speculative phase: reclaim list overflow (pool nodes leaked)"; return -6; }
  return 0;
}
// One particle phase (SoilMachine.cpp:287-298 or :303-307) with the speculative engine, in sub-phases of at most SPEC_SUB top-level
// particles (round 4; round 3 gave the WHOLE rest of a phase to the one-lane serial walker as soon as 1 024 nested particles had
// committed: 0.4 M steps/s on the headline workload). Only what the speculation cannot do at all goes to the serial walker.
static int spec_phase(smx_ctx* ctx, int32_t n, bool wind) {
  if (n <= 0) return 0;
  static const uint32_t SPEC_SUB_ENV = (uint32_t)std::max(64ll, env_int("SMX_SPEC_SUB"));
  const uint32_t SPEC_SUB = ctx->spec_sub ? ctx->spec_sub : SPEC_SUB_ENV;
  if (spec_alloc(ctx, std::min<uint32_t>((uint32_t)n, SPEC_SUB))) return -1;
  hipStream_t st = ctx->stream;
  uint32_t remaining = (uint32_t)n;
  auto serial = [&](uint32_t k) {                            // the reference's order on one lane, from the state as it stands
    PhaseTimer tk(ctx, wind ? PH_K_WIND : PH_K_WATER);
    if (wind) hipLaunchKernelGGL(k_wind_serial, dim3(1), dim3(64), 0, st, ctx->d, (int)k);
    else hipLaunchKernelGGL(k_water_serial, dim3(1), dim3(64), 0, st, ctx->d, (int)k);
  };
  while (remaining > 0) {
    const uint32_t m = std::min(remaining, SPEC_SUB);
    uint32_t committed = 0; int outcome = 0;
    const int rc = spec_subphase(ctx, (int32_t)m, wind, &committed, &outcome);
    if (rc) return rc;
    remaining -= committed;
    if (outcome == 0) continue;
    ctx->spec_subphases_cut++;
    if (outcome == 2) { ctx->spec_fallbacks++; serial(remaining); remaining = 0; }
    else if (committed == 0) { ctx->spec_serial_particles++; serial(1u); remaining -= 1u; }   // one particle with more nested particles than a sub-phase has slots
  }
  HIPCHK(ctx, hipGetLastError());
  return 0;
}


static void launch_classify(smx_ctx* ctx);
// ---------------- batched engine: host driver (tests/hostsim/hostsim.cpp batch_generations drives the same headers on host threads) ----------------
static int batch_alloc(smx_ctx* ctx, uint32_t nslots, bool wind) {
  BatchShared& bs = ctx->bs;
  DevMem& m = ctx->mem;
  if (!bs.ctrl) {
    bs.tshift = -1; bs.ntx = ctx->cfg.dimx; bs.nty = ctx->cfg.dimy; bs.txb = 0; bs.txe = ctx->cfg.dimx;
    const size_t nt = ctx->lcells + 2 * (size_t)ctx->cfg.dimy;   // one claim word per held cell (+ a row of slack for tiles cut by the range's edges): enough for every granularity
    HIPCHK(ctx, m.dev(bs.claim[0], nt)); HIPCHK(ctx, m.dev(bs.claim[1], nt));
    HIPCHK(ctx, m.dev(bs.ctrl, BC_COUNT)); HIPCHK(ctx, hipMemsetAsync(bs.ctrl, 0, BC_COUNT * 4, ctx->stream));
    // nested particles of one generation / pool nodes released in one chunk: sized by the map (a grid pass over a map full
    // of lakes emits children for a sizeable part of its cells); running out is counted (children_lost) / an error (freed)
    bs.child_cap = (uint32_t)std::max<size_t>((size_t)1 << 20, ctx->lcells / 2); HIPCHK(ctx, m.dev(bs.children, bs.child_cap));
    bs.freed_cap = (uint32_t)std::max<size_t>((size_t)1 << 22, ctx->lcells / 2); HIPCHK(ctx, m.dev(bs.freed, bs.freed_cap));
    {
      const size_t ngt = (size_t)((ctx->cfg.dimx + 3) >> 2) * ((ctx->cfg.dimy + 3) >> 2);
      HIPCHK(ctx, m.dev(bs.dirty, ngt)); HIPCHK(ctx, hipMemsetAsync(bs.dirty, 0, ngt, ctx->stream));
    }
    HIPCHK(ctx, m.pinned(ctx->h_bctrl, BC_COUNT));
  }
  if (ctx->batch_cap < nslots) {
    m.drop(bs.water); m.drop(bs.wind); m.drop(bs.live); ctx->batch_cap = 0;
    const uint32_t cap = nslots < 4096u ? 4096u : nslots;
    HIPCHK(ctx, m.dev(bs.water, cap)); HIPCHK(ctx, m.dev(bs.wind, cap)); HIPCHK(ctx, m.dev(bs.live, cap));
    ctx->batch_cap = cap;
  }
  if (ctx->cfg.engine == SMX_ENGINE_RELAXED && ctx->relax_cap < ctx->batch_cap) {   // request entries (2 per step), per-epoch flood and cascade lists
    m.drop(bs.req); m.drop(bs.rnext); m.drop(bs.rcount); ctx->relax_cap = 0;
    for (int k = 0; k < 2; k++) { m.drop(bs.flist[k]); m.drop(bs.flagl[k]); m.drop(bs.clist[k]); }
    const uint32_t cap = ctx->batch_cap;
    const size_t ent = (size_t)cap * 2 * R_MAXSTEPS;
    HIPCHK(ctx, m.dev(bs.req, ent)); HIPCHK(ctx, m.dev(bs.rnext, ent)); HIPCHK(ctx, m.dev(bs.rcount, cap));
    HIPCHK(ctx, hipMemsetAsync(bs.rcount, 0, (size_t)cap * 4, ctx->stream));
    bs.list_cap = cap; bs.flag_cap = (uint32_t)ent; bs.clist_cap = (uint32_t)std::max<size_t>(4096, ent / 2);
    for (int k = 0; k < 2; k++) {
      HIPCHK(ctx, m.dev(bs.flist[k], bs.list_cap)); HIPCHK(ctx, m.dev(bs.flagl[k], bs.flag_cap));
      HIPCHK(ctx, m.dev(bs.clist[k], (size_t)9 * bs.clist_cap));
    }
    ctx->relax_cap = cap;
  }
  if (ctx->cfg.engine == SMX_ENGINE_RELAXED && !bs.rhead) {   // per-cell request lists and cascade flags (8 B / cell), empty between epochs
    HIPCHK(ctx, m.dev(ctx->rhead_alloc, ctx->lcells)); HIPCHK(ctx, m.dev(ctx->cflag_alloc, ctx->lcells));
    HIPCHK(ctx, hipMemsetAsync(ctx->rhead_alloc, 0xFF, ctx->lcells * 4, ctx->stream)); HIPCHK(ctx, hipMemsetAsync(ctx->cflag_alloc, 0, ctx->lcells * 4, ctx->stream));
    HIPCHK(ctx, m.dev(ctx->cstate_alloc, ctx->lcells)); HIPCHK(ctx, hipMemsetAsync(ctx->cstate_alloc, 0, ctx->lcells * 4, ctx->stream));
    bs.rhead = ctx->rhead_alloc - ctx->c_lo; bs.cflag = ctx->cflag_alloc - ctx->c_lo; bs.cstate = ctx->cstate_alloc - ctx->c_lo;   // (global cell index, held range only)
  }
  if (ctx->draws_cap < 2u * nslots) {
    m.drop(ctx->d_draws); m.drop(ctx->h_draws); ctx->draws_cap = 0;
    const uint32_t cap = 2u * (nslots < 4096u ? 4096u : nslots);
    HIPCHK(ctx, m.dev(ctx->d_draws, cap)); HIPCHK(ctx, m.pinned(ctx->h_draws, cap));
    ctx->draws_cap = cap;
  }
  bs.draws = ctx->d_draws; bs.dilate = ctx->batch_dilate; bs.maxsteps = 1;
  bs.strips = batch_make_strips(ctx->cfg.dimx, ctx->strips_n, ctx->strips_a, ctx->strips_b); bs.sphase = STRIP_INTERIOR;
  bs.own_x0 = ctx->own_x0; bs.own_x1 = ctx->own_x1 < 0 ? ctx->cfg.dimx : ctx->own_x1;
  bs.birth_n = 0u; bs.birth_gap = 0u;
  if (!wind && ctx->stagger_phase_n) {                       // staggered generations (smx_set_water_stagger): slot i of the phase's top-level particles is born in epoch (i / birth_n) * gap
    const uint32_t k = (uint32_t)(ctx->water_generations < 1 ? 1 : ctx->water_generations);
    bs.birth_n = (ctx->stagger_phase_n + k - 1u) / k; bs.birth_gap = (uint32_t)ctx->water_stagger;
  }
  return 0;
}
// generations of one phase: `kids` = children to start from (grid pass), else n top-level particles
// every slot whose particle waits for its flood joins the flood list of `parity` (column strips: particles arrive and leave between chunks)
__global__ void __launch_bounds__(256) k_relax_rebuild_floods(BatchShared bs, uint32_t nslots, uint32_t parity) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  relax_flood_later(bs, i, parity, i < nslots && bs.water[i].state == B_ENDED);
}
// Children of a generation -> the next generation's slots, in key order (the order decides slot numbers = priorities and rand() draws),
// without leaving the device: keys are unique ((parent << 8) | sequence), so any sort gives the one order. Round 3 copied the records to
// the host, std::sort-ed them there and copied them back: 5-6 ms of an idle device per generation once a tick spawns 10^6 nested
// particles (profiles/r04_relaxed.md).
__global__ void __launch_bounds__(256) k_child_keys(const BChild* __restrict__ ch, uint32_t n, unsigned long long* __restrict__ keys, uint32_t* __restrict__ idx) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) { keys[i] = ch[i].key; idx[i] = i; }
}
__global__ void __launch_bounds__(256) k_child_gather(const BChild* __restrict__ ch, const uint32_t* __restrict__ idx, uint32_t n, BChild* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) out[i] = ch[idx[i]];
}
static int sort_children(smx_ctx* ctx, uint32_t nc) {       // bs.children[0, nc) -> ctx->d_kids[0, nc), ascending key; asynchronous on the context's stream
  hipStream_t st = ctx->stream;
  if (nc == 0) return 0;
  DevMem& m = ctx->mem;
  HIPCHK(ctx, m.grow(ctx->d_kids, ctx->kids_cap, nc, nc + nc / 2));
  if (ctx->sort_cap < nc) {
    for (int k = 0; k < 2; k++) { m.drop(ctx->d_skeys[k]); m.drop(ctx->d_sidx[k]); }
    m.drop(ctx->d_stemp); ctx->stemp_bytes = 0; ctx->sort_cap = 0;
    const uint32_t cap = nc + nc / 2;
    for (int k = 0; k < 2; k++) { HIPCHK(ctx, m.dev(ctx->d_skeys[k], cap)); HIPCHK(ctx, m.dev(ctx->d_sidx[k], cap)); }
    size_t tb = 0;
    HIPCHK(ctx, rocprim::radix_sort_pairs(nullptr, tb, ctx->d_skeys[0], ctx->d_skeys[1], ctx->d_sidx[0], ctx->d_sidx[1], (size_t)cap, 0u, 64u, st));
    HIPCHK(ctx, m.dev(ctx->d_stemp, tb)); ctx->stemp_bytes = tb; ctx->sort_cap = cap;
  }
  const unsigned nb = (nc + 255u) / 256u;
  hipLaunchKernelGGL(k_child_keys, dim3(nb), dim3(256), 0, st, ctx->bs.children, nc, ctx->d_skeys[0], ctx->d_sidx[0]);
  size_t tb = ctx->stemp_bytes;
  HIPCHK(ctx, rocprim::radix_sort_pairs(ctx->d_stemp, tb, ctx->d_skeys[0], ctx->d_skeys[1], ctx->d_sidx[0], ctx->d_sidx[1], (size_t)nc, 0u, 64u, st));
  hipLaunchKernelGGL(k_child_gather, dim3(nb), dim3(256), 0, st, ctx->bs.children, ctx->d_sidx[1], nc, ctx->d_kids);
  return 0;
}
// What the batch control block, as last copied to ctx->h_bctrl, says about the generation (or the grid pass) that just ended: work that
// was dropped is an error; `nc` = the children it left, as many as the buffer holds.
static int batch_check_ctrl(smx_ctx* ctx, uint32_t& nc) {
  nc = ctx->h_bctrl[BC_NCHILD];
  if (ctx->h_bctrl[BC_CHILD_LOST]) ctx->batch_children_lost += ctx->h_bctrl[BC_CHILD_LOST];
  if (ctx->h_bctrl[BC_FREED_LOST]) { ctx->err = "batched engine: freed-node list overflow (pool nodes leaked)"; return -6; }
  if (ctx->h_bctrl[BC_LIST_LOST]) { ctx->err = "relaxed schedule: flood / cascade list overflow (work was dropped)"; return -6; }
  if (ctx->h_bctrl[BC_STALLED]) { ctx->err = "throughput schedule: a device-side wait ran out of its spin budget (a dataflow dependency or a barrier was never released)"; return -9; }
  if (nc > ctx->bs.child_cap) nc = ctx->bs.child_cap;
  return 0;
}
// `nepochs` dense epochs of the running relaxed water generation as one persistent cooperative launch (k_relax_epochs). 0 = launched.
static int relax_epochs_launch(smx_ctx* ctx, uint32_t nlive, uint32_t epoch, uint32_t nepochs) {
  hipStream_t st = ctx->stream;
  if (!ctx->d_gbar) {
    if (ctx->mem.dev(ctx->d_gbar, 1) != hipSuccess) { ctx->mega_off = true; return 1; }
    hipMemsetAsync(ctx->d_gbar, 0, sizeof(GridBar), st);
  }
  if (!ctx->mega_blocks) {
    int dev = 0, ncu = 0, coop = 0, per_cu = 0;
    hipGetDevice(&dev);
    hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
    hipDeviceGetAttribute(&coop, hipDeviceAttributeCooperativeLaunch, dev);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_relax_epochs, 256, 0) != hipSuccess) per_cu = 0;
    static const int want = (int)env_int("SMX_RELAX_MEGA_BLOCKS");   // (0: one workgroup per CU)
    int nb = want > 0 ? want : ncu;
    if (nb > ncu * per_cu) nb = ncu * per_cu;
    if (!coop || nb < 1) {
      fprintf(stderr, "[soilmx] cooperative launch unavailable (attribute %d, %d CUs x %d workgroups): the relaxed epochs run as per-phase launches\n", coop, ncu, per_cu);
      ctx->mega_off = true; return 1;
    }
    ctx->mega_blocks = nb;
  }
  BatchShared bs = ctx->bs;
  uint32_t tag0 = ctx->relax_tag + 1u;
  GridBar* bar = ctx->d_gbar;
  static const uint32_t dense_waves_env = (uint32_t)env_int("SMX_RELAX_MEGA_WAVES");   // (0: one wavefront per workgroup)
  uint32_t dense_waves = dense_waves_env ? dense_waves_env : (uint32_t)ctx->mega_blocks, flags = relax_mega_flags();
  void* args[] = {(void*)&ctx->d, (void*)&bs, (void*)&nlive, (void*)&epoch, (void*)&nepochs, (void*)&tag0, (void*)&bar, (void*)&dense_waves, (void*)&flags};
  PhaseTimer tk(ctx, PH_K_EPOCHS, nepochs);
  const hipError_t e = hipLaunchCooperativeKernel((const void*)k_relax_epochs, dim3((unsigned)ctx->mega_blocks), dim3(256), args, 0, st);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    fprintf(stderr, "[soilmx] hipLaunchCooperativeKernel(k_relax_epochs, %d workgroups): %s -- the relaxed epochs run as per-phase launches\n", ctx->mega_blocks, hipGetErrorString(e));
    ctx->mega_off = true; return 1;
  }
  return 0;
}
// Flagged cells per wavefront of the two dense launches after apply, k_relax_settle and k_relax_filter: as thin as `waves` wavefronts allow for the worst
// case of `worst` flagged cells (every entry of every running particle flags another cell), as batch_lanes_per_wave spreads particles. 0: even 64 per
// wavefront need more. Which lane holds a cell has no influence on results.
// The count the rule starts from, measured on the headline (profiles/r14_settle.md; generations of 8 000 particles, k_relax_settle):
//   cells per wavefront      4        8       16       32       64
//   ms per tick         1 175.6  1 157.3  1 160.5  1 167.6  1 178.1     (water phase: 790.9  774.0  774.1  779.4  788.9)
// thinner than 8, dispatching wavefronts that read the count and leave costs more than the shorter union of paths saves.
constexpr uint32_t RELAX_SETTLE_LANES = 8;
static uint32_t relax_settle_lanes(size_t worst, size_t waves, uint32_t forced) {
  uint32_t l = forced ? forced : RELAX_SETTLE_LANES;
  while (l < 64u && (worst + l - 1u) / l > waves) l = std::min(64u, l * 2u);
  return (worst + l - 1u) / l > waves ? 0u : l;
}
// k_relax_settle waits between wavefronts: ALL wavefronts of a launch must be resident together (the argument above the kernel). How many the device
// holds is asked once per context; an epoch whose worst-case grid exceeds it takes the two launches. 0: this epoch cannot be fused.
constexpr int RELAX_SETTLE_DEFAULT = 2;   // (three runs each, ms per tick: parent 1 229.9, two launches 1 196.3, fused 1 160.7 -- profiles/r14_settle.md;
                                          //  with the floods inside the fused launch, mode 2: profiles/r15_settle_floods.md)
static int relax_resident_waves(const void* kernel) {                  // wavefronts of a one-wavefront-per-workgroup kernel the device holds at once (-1: the query failed)
  int dev = 0, ncu = 0, per_cu = 0;
  hipGetDevice(&dev);
  hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 64, 0) != hipSuccess) { (void)hipGetLastError(); per_cu = 0; }
  return ncu * per_cu > 0 ? ncu * per_cu : -1;
}
static bool relax_settle_counters(smx_ctx* ctx) {
  if (!ctx->d_settle_crowded) {
    if (ctx->mem.dev(ctx->d_settle_crowded, 3) != hipSuccess) { (void)hipGetLastError(); return false; }
    hipMemsetAsync(ctx->d_settle_crowded, 0, 3 * sizeof(unsigned long long), ctx->stream);
  }
  return true;
}
static uint32_t relax_settle_plan(smx_ctx* ctx, size_t worst) {
  if (!ctx->settle_resident) ctx->settle_resident = relax_resident_waves((const void*)k_relax_settle);
  if (ctx->settle_resident < 0) return 0u;
  if (!relax_settle_counters(ctx)) { ctx->settle_resident = -1; return 0u; }
  const size_t waves = ctx->settle_max_waves > 0 ? std::min<size_t>((size_t)ctx->settle_max_waves, (size_t)ctx->settle_resident) : (size_t)ctx->settle_resident;
  return relax_settle_lanes(worst, waves, (uint32_t)ctx->settle_lanes);
}
// k_relax_settle_floods: S settle and F flood wavefronts must be resident TOGETHER (flood wavefronts wait for settle wavefronts). The resident count is
// this kernel's own (the flood body's registers: about one wavefront per SIMD, half of k_relax_settle's). F >= ceil(nslots / 64), because the host does
// not know the length of the flood list; the settle lanes per wavefront double from the rule's 8 until S fits beside that (8 and 16 lanes are one run's
// noise apart, profiles/r14_settle.md); the floods then spread over what is left, up to the `nfb` wavefronts k_relax_floods gets. false: it does not fit,
// the epoch takes k_relax_settle and k_relax_floods.
static bool relax_settle_floods_plan(smx_ctx* ctx, size_t worst, uint32_t nslots, unsigned nfb, uint32_t& lpw, unsigned& nsettle, unsigned& nfloods) {
  if (!ctx->joined_resident) ctx->joined_resident = relax_resident_waves((const void*)k_relax_settle_floods);
  if (ctx->joined_resident < 0) return false;
  if (!relax_settle_counters(ctx)) { ctx->joined_resident = -1; return false; }
  const size_t waves = ctx->settle_max_waves > 0 ? std::min<size_t>((size_t)ctx->settle_max_waves, (size_t)ctx->joined_resident) : (size_t)ctx->joined_resident;
  const size_t fmin = std::max<size_t>(1u, ((size_t)nslots + 63u) / 64u);
  if (waves <= fmin) return false;
  lpw = relax_settle_lanes(worst, waves - fmin, (uint32_t)ctx->settle_lanes);
  if (!lpw) return false;
  nsettle = (unsigned)((worst + lpw - 1u) / lpw);
  nfloods = (unsigned)std::min<size_t>(waves - nsettle, std::max<size_t>(nfb, fmin));
  return true;
}
// One CHUNK of a particle phase on the context's current generation: the schedule for `nlive_sched` running particles (all strips
// together), fresh reservations where the schedule asks for them, then the chunk's epochs over the `nlive` slots of bs.live.
// Shared by the single-context driver (batch_generations) and the step-wise one of the column strips (smx_d_chunk).
static int run_chunk(smx_ctx* ctx, bool wind, uint32_t nlive_sched, uint32_t nlive, uint32_t nslots, bool first, bool relax_gen, uint32_t& epoch, uint32_t& chunk,
                     int* epochs_run) {
  hipStream_t st = ctx->stream;
  const BatchShared& bs = ctx->bs;
  static const int CHUNK = (int)std::max(1ll, env_int("SMX_BATCH_CHUNK"));
  BSched sc = batch_schedule(wind, nlive_sched, ctx->batch_dilate);
  {   // experiments only: SMX_BATCH_SCHED="tshift,dilate,maxsteps" (water) / SMX_BATCH_SCHED_WIND pins the schedule
    static const char* ew = env_str("SMX_BATCH_SCHED"); static const char* ed = env_str("SMX_BATCH_SCHED_WIND");
    const char* e = wind ? ed : ew; int a, d, k;
    if (e && sscanf(e, "%d,%d,%d", &a, &d, &k) == 3) { sc.tshift = a; sc.dilate = d; sc.maxsteps = k; }
    static const char* etw = env_str("SMX_BATCH_SCHED_TAIL"); static const char* etd = env_str("SMX_BATCH_SCHED_TAIL_WIND");   // "thr:tshift,dilate,maxsteps[;thr2:...]" (ascending thr): first thr >= nlive wins
    const char* et = wind ? etd : etw;
    if (et) {
      const char* q = et; unsigned thr;
      while (q && sscanf(q, "%u:%d,%d,%d", &thr, &a, &d, &k) == 4) {
        if (nlive_sched <= thr) { sc.tshift = a; sc.dilate = d; sc.maxsteps = k; break; }
        q = strchr(q, ';'); if (q) q++;
      }
    }
  }
  const bool strips = bs.strips.n > 1;
  // (bs aliases ctx->bs, passed by value per launch: the plan is written before the first one)
  const BChunkPlan plan = batch_plan_chunk(ctx->bs, ctx->d, sc, wind, nlive_sched, relax_gen, ctx->relax_wind_min, ctx->relax_wind_steps, ctx->relax_water_steps, first, epoch, chunk);
  const bool regrain = plan.regrain;
  if (regrain) {                                           // (the planes hold the tile columns of the context's range)
    const size_t nt = (size_t)(((ctx->d.x_hi - 1) >> bs.tshift) - (ctx->d.x_lo >> bs.tshift) + 1) * bs.nty;
    HIPCHK(ctx, hipMemsetAsync(bs.claim[0], 0, nt * 8, st)); HIPCHK(ctx, hipMemsetAsync(bs.claim[1], 0, nt * 8, st));
  }
  if ((regrain || strips) && nlive)                        // under strips every chunk starts with fresh reservations
    LAUNCH_WIND_WATER(wind, k_batch_reclaim, dim3((nlive + 63u) / 64u), dim3(64), st, ctx->d, bs, nlive, epoch);
  int chunk_epochs = CHUNK;
  if (plan.relaxed_now) {
    // relaxed schedule: per epoch one step of every running particle, the queued edits per cell, the nine cascade colours,
    // then one flood epoch behind claim tiles. Without strips the chunk lengths are the launch shape's to choose (batch_plan_chunk).
    static const int RCHUNK_KIDS = (int)std::max(1ll, env_int("SMX_RELAX_CHUNK_KIDS"));
    static const bool use_tail = env_flag("SMX_RELAX_TAIL");
    static const uint32_t tail_at_env = (uint32_t)env_int("SMX_RELAX_TAIL_AT");
    const uint32_t tail_at = ctx->relax_tail_at >= 0 ? (uint32_t)ctx->relax_tail_at : tail_at_env;
    const bool tail = !wind && use_tail && nlive <= tail_at;
    static const bool use_mega_env = env_flag("SMX_RELAX_MEGA");   // (off by default: measured slower, see k_relax_epochs)
    const bool use_mega = ctx->relax_persistent >= 0 ? ctx->relax_persistent != 0 : use_mega_env;
    static const int mega_chunk = (int)std::max(0ll, env_int("SMX_RELAX_MEGA_CHUNK"));   // (0: the chunk lengths of the per-phase launches)
    const bool mega = !wind && !tail && use_mega && !ctx->mega_off && bs.cstate != nullptr;
    chunk_epochs = strips ? plan.chunk_epochs : (tail ? 64 : (mega && mega_chunk ? mega_chunk : (first ? CHUNK : RCHUNK_KIDS)));
    if (ctx->relax_tag > 0x7FFF0000u) { ctx->relax_tag = 0; HIPCHK(ctx, hipMemsetAsync(ctx->cflag_alloc, 0, ctx->lcells * 4, st)); HIPCHK(ctx, hipMemsetAsync(ctx->cstate_alloc, 0, ctx->lcells * 4, st)); }   // (tags never repeat; 2 * tag + 1 fits 32 bits)
    if (strips) HIPCHK(ctx, hipMemsetAsync(bs.ctrl + BC_NFLOOD, 0, (BC_LISTS_END - BC_NFLOOD) * 4, st));   // (the epoch skipped between two chunks breaks the lists' parity hand-over)
    if (strips && !wind) {                                   // who waits for a flood on this device right now?
      if (nslots) hipLaunchKernelGGL(k_relax_rebuild_floods, dim3((nslots + 255u) / 256u), dim3(256), 0, st, bs, nslots, epoch & 1u);
    }
    if (nlive == 0) { epoch += (uint32_t)chunk_epochs; ctx->relax_tag += (uint32_t)chunk_epochs; }   // (a strip with nobody home this chunk)
    else if (tail) {                                         // few particles left: whole epochs inside one workgroup (k_relax_tail)
      PhaseTimer tk(ctx, PH_K_TAIL, (uint32_t)chunk_epochs);
      hipLaunchKernelGGL(k_relax_tail, dim3(1), dim3(256), 0, st, ctx->d, bs, nlive, epoch, (uint32_t)chunk_epochs, ctx->relax_tag + 1u);
      ctx->relax_tag += (uint32_t)chunk_epochs; epoch += (uint32_t)chunk_epochs;
    } else if (mega && relax_epochs_launch(ctx, nlive, epoch, (uint32_t)chunk_epochs) == 0) {   // the chunk's dense epochs as ONE persistent launch (k_relax_epochs)
      ctx->relax_tag += (uint32_t)chunk_epochs; epoch += (uint32_t)chunk_epochs;
    } else {
      const uint32_t lpw = batch_lanes_per_wave(nlive);
      const unsigned nbl = (nlive + lpw - 1u) / lpw, nb64 = (nlive + 63u) / 64u;
      const unsigned ncb = (unsigned)(((size_t)nlive * (size_t)(wind ? ctx->bs.rstride : ctx->bs.rsteps) + 63u) / 64u);   // worst case of the flagged / one cascade list
      static const unsigned fb_min = (unsigned)env_int("SMX_RELAX_FLOOD_BLOCKS");
      const unsigned nfb = std::max(fb_min, (unsigned)((nslots + 63u) / 64u));   // floods: at least 1024 wavefronts to spread over
      static const unsigned casc_blocks = (unsigned)env_int("SMX_RELAX_CASC_BLOCKS");
      static const unsigned casc_flow = (unsigned)env_int("SMX_RELAX_CASC_FLOW");   // 0: nine launches (round 4)
      const size_t worst = (size_t)nlive * (size_t)(wind ? ctx->bs.rstride : ctx->bs.rsteps);   // (what ncb holds 64 of per wavefront)
      // after apply: ONE dataflow launch where every wavefront of its worst-case grid is resident (smx_set_relax_settle; not under column strips, whose
      // partition nothing on one device can measure; SMX_RELAX_CASC_FLOW=0 keeps meaning filter + nine colour launches) -- else filter + colour lists
      const int settle_mode = ctx->relax_settle >= 0 ? ctx->relax_settle : RELAX_SETTLE_DEFAULT;
      const bool settle_on = settle_mode >= 1 && !strips && casc_flow && bs.cstate;
      uint32_t joined_lpw = 0u; unsigned joined_s = 0u, joined_f = 0u;   // water: settle and floods as ONE launch (k_relax_settle_floods) where S + F wavefronts are resident
      const bool joined = settle_on && settle_mode == 2 && !wind && relax_settle_floods_plan(ctx, worst, nslots, nfb, joined_lpw, joined_s, joined_f);
      const uint32_t settle_lpw = settle_on && !joined ? relax_settle_plan(ctx, worst) : 0u;
      uint32_t filter_lpw = relax_settle_lanes(worst, 4096u, (uint32_t)ctx->settle_lanes);      // (no residency to respect: a bound on the grid)
      if (!filter_lpw) filter_lpw = 64u;
      for (int k = 0; k < chunk_epochs; k++, epoch++) {
        ctx->bs.rtag = ++ctx->relax_tag;
        {
          // the step kernel between its own pair of events -- every `sample`-th launch (an event pair costs a few microseconds of an epoch
          // that lasts a few hundred; the average launch duration bench.py reports is over the bracketed launches only)
          static const int sample = (int)std::max(0ll, env_int("SMX_STEP_EVENT_SAMPLE"));
          const bool timed = sample > 0 && (k % sample) == 0;
          if (wind) ctx->timing.launches_step_wind++; else ctx->timing.launches_step_water++;   // (every launch, bracketed or not)
          if (timed) { PhaseTimer tk(ctx, wind ? PH_K_WIND : PH_K_WATER, 1u); LAUNCH_WIND_WATER(wind, k_relax_step, dim3(nbl), dim3(64), st, ctx->d, bs, nlive, epoch, lpw); }
          else LAUNCH_WIND_WATER(wind, k_relax_step, dim3(nbl), dim3(64), st, ctx->d, bs, nlive, epoch, lpw);
        }
        hipLaunchKernelGGL(k_relax_apply, dim3(nb64), dim3(64), 0, st, ctx->d, bs, nlive, epoch);
        if (joined) {                                        // settle and floods as ONE dataflow launch: counted and bracketed as the flood launch it replaces
          ctx->settle_epochs_fused++; ctx->settle_epochs_joined++;
          ctx->timing.launches_floods_all++;
          const uint32_t fprof = flood_prof();
          const bool timed = ctx->flood_launch_no++ % 7u == 0u;
          if (timed) { PhaseTimer tk(ctx, PH_K_FLOODS, 1u); hipLaunchKernelGGL(k_relax_settle_floods, dim3(joined_s + joined_f), dim3(64), 0, st, ctx->d, bs, epoch, joined_lpw, joined_s, spin_budget(1u << 24), fprof, ctx->d_settle_crowded, ctx->d_settle_crowded + 1); }
          else hipLaunchKernelGGL(k_relax_settle_floods, dim3(joined_s + joined_f), dim3(64), 0, st, ctx->d, bs, epoch, joined_lpw, joined_s, spin_budget(1u << 24), fprof, ctx->d_settle_crowded, ctx->d_settle_crowded + 1);
          continue;
        }
        if (settle_lpw) {                                    // filter and colour lists as ONE dataflow launch (k_relax_settle)
          ctx->settle_epochs_fused++;
          hipLaunchKernelGGL(k_relax_settle, dim3((unsigned)((worst + settle_lpw - 1u) / settle_lpw)), dim3(64), 0, st, ctx->d, bs, epoch, settle_lpw, spin_budget(1u << 24), ctx->d_settle_crowded);
        } else {
          ctx->settle_epochs_split++;
          hipLaunchKernelGGL(k_relax_filter, dim3((unsigned)((worst + filter_lpw - 1u) / filter_lpw)), dim3(64), 0, st, ctx->d, bs, epoch, filter_lpw);
          if (casc_flow && bs.cstate) hipLaunchKernelGGL(k_relax_cascade_flow, dim3(std::min(ncb, casc_flow)), dim3(64), 0, st, ctx->d, bs, epoch, spin_budget(1u << 24));
          else {
            const unsigned ncc = std::min(ncb, std::max(1u, casc_blocks));
            for (uint32_t col = 0; col < 9u; col++) hipLaunchKernelGGL(k_relax_cascade, dim3(ncc), dim3(64), 0, st, ctx->d, bs, epoch, col);
          }
        }
        if (!wind) {                                         // (bracketed every 7th launch of the context: a stride coprime to the every-4th-epoch rule of relax_floods_due)
          ctx->timing.launches_floods_all++;
          const uint32_t fprof = flood_prof();
          if (ctx->flood_launch_no++ % 7u == 0u) { PhaseTimer tk(ctx, PH_K_FLOODS, 1u); hipLaunchKernelGGL(k_relax_floods, dim3(nfb), dim3(64), 0, st, ctx->d, bs, epoch, fprof); }
          else hipLaunchKernelGGL(k_relax_floods, dim3(nfb), dim3(64), 0, st, ctx->d, bs, epoch, fprof);
        }
      }
    }
  } else if (nlive) {
    PhaseTimer tk(ctx, wind ? PH_K_WIND : PH_K_WATER, (uint32_t)CHUNK);   // CHUNK back-to-back launches of the epoch kernel, nothing else
    if (wind) ctx->timing.launches_step_wind += (uint64_t)CHUNK; else ctx->timing.launches_step_water += (uint64_t)CHUNK;
    const uint32_t lpw = batch_lanes_per_wave(nlive);
    const unsigned nbl = (nlive + lpw - 1u) / lpw;
    // more wavefronts than SIMDs (> 65 536 running particles): the 256-register build, two wavefronts per SIMD -- +5 % at 16384^2,
    // nothing below (profiles/r02_batched_schedules.md); results do not depend on it
    static const uint32_t occ2_above = (uint32_t)env_int("SMX_BATCH_OCC2_ABOVE");
    const bool occ2 = nlive > occ2_above;
    for (int k = 0; k < CHUNK; k++, epoch++) {
      if (occ2) LAUNCH_WIND_WATER(wind, k_batch_epoch2, dim3(nbl), dim3(64), st, ctx->d, bs, nlive, epoch, lpw);
      else LAUNCH_WIND_WATER(wind, k_batch_epoch, dim3(nbl), dim3(64), st, ctx->d, bs, nlive, epoch, lpw);
    }
  } else epoch += (uint32_t)CHUNK;
  hipLaunchKernelGGL(k_batch_merge_freed, dim3(1), dim3(256), 0, st, ctx->d, bs);   // frees of the chunk go back on the stack
  if (epochs_run) *epochs_run = chunk_epochs;
  return 0;
}
// generations of one phase: n top-level particles, or (nkids > 0) the children the grid pass left, already sorted into ctx->d_kids
static int batch_generations(smx_ctx* ctx, bool wind, uint32_t n, uint32_t nkids) {
  hipStream_t st = ctx->stream;
  bool first = nkids == 0;
  uint32_t nslots = first ? n : nkids;
  if (nslots == 0) return 0;
  RandState r;                                              // the host draws for the device: glibc rand() is a serial recurrence
  const bool draws = first;                                 // (suspended nested particles carry their state: no draws, no round trip)
  if (draws) {
    HIPCHK(ctx, hipMemcpyAsync(&r, ctx->d.rnd, sizeof(r), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
  }
  while (nslots > 0) {
    if (batch_alloc(ctx, nslots, wind)) return -1;
    const BatchShared& bs = ctx->bs;
    if (first) {                                              // (suspended nested particles carry their state: no draws)
      for (uint32_t i = 0; i < 2u * nslots; i++) {
        ctx->h_draws[i] = rand_step(r) >> 1;
        r.calls++;
      }
      HIPCHK(ctx, hipMemcpyAsync(ctx->d_draws, ctx->h_draws, (size_t)2u * nslots * 4, hipMemcpyHostToDevice, st));
    }
    ctx->bs.tshift = -1;                                      // (the first chunk clears the planes and issues the first reservations)
    const bool relax_gen = ctx->cfg.engine == SMX_ENGINE_RELAXED;
    ctx->bs.relaxed = relax_gen ? 1 : 0;
    if (relax_gen) HIPCHK(ctx, hipMemsetAsync(ctx->bs.ctrl + BC_NFLOOD, 0, (BC_LISTS_END - BC_NFLOOD) * 4, st));   // flood, flag and cascade lists start empty
    const BChild* dk = first ? nullptr : ctx->d_kids;        // (sorted there by sort_children)
    const unsigned nb = (nslots + 63u) / 64u;
    LAUNCH_WIND_WATER(wind, k_batch_spawn, dim3(nb), dim3(64), st, ctx->d, bs, nslots, dk, (const uint32_t*)nullptr);
    hipLaunchKernelGGL(k_batch_iota, dim3((nslots + 255u) / 256u), dim3(256), 0, st, bs.live, nslots);
    uint32_t nlive = nslots, epoch = 0, chunk = 0;
    const bool trace = trace_batch();
    while (nlive > 0) {
      const auto t_chunk = std::chrono::steady_clock::now();
      const uint32_t live_in = nlive;
      int chunk_epochs = 0;
      if (run_chunk(ctx, wind, nlive, nlive, nslots, first, relax_gen, epoch, chunk, &chunk_epochs)) return -1;
      HIPCHK(ctx, hipMemsetAsync(bs.ctrl + BC_NLIVE, 0, 4, st));
      LAUNCH_WIND_WATER(wind, k_batch_compact, dim3((nslots + 255u) / 256u), dim3(256), st, bs, nslots);
      HIPCHK(ctx, hipMemcpyAsync(ctx->h_bctrl, bs.ctrl, BC_COUNT * 4, hipMemcpyDeviceToHost, st));
      HIPCHK(ctx, hipStreamSynchronize(st));
      nlive = ctx->h_bctrl[BC_NLIVE];
      ctx->batch_epochs += chunk_epochs;
      if (trace) fprintf(stderr, "[soilmx] batched %s gen-slots %u epochs %u..%u live %u -> %u grain %d dilate %d maxsteps %d  %.3f ms\n", wind ? "wind " : "water", nslots,
                         epoch - chunk_epochs, epoch, live_in, nlive, 1 << bs.tshift, bs.dilate, bs.maxsteps, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_chunk).count());
    }
    LAUNCH_WIND_WATER(wind, k_batch_counters, dim3(64), dim3(256), st, ctx->d, bs, nslots);
    ctx->batch_generations++;
    // children -> the next generation, in key order (the order decides slot numbers = priorities and rand() draws)
    uint32_t nc = 0;
    if (const int rc = batch_check_ctrl(ctx, nc)) return rc;
    if (wind) nc = 0;
    if (nc && sort_children(ctx, nc)) return -1;             // -> ctx->d_kids, on the device
    HIPCHK(ctx, hipMemsetAsync(bs.ctrl + BC_NCHILD, 0, 8, st));   // NCHILD, CHILD_LOST
    first = false;
    nslots = nc;
  }
  if (draws) {
    HIPCHK(ctx, hipMemcpyAsync(ctx->d.rnd, &r, sizeof(r), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
  }
  HIPCHK(ctx, hipGetLastError());
  return 0;
}
// One sweep of the grid pass over the tile columns [tx_lo, tx_hi): the tiles with work, in (colour, tile) order, through the dataflow
// kernel (k_grid_tiles_flow); bs.sphase says which kind of tile the sweep takes under column strips.
static int grid_sweep(smx_ctx* ctx, int phase, int tx_lo, int tx_hi) {
  hipStream_t st = ctx->stream;
  const int gtx = (ctx->cfg.dimx + (1 << GRID_SHIFT) - 1) >> GRID_SHIFT, gty = (ctx->cfg.dimy + (1 << GRID_SHIFT) - 1) >> GRID_SHIFT;
  const int txb = ctx->d.x_lo >> GRID_SHIFT, txe = ((ctx->d.x_hi - 1) >> GRID_SHIFT) + 1;
  if (tx_lo < txb) tx_lo = txb;
  if (tx_hi > txe) tx_hi = txe;
  if (tx_hi <= tx_lo) return 0;
  if (!ctx->d_tdone) {
    const size_t nt = (size_t)(txe - txb) * gty;
    HIPCHK(ctx, ctx->mem.dev(ctx->d_tdone, nt)); HIPCHK(ctx, ctx->mem.dev(ctx->d_tpend[0], nt)); HIPCHK(ctx, ctx->mem.dev(ctx->d_tpend[1], nt));
    HIPCHK(ctx, ctx->mem.dev(ctx->d_tcount, 2)); HIPCHK(ctx, ctx->mem.pinned(ctx->h_tcount, 2));
  }
  ctx->bs.tshift = GRID_SHIFT; ctx->bs.sphase = phase;
  const BatchShared& bs = ctx->bs;
  GridTiles g;
  g.tdone = ctx->d_tdone; g.pend[0] = ctx->d_tpend[0]; g.pend[1] = ctx->d_tpend[1]; g.count = ctx->d_tcount;
  g.gtx = gtx; g.gty = gty; g.txb = txb; g.txe = txe; g.tx_lo = tx_lo; g.tx_hi = tx_hi;
  g.keybase = (unsigned long long)phase * 9ull * (unsigned long long)gtx * (unsigned long long)gty;   // key prefix = (phase * 9 + colour) * tiles + tile
  HIPCHK(ctx, hipMemsetAsync(ctx->d_tcount, 0, 8, st));
  const uint32_t ntl = (uint32_t)(tx_hi - tx_lo) * (uint32_t)gty;
  hipLaunchKernelGGL(k_grid_tiles_init, dim3((ntl + 255u) / 256u), dim3(256), 0, st, ctx->d, bs, g);
  HIPCHK(ctx, hipMemcpyAsync(ctx->h_tcount, ctx->d_tcount, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  const uint32_t n = ctx->h_tcount[0];
  const bool trace = trace_batch();
  const auto t_sweep = std::chrono::steady_clock::now();
  if (n > 0) {
    // the tiles with work in (colour, tile) order (the init kernel appended them as its wavefronts came); entries are unique
    if (ctx->tsort_cap < n) {
      ctx->mem.drop(ctx->d_tsort); ctx->tsort_cap = 0; ctx->tsort_bytes = 0;
      const uint32_t cap = (uint32_t)((size_t)(txe - txb) * gty);
      size_t tb = 0;
      HIPCHK(ctx, rocprim::radix_sort_keys(nullptr, tb, ctx->d_tpend[0], ctx->d_tpend[1], (size_t)cap, 0u, 32u, st));
      HIPCHK(ctx, ctx->mem.dev(ctx->d_tsort, tb)); ctx->tsort_bytes = tb; ctx->tsort_cap = cap;
    }
    size_t tb = ctx->tsort_bytes;
    HIPCHK(ctx, rocprim::radix_sort_keys(ctx->d_tsort, tb, ctx->d_tpend[0], ctx->d_tpend[1], (size_t)n, 0u, 32u, st));
    HIPCHK(ctx, hipMemsetAsync(ctx->d_tcount + 1, 0, 4, st));     // the cursor of the dataflow kernel
    static const unsigned flow_waves = (unsigned)std::max(1ll, env_int("SMX_GRID_FLOW_WAVES"));
    static const uint32_t poll_naps = (uint32_t)env_int("SMX_GRID_POLL_NAPS");   // (x 3.4 us between two polls of a waiting tile)
    { PhaseTimer tk(ctx, PH_K_GRIDTILES); hipLaunchKernelGGL(k_grid_tiles_flow, dim3(std::min<unsigned>(n, flow_waves)), dim3(64), 0, st, ctx->d, bs, g, ctx->d_tpend[1], n, poll_naps | (flood_prof() ? 0x80000000u : 0u), spin_budget(1u << 22)); }
    hipLaunchKernelGGL(k_batch_merge_freed, dim3(1), dim3(256), 0, st, ctx->d, bs);
    HIPCHK(ctx, hipStreamSynchronize(st));
    ctx->grid_passes++;
  }
  if (trace) fprintf(stderr, "[soilmx] grid sweep (kind %d): %u tiles with work  %.3f ms\n", phase, n, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_sweep).count());
  HIPCHK(ctx, hipGetLastError());
  return 0;
}
static int batch_grid(smx_ctx* ctx) {
  hipStream_t st = ctx->stream;
  if (batch_alloc(ctx, 1, false)) return -1;
  const BatchShared& bs = ctx->bs;
  unsigned long long v0 = 0;
  HIPCHK(ctx, hipMemcpyAsync(&v0, ctx->d.ctr + C_GRID_ACTIVE, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipMemsetAsync(ctx->d.active1, 0, (ctx->nw1 + 64) * 8, st));
  HIPCHK(ctx, hipMemsetAsync(ctx->d.active2, 0, (ctx->nw2 + 64) * 8, st));
  launch_classify(ctx);
  HIPCHK(ctx, hipStreamSynchronize(st));
  const int gtx = (ctx->cfg.dimx + (1 << GRID_SHIFT) - 1) >> GRID_SHIFT;
  for (int ph = 0; ph < (bs.strips.n > 1 ? 2 : 1); ph++) { const int rc = grid_sweep(ctx, ph, 0, gtx); if (rc) return rc; }
  hipLaunchKernelGGL(k_batch_grid_finish, dim3(1), dim3(1), 0, st, ctx->d, v0);
  HIPCHK(ctx, hipMemcpyAsync(ctx->h_bctrl, bs.ctrl, BC_COUNT * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  uint32_t nc = 0;
  if (const int rc = batch_check_ctrl(ctx, nc)) return rc;
  if (nc && sort_children(ctx, nc)) return -1;
  HIPCHK(ctx, hipMemsetAsync(bs.ctrl + BC_NCHILD, 0, 8, st));
  if (nc) { PhaseTimer tk(ctx, PH_K_GRID_CHILDREN); return batch_generations(ctx, false, 0, nc); }   // the nested particles that left their tile's region
  return 0;
}

static void launch_classify(smx_ctx* ctx) {                  // which cells can the grid pass change at all? (one flag byte per cell in, one bit out)
  PhaseTimer tk(ctx, PH_K_CLASSIFY);
  static const bool scalar = env_flag("SMX_CLASSIFY_SCALAR");
  if (ctx->cfg.dimy % 8 == 0 && ctx->lcells % 64 == 0 && ctx->c_lo % 64 == 0 && !scalar)
    hipLaunchKernelGGL(k_grid_classify8, dim3((unsigned)((ctx->lcells / 8 + 255) / 256)), dim3(256), 0, ctx->stream, ctx->d);
  else
    hipLaunchKernelGGL(k_grid_classify, dim3((unsigned)((ctx->lcells + 255) / 256)), dim3(256), 0, ctx->stream, ctx->d);
}

}  // extern "C"

// ---------------- column strips, step by step (the same entry points exist in tests/hostsim as hs_d_*) ----------------
static int xbuf_alloc(smx_ctx* ctx) {
  if (ctx->d_xdata) return 0;
  ctx->xdata_cap = 256ull << 20; ctx->xoffs_cap = 8u << 20;
  HIPCHK(ctx, ctx->mem.dev(ctx->d_xdata, ctx->xdata_cap)); HIPCHK(ctx, ctx->mem.dev(ctx->d_xoffs, ctx->xoffs_cap)); HIPCHK(ctx, ctx->mem.dev(ctx->d_xcur, 2));   // [0] columns, [1] particles (st_pack_band)
  return 0;
}
extern "C" {
int smx_d_set_own(smx_ctx* ctx, int32_t x0, int32_t x1) { ctx->own_x0 = x0; ctx->own_x1 = x1; return 0; }
int smx_d_gen_begin(smx_ctx* ctx, int32_t wind, uint32_t nslots, const void* kids_host, uint32_t* contains_out) {
  hipStream_t st = ctx->stream;
  ctx->d_wind = wind != 0; ctx->d_first = kids_host == nullptr; ctx->d_nslots = nslots; ctx->d_epoch = 0; ctx->d_chunk = 0;
  if (!ctx->strip)                                           // (the step-wise driver of tests/strips_ref.py: a top-level water generation of a staggered phase is the whole phase; smx_strips_tick sets it itself)
    ctx->stagger_phase_n = (!wind && !kids_host && ctx->cfg.engine == SMX_ENGINE_RELAXED && ctx->water_stagger > 0 && ctx->water_generations > 1) ? nslots : 0u;
  if (batch_alloc(ctx, nslots ? nslots : 1, ctx->d_wind)) return -1;
  RandState r;                                              // every rank holds the same generator state and draws the same values
  HIPCHK(ctx, hipMemcpyAsync(&r, ctx->d.rnd, sizeof(r), hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  const uint32_t ndraw = kids_host ? 0u : 2u * nslots;          // (suspended nested particles carry their state: no draws)
  for (uint32_t i = 0; i < ndraw; i++) {
    ctx->h_draws[i] = rand_step(r) >> 1;
    r.calls++;
  }
  HIPCHK(ctx, hipMemcpyAsync(ctx->d.rnd, &r, sizeof(r), hipMemcpyHostToDevice, st));
  if (ndraw) HIPCHK(ctx, hipMemcpyAsync(ctx->d_draws, ctx->h_draws, (size_t)ndraw * 4, hipMemcpyHostToDevice, st));
  ctx->bs.tshift = -1;
  HIPCHK(ctx, hipMemsetAsync(ctx->bs.ctrl + BC_NCHILD, 0, 8, st));
  ctx->bs.relaxed = ctx->cfg.engine == SMX_ENGINE_RELAXED ? 1 : 0;
  if (ctx->bs.relaxed) HIPCHK(ctx, hipMemsetAsync(ctx->bs.ctrl + BC_NFLOOD, 0, (BC_LISTS_END - BC_NFLOOD) * 4, st));   // flood, flag and cascade lists start empty
  if (kids_host) {
    HIPCHK(ctx, ctx->mem.grow(ctx->d_kids, ctx->kids_cap, nslots, nslots));
    HIPCHK(ctx, ctx->mem.grow(ctx->d_contains, ctx->contains_cap, nslots, nslots));
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_kids, kids_host, (size_t)nslots * sizeof(BChild), hipMemcpyHostToDevice, st));
    if (contains_out) {
      hipLaunchKernelGGL(k_batch_child_contains, dim3((nslots + 63u) / 64u), dim3(64), 0, st, ctx->d_kids, nslots, ctx->d_contains);
      HIPCHK(ctx, hipMemcpyAsync(contains_out, ctx->d_contains, (size_t)nslots * 4, hipMemcpyDeviceToHost, st));
    }
  }
  HIPCHK(ctx, hipStreamSynchronize(st));
  return 0;
}
static int d_compact(smx_ctx* ctx, uint32_t* nlive) {
  hipStream_t st = ctx->stream; const BatchShared& bs = ctx->bs; const uint32_t nslots = ctx->d_nslots;
  HIPCHK(ctx, hipMemsetAsync(bs.ctrl + BC_NLIVE, 0, 4, st));
  if (nslots) LAUNCH_WIND_WATER(ctx->d_wind, k_batch_compact, dim3((nslots + 255u) / 256u), dim3(256), st, bs, nslots);
  HIPCHK(ctx, hipMemcpyAsync(ctx->h_bctrl, bs.ctrl, BC_COUNT * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  *nlive = ctx->h_bctrl[BC_NLIVE];
  return 0;
}
int smx_d_gen_spawn(smx_ctx* ctx, const uint32_t* contains_host, uint32_t* nlive_local) {
  hipStream_t st = ctx->stream; const uint32_t nslots = ctx->d_nslots;
  if (nslots == 0) { *nlive_local = 0; return 0; }
  const BChild* dk = ctx->d_first ? nullptr : ctx->d_kids;
  if (dk && contains_host) HIPCHK(ctx, hipMemcpyAsync(ctx->d_contains, contains_host, (size_t)nslots * 4, hipMemcpyHostToDevice, st));
  const unsigned nb = (nslots + 63u) / 64u;
  if (ctx->d_wind) hipLaunchKernelGGL(k_batch_spawn<true>, dim3(nb), dim3(64), 0, st, ctx->d, ctx->bs, nslots, dk, (const uint32_t*)nullptr);
  else hipLaunchKernelGGL(k_batch_spawn<false>, dim3(nb), dim3(64), 0, st, ctx->d, ctx->bs, nslots, dk, (const uint32_t*)(dk && contains_host ? ctx->d_contains : nullptr));
  return d_compact(ctx, nlive_local);
}
int smx_d_next_phase(smx_ctx* ctx) { return ctx->strips_n > 1 ? (int)(ctx->d_chunk & 1u) : STRIP_INTERIOR; }
int smx_d_chunk(smx_ctx* ctx, uint32_t nlive_global, uint32_t* nlive_local) {
  uint32_t nlive = 0;
  if (d_compact(ctx, &nlive)) return -1;                      // residents that run (particles may have arrived or left)
  int epochs = 0;
  if (run_chunk(ctx, ctx->d_wind, nlive_global, nlive, ctx->d_nslots, ctx->d_first, ctx->cfg.engine == SMX_ENGINE_RELAXED, ctx->d_epoch, ctx->d_chunk, &epochs)) return -1;
  ctx->batch_epochs += (uint64_t)epochs;
  return d_compact(ctx, nlive_local);
}
static int d_gen_end_impl(smx_ctx* ctx, void* children_out, uint32_t cap, uint32_t* n, std::vector<BChild>* vec) {
  hipStream_t st = ctx->stream; const BatchShared& bs = ctx->bs; const uint32_t nslots = ctx->d_nslots;
  if (nslots) {
    LAUNCH_WIND_WATER(ctx->d_wind, k_batch_counters, dim3(64), dim3(256), st, ctx->d, bs, nslots);
    ctx->d_nslots = 0;                                       // (the slots' counters are committed once, whatever happens below)
  }
  HIPCHK(ctx, hipMemcpyAsync(ctx->h_bctrl, bs.ctrl, BC_COUNT * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  uint32_t nc = 0;
  if (const int rc = batch_check_ctrl(ctx, nc)) return rc;
  if (vec) { vec->resize(nc); children_out = vec->data(); cap = nc; }
  if (nc > cap) { ctx->err = "smx_d_gen_end: children buffer too small (call again with room for *n records)"; *n = nc; return -2; }
  if (nc) HIPCHK(ctx, hipMemcpyAsync(children_out, bs.children, (size_t)nc * sizeof(BChild), hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipMemsetAsync(bs.ctrl + BC_NCHILD, 0, 8, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  *n = nc;
  ctx->batch_generations++;
  return 0;
}
int smx_d_gen_end(smx_ctx* ctx, void* children_out, uint32_t cap, uint32_t* n) { return d_gen_end_impl(ctx, children_out, cap, n, nullptr); }
// -> [u32 nrec][u32 data bytes][u32 offs[nrec]][records]   (record layout: k_strip_pack_columns)
int smx_d_pack_columns(smx_ctx* ctx, int32_t x0, int32_t x1, void* host_buf, uint64_t cap, uint64_t* bytes) {
  hipStream_t st = ctx->stream;
  if (batch_alloc(ctx, 1, false) || xbuf_alloc(ctx)) return -1;
  if (x0 < 0) x0 = 0; if (x1 > ctx->cfg.dimx) x1 = ctx->cfg.dimx;
  const int gx0 = x0 >> 2, gx1 = (x1 + 3) >> 2, gty = (ctx->cfg.dimy + 3) >> 2;
  HIPCHK(ctx, hipMemsetAsync(ctx->d_xcur, 0, sizeof(XCursor), st));
  const long long nt = (long long)(gx1 - gx0) * gty;
  if (nt > 0) hipLaunchKernelGGL(k_strip_pack_columns, dim3((unsigned)((nt + 63) / 64)), dim3(64), 0, st, ctx->d, ctx->bs, gx0, gx1, ctx->d_xdata, ctx->xdata_cap, ctx->d_xoffs, ctx->xoffs_cap, ctx->d_xcur);
  XCursor c;
  HIPCHK(ctx, hipMemcpyAsync(&c, ctx->d_xcur, sizeof(c), hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  if (c.lost) { ctx->err = "smx_d_pack_columns: exchange buffer too small"; return -2; }
  const uint64_t total = 8 + 4ull * c.nrec + c.bytes;
  if (total > cap) { ctx->err = "smx_d_pack_columns: host buffer too small"; return -2; }
  uint8_t* hb = (uint8_t*)host_buf;
  const uint32_t nb = (uint32_t)c.bytes;
  memcpy(hb, &c.nrec, 4); memcpy(hb + 4, &nb, 4);
  if (c.nrec) HIPCHK(ctx, hipMemcpyAsync(hb + 8, ctx->d_xoffs, 4ull * c.nrec, hipMemcpyDeviceToHost, st));
  if (c.bytes) HIPCHK(ctx, hipMemcpyAsync(hb + 8 + 4ull * c.nrec, ctx->d_xdata, c.bytes, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  *bytes = total;
  return 0;
}
int smx_d_unpack_columns(smx_ctx* ctx, const void* host_buf, uint64_t bytes) {
  hipStream_t st = ctx->stream;
  if (bytes < 8) return 0;
  if (batch_alloc(ctx, 1, false) || xbuf_alloc(ctx)) return -1;
  const uint8_t* hb = (const uint8_t*)host_buf;
  uint32_t nrec, nb; memcpy(&nrec, hb, 4); memcpy(&nb, hb + 4, 4);
  if (nrec == 0) return 0;
  if (nrec > ctx->xoffs_cap || nb > ctx->xdata_cap || 8 + 4ull * nrec + nb > bytes) { ctx->err = "smx_d_unpack_columns: bad buffer"; return -2; }
  for (uint32_t i = 0; i < nrec; i++) {                       // (the kernel follows these offsets and counts: they must stay inside the data)
    uint32_t o, hd[2]; memcpy(&o, hb + 8 + 4ull * i, 4);
    if ((uint64_t)o + 24 > nb) { ctx->err = "smx_d_unpack_columns: record offset outside the buffer"; return -2; }
    memcpy(hd, hb + 8 + 4ull * nrec + o, 8);                  // {cell, section count}
    if (hd[0] >= ctx->ncells || (uint64_t)o + 24 + 32ull * hd[1] > nb) { ctx->err = "smx_d_unpack_columns: bad record"; return -2; }
  }
  HIPCHK(ctx, hipMemcpyAsync(ctx->d_xoffs, hb + 8, 4ull * nrec, hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipMemcpyAsync(ctx->d_xdata, hb + 8 + 4ull * nrec, nb, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_strip_unpack_columns, dim3((nrec + 63u) / 64u), dim3(64), 0, st, ctx->d, ctx->bs, ctx->d_xdata, ctx->d_xoffs, nrec, nb);
  hipLaunchKernelGGL(k_batch_merge_freed, dim3(1), dim3(256), 0, st, ctx->d, ctx->bs);
  HIPCHK(ctx, hipStreamSynchronize(st));
  HIPCHK(ctx, hipGetLastError());
  return 0;
}
int smx_d_pack_particles(smx_ctx* ctx, int32_t x0, int32_t x1, void* host_buf, uint64_t cap, uint64_t* bytes) {
  hipStream_t st = ctx->stream;
  if (xbuf_alloc(ctx)) return -1;
  const uint32_t nslots = ctx->d_nslots;
  const uint64_t rs = 4 + (ctx->d_wind ? sizeof(BWind) : sizeof(BWater));
  HIPCHK(ctx, hipMemsetAsync(ctx->d_xcur, 0, sizeof(XCursor), st));
  if (nslots) LAUNCH_WIND_WATER(ctx->d_wind, k_strip_pack_particles, dim3((nslots + 255u) / 256u), dim3(256), st, ctx->bs, nslots, x0, x1, ctx->d_xdata, ctx->xdata_cap, ctx->d_xcur);
  XCursor c;
  HIPCHK(ctx, hipMemcpyAsync(&c, ctx->d_xcur, sizeof(c), hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  if (c.lost || 4 + c.nrec * rs > cap) { ctx->err = "smx_d_pack_particles: buffer too small"; return -2; }
  uint8_t* hb = (uint8_t*)host_buf;
  memcpy(hb, &c.nrec, 4);
  if (c.nrec) HIPCHK(ctx, hipMemcpyAsync(hb + 4, ctx->d_xdata, c.nrec * rs, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  *bytes = 4 + c.nrec * rs;
  return 0;
}
int smx_d_unpack_particles(smx_ctx* ctx, const void* host_buf, uint64_t bytes) {
  hipStream_t st = ctx->stream;
  if (bytes < 4) return 0;
  if (xbuf_alloc(ctx)) return -1;
  const uint8_t* hb = (const uint8_t*)host_buf;
  uint32_t n; memcpy(&n, hb, 4);
  if (n == 0) return 0;
  const uint64_t rs = 4 + (ctx->d_wind ? sizeof(BWind) : sizeof(BWater));
  if (4 + n * rs > bytes || n * rs > ctx->xdata_cap) { ctx->err = "smx_d_unpack_particles: bad buffer"; return -2; }
  HIPCHK(ctx, hipMemcpyAsync(ctx->d_xdata, hb + 4, n * rs, hipMemcpyHostToDevice, st));
  LAUNCH_WIND_WATER(ctx->d_wind, k_strip_unpack_particles, dim3((n + 255u) / 256u), dim3(256), st, ctx->bs, ctx->d_xdata, n);
  HIPCHK(ctx, hipStreamSynchronize(st));
  return 0;
}
int smx_d_grid_begin(smx_ctx* ctx) {
  hipStream_t st = ctx->stream;
  if (batch_alloc(ctx, 1, false)) return -1;
  ctx->d_wind = false; ctx->d_nslots = 0; ctx->d_first = true;
  HIPCHK(ctx, hipMemsetAsync(ctx->d.active1, 0, (ctx->nw1 + 64) * 8, st));
  HIPCHK(ctx, hipMemsetAsync(ctx->d.active2, 0, (ctx->nw2 + 64) * 8, st));
  HIPCHK(ctx, hipMemsetAsync(ctx->bs.ctrl + BC_NCHILD, 0, 8, st));
  launch_classify(ctx);
  return 0;
}
int smx_d_grid_sweep_cols(smx_ctx* ctx, int32_t phase, int32_t x_lo, int32_t x_hi) {   // the tiles of the COLUMNS [x_lo, x_hi) (multiples of the tile size)
  const int rc = grid_sweep(ctx, phase, x_lo >> GRID_SHIFT, (x_hi + (1 << GRID_SHIFT) - 1) >> GRID_SHIFT);
  if (rc) return rc;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return 0;
}
}  // extern "C"

static bool is_batched(const smx_ctx* ctx) { return ctx->cfg.engine == SMX_ENGINE_BATCHED || ctx->cfg.engine == SMX_ENGINE_RELAXED; }
extern "C" {
// ---------------- the hot path ----------------
int smx_tick_water(smx_ctx* ctx, int32_t nwater) {
  FULLMAP("smx_tick_water (a strip ticks with smx_strips_tick)")
  roctx_range rr("soilmx:water");
  PhaseTimer t(ctx, PH_WATER);
  if (is_batched(ctx)) {
    // throughput engines: the phase's particles as `water_generations` consecutive top-level generations of n/k (smx_set_water_generations;
    // default 1). Particles of one generation advance together and do not see the water the same generation adds; k > 1 trades
    // throughput for the reference's feedback between particles of a tick (profiles/r04_p2_analysis.md). Exactly k phase calls of n/k.
    uint32_t left = nwater > 0 ? (uint32_t)nwater : 0u;
    const uint32_t k = ctx->water_generations < 1 ? 1u : (uint32_t)ctx->water_generations;
    if (ctx->cfg.engine == SMX_ENGINE_RELAXED && ctx->water_stagger > 0 && k > 1u && left > 0u) {
      // STAGGERED generations (smx_set_water_stagger): ONE phase; batch b of ceil(n / k) particles takes its first step in epoch b * gap. A particle of
      // batch b finds what the batches before it have done in the `gap` epochs they are ahead -- the lakes their stopped particles made on the way --, the
      // epoch chain of a tick is (k - 1) * gap + one generation long instead of k generations (relax_water_step)
      ctx->stagger_phase_n = left;
      const int rc = batch_generations(ctx, false, left, 0u);
      ctx->stagger_phase_n = 0u;
      return rc;
    }
    for (uint32_t q = 0; q < k && left > 0; q++) {
      const uint32_t nq = batch_generation_share(left, k, q);
      if (nq) { const int rc = batch_generations(ctx, false, nq, 0u); if (rc) return rc; }
    }
    return 0;
  }
  if (ctx->cfg.engine == SMX_ENGINE_SPECULATIVE) return spec_phase(ctx, nwater, false);
  PhaseTimer tk(ctx, PH_K_WATER);
  hipLaunchKernelGGL(k_water_serial, dim3(1), dim3(64), 0, ctx->stream, ctx->d, nwater);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}
int smx_grid_pass(smx_ctx* ctx) {
  FULLMAP("smx_grid_pass (a strip ticks with smx_strips_tick)")
  roctx_range rr("soilmx:grid");
  PhaseTimer t(ctx, PH_GRID);
  if (is_batched(ctx)) return batch_grid(ctx);
  HIPCHK(ctx, hipMemsetAsync(ctx->d.active1, 0, (ctx->nw1 + 64) * 8, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(ctx->d.active2, 0, (ctx->nw2 + 64) * 8, ctx->stream));
  launch_classify(ctx);
  hipLaunchKernelGGL(k_grid_serial, dim3(1), dim3(64), 0, ctx->stream, ctx->d);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}
int smx_tick_wind(smx_ctx* ctx, int32_t nwind) {
  FULLMAP("smx_tick_wind (a strip ticks with smx_strips_tick)")
  roctx_range rr("soilmx:wind");
  PhaseTimer t(ctx, PH_WIND);
  if (is_batched(ctx)) return batch_generations(ctx, true, nwind > 0 ? (uint32_t)nwind : 0u, 0u);
  if (ctx->cfg.engine == SMX_ENGINE_SPECULATIVE) return spec_phase(ctx, nwind, true);
  PhaseTimer tk(ctx, PH_K_WIND);
  hipLaunchKernelGGL(k_wind_serial, dim3(1), dim3(64), 0, ctx->stream, ctx->d, nwind);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}
int smx_map_frequency(smx_ctx* ctx) {
  roctx_range rr("soilmx:frequency");
  PhaseTimer t(ctx, PH_FREQ);
  const size_t n = ctx->ncells, n4 = n / 4;
  unsigned nb = (unsigned)((n4 + 255) / 256);
  if (nb > 2048) nb = 2048;
  if (nb == 0) nb = 1;
  { PhaseTimer tk(ctx, PH_K_MAPFREQ); hipLaunchKernelGGL(k_map_frequency, dim3(nb), dim3(256), 0, ctx->stream, ctx->d.wfreq, ctx->d.wtrack, n4, n); }
  HIPCHK(ctx, hipGetLastError());
  return 0;
}
int smx_reset_frequency(smx_ctx* ctx) {
  PhaseTimer t(ctx, PH_FREQ);
  HIPCHK(ctx, hipMemsetAsync(ctx->d.wtrack, 0, ctx->ncells * 4, ctx->stream));
  return 0;
}
int smx_tick(smx_ctx* ctx, int32_t nwater, int32_t nwind, int32_t dowater, int32_t dowind) {   // SoilMachine.cpp:283-329
  int rc = 0;                                                 // (a phase's own code comes through: -6 work dropped, -9 a device-side wait gave up, ...)
  if (dowater) { if ((rc = smx_tick_water(ctx, nwater)) != 0) return rc; if ((rc = smx_grid_pass(ctx)) != 0) return rc; }
  if (dowind) { if ((rc = smx_tick_wind(ctx, nwind)) != 0) return rc; }
  if (dowater) { if ((rc = smx_map_frequency(ctx)) != 0) return rc; if ((rc = smx_reset_frequency(ctx)) != 0) return rc; }
  return 0;
}
int smx_sync(smx_ctx* ctx) {
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  HIPCHK(ctx, hipGetLastError());
  return 0;
}
}  // extern "C"

// ---------------- ensembles: many exact contexts, one launch per phase for all of them ----------------
// The members are ordinary SERIAL contexts created on the ensemble's stream (create_range), so a call on a member and a call on the
// ensemble are ordered without events. A tick writes the member table into one slot of a pinned ring, uploads it with one async copy
// and launches the same kernels whatever the member count: k_ens_water, k_ens_grid_clear, k_ens_classify, k_ens_grid, k_ens_wind,
// k_ens_frequency. A ring slot is rewritten only after the copy out of it has run (its event), so the host may run ahead of the stream.
constexpr int ENS_RING = 4;
struct smx_ensemble : EventTimer {
  int device = 0;
  std::string err;
  DevMem mem;                             // owns the tables, the observation scratch and the fork scratch
  std::vector<smx_ctx*> members;          // in order of addition
  uint32_t cap = 0;                       // members the tables are sized for
  EnsEntry* d_tab = nullptr;              // the table the kernels read
  EnsEntry* h_tab = nullptr;              // ENS_RING pinned tables of `cap` entries
  hipEvent_t h_free[ENS_RING] = {};       // recorded after the upload out of ring slot k
  bool h_used[ENS_RING] = {};
  int slot = 0;
  // smx_ensemble_figures / smx_ensemble_plane_stats: results on the device and their pinned landing place (grown on demand, kept)
  void* d_obs = nullptr; size_t d_obs_cap = 0;
  void* h_obs = nullptr; size_t h_obs_cap = 0;
  ForkScratch fork;                       // smx_ensemble_fork
  AnalysisScratch lakes, drain, streams, spill, through, hills, paths;   // smx_ensemble_lakes, _drainage, _streams, _spill, _through, _hillslopes, _flowpaths: one each
  AnalysisScratch disp;                                                  // smx_ensemble_dispersal
  AnalysisScratch catchments;                                            // smx_ensemble_catchments
  AnalysisScratch horizons;                                              // smx_ensemble_horizons
  AnalysisScratch proximity;                                             // smx_ensemble_proximity
  StrataScratch strata;                   // smx_ensemble_soil_totals
  BudgetScratch budget;                   // smx_ensemble_budget
  AnalysisLaunch launch;                  // smx_ensemble_set_analysis_launch
};

static int ens_reserve(smx_ensemble* e, uint32_t n) {   // tables for n members (the old ones are dropped once the stream is idle)
  if (n <= e->cap) return 0;
  uint32_t cap = e->cap ? e->cap : 64u;
  while (cap < n) cap *= 2u;
  if (cap > (uint32_t)SMX_ENSEMBLE_MAX_MEMBERS) cap = (uint32_t)SMX_ENSEMBLE_MAX_MEMBERS;
  HIPCHK(e, hipStreamSynchronize(e->stream));
  EnsEntry* d = nullptr; EnsEntry* h = nullptr;   // the new pair first: the old tables stay if either allocation fails
  if (e->mem.dev(d, cap) != hipSuccess || e->mem.pinned(h, (size_t)ENS_RING * cap) != hipSuccess) {
    e->mem.drop(d);
    (void)hipGetLastError();
    e->err = "smx_ensemble_add: out of memory for the member table";
    return -1;
  }
  e->mem.drop(e->d_tab); e->mem.drop(e->h_tab);
  for (int k = 0; k < ENS_RING; k++) e->h_used[k] = false;
  e->d_tab = d; e->h_tab = h; e->cap = cap;
  return 0;
}

extern "C" {
int smx_ensemble_create(int32_t device, smx_ensemble** out) {
  if (!out) return -2;
  smx_ensemble* e = new smx_ensemble();
  e->device = device;
  *out = e;   // handed out even on failure so the caller can read smx_ensemble_last_error(); smx_ensemble_destroy() is safe
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { e->err = "no HIP device visible (the soilmx product path has no CPU fallback)"; return -3; }
  HIPCHK(e, hipSetDevice(device));
  HIPCHK(e, hipStreamCreate(&e->stream));
  for (int k = 0; k < ENS_RING; k++) HIPCHK(e, hipEventCreateWithFlags(&e->h_free[k], hipEventDisableTiming));
  return 0;
}
void smx_ensemble_destroy(smx_ensemble* e) {
  if (!e) return;
  if (e->stream) hipStreamSynchronize(e->stream);
  for (smx_ctx* m : e->members) { m->ensemble = nullptr; smx_destroy(m); }
  e->members.clear();
  drain_events(e);
  for (hipEvent_t ev : e->evpool) hipEventDestroy(ev);
  for (int k = 0; k < ENS_RING; k++) if (e->h_free[k]) hipEventDestroy(e->h_free[k]);
  e->mem.clear();
  if (e->stream) hipStreamDestroy(e->stream);
  delete e;
}
const char* smx_ensemble_last_error(smx_ensemble* e) { return e ? e->err.c_str() : "null ensemble"; }

int smx_ensemble_add(smx_ensemble* e, const smx_config* cfg, smx_ctx** member) {
  if (!e) return -2;
  if (!cfg || !member) { e->err = "smx_ensemble_add: null argument"; return -2; }
  *member = nullptr;
  if (!e->stream) { e->err = "smx_ensemble_add: the ensemble has no device (smx_ensemble_create failed)"; return -3; }
  if (cfg->engine != SMX_ENGINE_SERIAL) { e->err = "smx_ensemble_add: members run the exact SERIAL engine only (speculative, batched and relaxed contexts are refused)"; return -2; }
  if (cfg->device != e->device) { e->err = "smx_ensemble_add: a member lives on the ensemble's device"; return -2; }
  if (e->members.size() >= (size_t)SMX_ENSEMBLE_MAX_MEMBERS) { e->err = "smx_ensemble_add: SMX_ENSEMBLE_MAX_MEMBERS reached"; return -2; }
  if (int rc = ens_reserve(e, (uint32_t)e->members.size() + 1u)) return rc;
  smx_ctx* ctx = nullptr;
  const int rc = create_range(cfg, 0, cfg->dimx, e->stream, &ctx);
  if (rc != 0) {
    e->err = std::string("smx_ensemble_add: ") + (ctx ? ctx->err : std::string("invalid configuration (dims, pool_capacity)"));
    if (ctx) smx_destroy(ctx);              // (not yet a member: frees what was allocated, leaves the ensemble's stream alone)
    (void)hipGetLastError();                // an out-of-memory failure must not surface in the next tick's launch check
    return rc;
  }
  ctx->ensemble = e;
  e->members.push_back(ctx);
  *member = ctx;
  return 0;
}
int smx_ensemble_remove(smx_ensemble* e, smx_ctx* member) {
  if (!e) return -2;
  auto it = std::find(e->members.begin(), e->members.end(), member);
  if (!member || it == e->members.end()) { e->err = "smx_ensemble_remove: not a member of this ensemble"; return -2; }
  HIPCHK(e, hipStreamSynchronize(e->stream));   // (no queued tick still reads the member's state)
  e->members.erase(it);
  member->ensemble = nullptr;
  smx_destroy(member);
  return 0;
}
int smx_ensemble_size(smx_ensemble* e, int32_t* n) {
  if (!e || !n) return -2;
  *n = (int32_t)e->members.size();
  return 0;
}

int smx_ensemble_tick(smx_ensemble* e, const int32_t* nwater, const int32_t* nwind, int32_t dowater, int32_t dowind) {   // SoilMachine.cpp:283-329 per member
  if (!e) return -2;
  if (!nwater) { e->err = "smx_ensemble_tick: nwater is null (one count per member; < 0 = the member sits the tick out)"; return -2; }
  if (dowind && !nwind) { e->err = "smx_ensemble_tick: nwind is null while dowind is set"; return -2; }
  const uint32_t nm = (uint32_t)e->members.size();
  if (nm == 0) return 0;
  for (uint32_t i = 0; i < nm; i++)
    if (e->members[i]->cfg.engine != SMX_ENGINE_SERIAL) { e->err = "smx_ensemble_tick: member " + std::to_string(i) + " was switched off the SERIAL engine (smx_set_engine)"; return -2; }
  roctx_range rr("soilmx:ensemble");
  const int k = e->slot;
  e->slot = (e->slot + 1) % ENS_RING;
  if (e->h_used[k]) HIPCHK(e, hipEventSynchronize(e->h_free[k]));   // the copy out of this slot has run
  EnsEntry* h = e->h_tab + (size_t)k * e->cap;
  size_t cls_blocks = 1, freq_blocks = 1;
  for (uint32_t i = 0; i < nm; i++) {
    const smx_ctx* c = e->members[i];
    EnsEntry& t = h[i];
    t.s = c->d;
    t.nwater = nwater[i];
    t.nwind = dowind ? nwind[i] : 0;
    t.on = nwater[i] >= 0;
    t.classify8 = c->cfg.dimy % 8 == 0 && c->lcells % 64 == 0;   // (launch_classify; a member holds the whole map: c_lo = 0)
    if (!t.on) continue;
    cls_blocks = std::max(cls_blocks, t.classify8 ? (c->lcells / 8 + 255) / 256 : (c->lcells + 255) / 256);
    freq_blocks = std::max(freq_blocks, std::min<size_t>(2048, (c->ncells / 4 + 255) / 256));
  }
  HIPCHK(e, hipMemcpyAsync(e->d_tab, h, (size_t)nm * sizeof(EnsEntry), hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipEventRecord(e->h_free[k], e->stream));
  e->h_used[k] = true;
  hipStream_t st = e->stream;
  const EnsEntry* tab = e->d_tab;
  if (dowater) {
    {
      PhaseTimer t(e, PH_WATER);
      PhaseTimer tk(e, PH_K_WATER);
      hipLaunchKernelGGL(k_ens_water, dim3(nm), dim3(64), 0, st, tab);
    }
    {
      PhaseTimer t(e, PH_GRID);
      hipLaunchKernelGGL(k_ens_grid_clear, dim3(nm), dim3(256), 0, st, tab);
      { PhaseTimer tk(e, PH_K_CLASSIFY); hipLaunchKernelGGL(k_ens_classify, dim3((unsigned)cls_blocks, nm), dim3(256), 0, st, tab); }
      hipLaunchKernelGGL(k_ens_grid, dim3(nm), dim3(64), 0, st, tab);
    }
  }
  if (dowind) {
    PhaseTimer t(e, PH_WIND);
    PhaseTimer tk(e, PH_K_WIND);
    hipLaunchKernelGGL(k_ens_wind, dim3(nm), dim3(64), 0, st, tab);
  }
  if (dowater) {
    PhaseTimer t(e, PH_FREQ);
    PhaseTimer tk(e, PH_K_MAPFREQ);
    hipLaunchKernelGGL(k_ens_frequency, dim3((unsigned)freq_blocks, nm), dim3(256), 0, st, tab);
  }
  HIPCHK(e, hipGetLastError());
  return 0;
}
int smx_ensemble_sync(smx_ensemble* e) {
  if (!e || !e->stream) return -2;
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipGetLastError());
  return 0;
}
int smx_ensemble_get_timing(smx_ensemble* e, smx_timing* out, uint64_t struct_size) {
  if (!e || !out || !e->stream) return -2;
  HIPCHK(e, hipStreamSynchronize(e->stream));
  drain_events(e);
  memcpy(out, &e->timing, struct_size < sizeof(e->timing) ? (size_t)struct_size : sizeof(e->timing));
  return 0;
}
int smx_ensemble_timing_reset(smx_ensemble* e) {
  if (!e || !e->stream) return -2;
  HIPCHK(e, hipStreamSynchronize(e->stream));
  drain_events(e);
  memset(&e->timing, 0, sizeof(e->timing));
  return 0;
}

// ---------------- an ensemble observed in one call ----------------
// Both calls: one table upload (the ring protocol of smx_ensemble_tick), the kernels, one copy back, one synchronisation -- whatever
// the member count. They read the members' states on the ensemble's stream, behind every tick queued before them.
static_assert(sizeof(smx_member_figures) == 80 && offsetof(ObsFigures, corrupt) == sizeof(smx_member_figures), "smx_member_figures layout");
static_assert(SMX_PLANE_HEIGHT == OBS_PLANE_HEIGHT && SMX_PLANE_WATER == OBS_PLANE_WATER && SMX_PLANE_WFREQ == OBS_PLANE_WFREQ &&
              SMX_PLANE_WINDFREQ == OBS_PLANE_WINDFREQ, "SMX_PLANE_*");

// the members sel[0..n) as entries 0..n-1 of the device table
static int ens_upload_selection(smx_ensemble* e, const uint32_t* sel, uint32_t n) {
  const int k = e->slot;
  e->slot = (e->slot + 1) % ENS_RING;
  if (e->h_used[k]) HIPCHK(e, hipEventSynchronize(e->h_free[k]));   // the copy out of this slot has run
  EnsEntry* h = e->h_tab + (size_t)k * e->cap;
  for (uint32_t i = 0; i < n; i++) {
    EnsEntry& t = h[i];
    t.s = e->members[sel ? sel[i] : i]->d;
    t.nwater = 0; t.nwind = 0; t.on = 0; t.classify8 = 0;
  }
  HIPCHK(e, hipMemcpyAsync(e->d_tab, h, (size_t)n * sizeof(EnsEntry), hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipEventRecord(e->h_free[k], e->stream));
  e->h_used[k] = true;
  return 0;
}
static int ens_obs_reserve(smx_ensemble* e, size_t bytes) {
  if (bytes <= e->d_obs_cap && bytes <= e->h_obs_cap) return 0;
  size_t cap = e->d_obs_cap ? e->d_obs_cap : 4096;
  while (cap < bytes) cap *= 2;
  HIPCHK(e, hipStreamSynchronize(e->stream));
  void* d = nullptr; void* h = nullptr;   // (as ens_reserve: the old pair stays if either allocation fails)
  if (e->mem.dev(d, cap) != hipSuccess || e->mem.pinned(h, cap) != hipSuccess) {
    e->mem.drop(d);
    (void)hipGetLastError();
    e->err = "out of memory for the observation scratch (" + std::to_string(cap) + " bytes)";
    return -1;
  }
  e->mem.drop(e->d_obs); e->mem.drop(e->h_obs);
  e->d_obs = d; e->h_obs = h; e->d_obs_cap = cap; e->h_obs_cap = cap;
  return 0;
}

int smx_ensemble_figures(smx_ensemble* e, smx_member_figures* out, uint64_t struct_size) {
  if (!e) return -2;
  if (!e->stream) { e->err = "smx_ensemble_figures: the ensemble has no device (smx_ensemble_create failed)"; return -3; }
  const uint32_t nm = (uint32_t)e->members.size();
  if (nm == 0) return 0;
  if (!out) { e->err = "smx_ensemble_figures: out is null (one entry per member)"; return -2; }
  roctx_range rr("soilmx:ensemble_figures");
  if (int rc = ens_obs_reserve(e, (size_t)nm * sizeof(ObsFigures))) { e->err = "smx_ensemble_figures: " + e->err; return rc; }
  if (int rc = ens_upload_selection(e, nullptr, nm)) return rc;
  hipLaunchKernelGGL(k_ens_figures, dim3(nm), dim3(FIG_LANES), 0, e->stream, e->d_tab, (ObsFigures*)e->d_obs);
  HIPCHK(e, hipGetLastError());
  HIPCHK(e, hipMemcpyAsync(e->h_obs, e->d_obs, (size_t)nm * sizeof(ObsFigures), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  const ObsFigures* r = (const ObsFigures*)e->h_obs;
  for (uint32_t i = 0; i < nm; i++)
    if (r[i].corrupt) { e->err = "smx_ensemble_figures: corrupt section chain in member " + std::to_string(i); return -5; }
  const size_t take = struct_size < sizeof(smx_member_figures) ? (size_t)struct_size : sizeof(smx_member_figures);
  for (uint32_t i = 0; i < nm; i++) memcpy(reinterpret_cast<char*>(out) + (size_t)i * struct_size, &r[i], take);
  return 0;
}

int smx_ensemble_plane_stats(smx_ensemble* e, int32_t plane, const int32_t* which, int32_t n, double* mean, double* var, double* vmin,
                             double* vmax, uint32_t* nonzero) {
  if (!e) return -2;
  if (!e->stream) { e->err = "smx_ensemble_plane_stats: the ensemble has no device (smx_ensemble_create failed)"; return -3; }
  if (plane < SMX_PLANE_HEIGHT || plane > SMX_PLANE_WINDFREQ) { e->err = "smx_ensemble_plane_stats: unknown plane " + std::to_string(plane); return -2; }
  const uint32_t nm = (uint32_t)e->members.size();
  if (!which) n = (int32_t)nm;
  if (n <= 0) { e->err = which ? "smx_ensemble_plane_stats: n = " + std::to_string(n) + ": no member selected" : std::string("smx_ensemble_plane_stats: the ensemble has no members"); return -2; }
  if ((uint32_t)n > nm) { e->err = "smx_ensemble_plane_stats: n = " + std::to_string(n) + " members selected, the ensemble has " + std::to_string(nm) + " (no member may be selected twice)"; return -2; }
  std::vector<uint32_t> sel((size_t)n);
  std::vector<char> seen(nm, 0);
  for (int32_t i = 0; i < n; i++) {
    const int64_t w = which ? (int64_t)which[i] : (int64_t)i;
    if (w < 0 || w >= (int64_t)nm) { e->err = "smx_ensemble_plane_stats: which[" + std::to_string(i) + "] = " + std::to_string(w) + " is not a member index (the ensemble has " + std::to_string(nm) + ")"; return -2; }
    if (seen[(size_t)w]) { e->err = "smx_ensemble_plane_stats: member " + std::to_string(w) + " is selected twice (which[" + std::to_string(i) + "])"; return -2; }
    seen[(size_t)w] = 1;
    sel[(size_t)i] = (uint32_t)w;
  }
  const smx_config& c0 = e->members[sel[0]]->cfg;
  for (int32_t i = 1; i < n; i++) {
    const smx_config& c = e->members[sel[(size_t)i]]->cfg;
    if (c.dimx != c0.dimx || c.dimy != c0.dimy) {
      e->err = "smx_ensemble_plane_stats: member " + std::to_string(sel[(size_t)i]) + " is " + std::to_string(c.dimx) + "x" + std::to_string(c.dimy) + ", member " +
               std::to_string(sel[0]) + " is " + std::to_string(c0.dimx) + "x" + std::to_string(c0.dimy) + ": the selected members must have equal dims";
      return -2;
    }
  }
  const size_t cells = (size_t)c0.dimx * c0.dimy;
  // the wanted outputs, one after the other in the scratch (f64 planes first: all offsets stay 8-byte aligned)
  double** const want[4] = {&mean, &var, &vmin, &vmax};
  size_t off[5], bytes = 0;
  for (int k = 0; k < 4; k++) { off[k] = bytes; if (*want[k]) bytes += cells * sizeof(double); }
  off[4] = bytes;
  if (nonzero) bytes += cells * sizeof(uint32_t);
  if (bytes == 0) return 0;
  roctx_range rr("soilmx:ensemble_plane_stats");
  if (int rc = ens_obs_reserve(e, bytes)) { e->err = "smx_ensemble_plane_stats: " + e->err; return rc; }
  if (int rc = ens_upload_selection(e, sel.data(), (uint32_t)n)) return rc;
  char* d = (char*)e->d_obs;
  double* dp[4];
  for (int k = 0; k < 4; k++) dp[k] = *want[k] ? reinterpret_cast<double*>(d + off[k]) : nullptr;
  uint32_t* dnz = nonzero ? reinterpret_cast<uint32_t*>(d + off[4]) : nullptr;
  const dim3 grid((unsigned)((cells + 255) / 256)), block(256);
  switch (plane) {
    case SMX_PLANE_HEIGHT: hipLaunchKernelGGL(k_ens_plane_stats<OBS_PLANE_HEIGHT>, grid, block, 0, e->stream, e->d_tab, (uint32_t)n, cells, dp[0], dp[1], dp[2], dp[3], dnz); break;
    case SMX_PLANE_WATER: hipLaunchKernelGGL(k_ens_plane_stats<OBS_PLANE_WATER>, grid, block, 0, e->stream, e->d_tab, (uint32_t)n, cells, dp[0], dp[1], dp[2], dp[3], dnz); break;
    case SMX_PLANE_WFREQ: hipLaunchKernelGGL(k_ens_plane_stats<OBS_PLANE_WFREQ>, grid, block, 0, e->stream, e->d_tab, (uint32_t)n, cells, dp[0], dp[1], dp[2], dp[3], dnz); break;
    default: hipLaunchKernelGGL(k_ens_plane_stats<OBS_PLANE_WINDFREQ>, grid, block, 0, e->stream, e->d_tab, (uint32_t)n, cells, dp[0], dp[1], dp[2], dp[3], dnz); break;
  }
  HIPCHK(e, hipGetLastError());
  HIPCHK(e, hipMemcpyAsync(e->h_obs, e->d_obs, bytes, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  const char* h = (const char*)e->h_obs;
  for (int k = 0; k < 4; k++) if (*want[k]) memcpy(*want[k], h + off[k], cells * sizeof(double));
  if (nonzero) memcpy(nonzero, h + off[4], cells * sizeof(uint32_t));
  return 0;
}

// ---------------- forking a map on the device (smx_copy_state / smx_ensemble_fork; kernels: soil_fork.h) ----------------
// Both calls: k_fork_count, rocPRIM's exclusive scan and one 24-byte copy back decide -4 / -5 before anything is written or allocated;
// then k_fork_scatter and k_fork_planes write every destination (blockIdx.y) -- the same launches whatever the member count.
// (`m`: the owner the scratch lives in -- the destination context's or the ensemble's)
static int fork_reserve(ForkScratch& f, DevMem& m, size_t ncells, uint32_t ntab, hipStream_t st, std::string& err) {
  bool ok = true;
  if (ncells > f.cells || !f.tot) {
    if (hipStreamSynchronize(st) != hipSuccess) ok = false;
    m.drop(f.buried); m.drop(f.base); m.drop(f.flag); m.drop(f.temp); m.drop(f.tot); f.cells = 0; f.temp_bytes = 0;
    size_t tb = 0;
    ok = ok && rocprim::exclusive_scan(nullptr, tb, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, ncells, rocprim::plus<uint32_t>(), st) == hipSuccess;
    ok = ok && m.dev(f.buried, ncells) == hipSuccess && m.dev(f.base, ncells) == hipSuccess && m.dev(f.flag, ncells) == hipSuccess &&
         m.dev(f.tot, 1) == hipSuccess && m.dev(f.temp, tb ? tb : 8) == hipSuccess;
    if (ok) { f.cells = ncells; f.temp_bytes = tb; }
  }
  if (ok && ntab > f.tab_cap) ok = hipStreamSynchronize(st) == hipSuccess && m.grow(f.tab, f.tab_cap, ntab, ntab) == hipSuccess;
  if (ok) return 0;
  (void)hipGetLastError();   // nothing half-sized stays behind
  m.drop(f.buried); m.drop(f.base); m.drop(f.flag); m.drop(f.tot); m.drop(f.temp); m.drop(f.tab);
  f = ForkScratch(); err = "out of device memory for the fork scratch"; return -1;
}
static ForkSrc fork_src(const smx_ctx* src) {
  ForkSrc s;
  s.cells = src->d.cells; s.pool = src->d.pool; s.flags = src->d.flags;
  s.wfreq = src->d.wfreq; s.wtrack = src->d.wtrack; s.windfreq = src->d.windfreq;
  s.soils = src->d_soils; s.rnd = src->d.rnd;
  s.cap = src->cfg.pool_capacity; s.ncells = src->ncells; s.nsoils = (uint32_t)src->nsoils;
  return s;
}
static ForkDst fork_dst(const smx_ctx* c, bool seeded, uint32_t seed) {
  ForkDst d;
  d.cells = c->d.cells; d.pool = c->d.pool; d.freelist = c->d.freelist; d.free_count = c->d.free_count; d.flags = c->d.flags;
  d.wfreq = c->d.wfreq; d.wtrack = c->d.wtrack; d.windfreq = c->d.windfreq;
  d.soils = c->d_soils; d.rnd = c->d.rnd; d.ctr = c->d.ctr;
  d.cap = c->cfg.pool_capacity; d.seeded = seeded ? 1u : 0u; d.seed = seed;
  return d;
}
// the work queued on src's stream happens before what `st` is given from here on
static int fork_order(smx_ctx* src, hipStream_t st, std::string& err) {
  if (src->stream == st) return 0;
  hipEvent_t ev;
  if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) { err = "hipEventCreateWithFlags failed"; return -1; }
  const bool ok = hipEventRecord(ev, src->stream) == hipSuccess && hipStreamWaitEvent(st, ev, 0) == hipSuccess;
  hipEventDestroy(ev);   // (released once the wait has passed it)
  if (!ok) { err = "could not order the copy behind the source's stream"; return -1; }
  return 0;
}
// count + scan on `st`, the totals back, the verdict for a destination pool of dst_cap sections (the text goes to err)
static int fork_measure(const char* who, smx_ctx* src, ForkScratch& f, DevMem& m, hipStream_t st, uint64_t dst_cap, ForkTotals& tot, std::string& err) {
  const ForkSrc s = fork_src(src);
  const ForkTotals zero = {0ull, 0ull, FORK_NONE};
  const unsigned nb = (unsigned)((s.ncells + FORK_LANES - 1) / FORK_LANES);
  bool ok = hipMemcpyAsync(f.tot, &zero, sizeof(zero), hipMemcpyHostToDevice, st) == hipSuccess;
  hipLaunchKernelGGL(k_fork_count, dim3(nb), dim3(FORK_LANES), 0, st, s, f.buried, f.flag, f.tot);
  size_t tb = 0;   // (what THIS size needs: the scratch was sized for the largest map so far)
  ok = ok && rocprim::exclusive_scan(nullptr, tb, f.buried, f.base, 0u, (size_t)s.ncells, rocprim::plus<uint32_t>(), st) == hipSuccess;
  if (ok && tb > f.temp_bytes) {
    ok = hipStreamSynchronize(st) == hipSuccess && m.grow(f.temp, f.temp_bytes, tb, tb) == hipSuccess;
  }
  ok = ok && rocprim::exclusive_scan(f.temp, tb, f.buried, f.base, 0u, (size_t)s.ncells, rocprim::plus<uint32_t>(), st) == hipSuccess;
  ok = ok && hipMemcpyAsync(&tot, f.tot, sizeof(tot), hipMemcpyDeviceToHost, st) == hipSuccess;
  ok = ok && hipStreamSynchronize(st) == hipSuccess && hipGetLastError() == hipSuccess;
  if (!ok) { err = std::string(who) + ": counting the source's sections failed on the device"; return -1; }
  const int v = fork_verdict(tot, dst_cap);
  if (v == -5) {
    const unsigned long long c = tot.bad;
    err = std::string(who) + ": corrupt section chain in the source, cell " + std::to_string(c) + " (x " + std::to_string(c / (unsigned long long)src->cfg.dimy) + ", y " +
          std::to_string(c % (unsigned long long)src->cfg.dimy) + "): it leaves the pool or has more links than the pool holds";
  } else if (v == -4) {
    err = std::string(who) + ": the source holds " + std::to_string(tot.used + tot.nonempty) + " live sections, more than the destination's pool_capacity " + std::to_string(dst_cap);
  }
  return v;
}
// scatter + planes for ntab destinations of the table (tab == null: `one`); asynchronous on `st`
static void fork_write(smx_ctx* src, const ForkScratch& f, hipStream_t st, const ForkTotals& tot, const ForkDst* tab, uint32_t ntab, const ForkDst& one) {
  const ForkSrc s = fork_src(src);
  const unsigned nb = (unsigned)((s.ncells + FORK_LANES - 1) / FORK_LANES);
  hipLaunchKernelGGL(k_fork_scatter, dim3(nb, ntab), dim3(FORK_LANES), 0, st, s, f.buried, f.base, f.flag, tot, tab, one);
  const unsigned pb = (unsigned)std::min<size_t>(2048, (s.ncells / 4 + 255) / 256 + 1);
  hipLaunchKernelGGL(k_fork_planes, dim3(pb, ntab), dim3(256), 0, st, s, tab, one);
}
static void fork_adopt(smx_ctx* dst, const smx_ctx* src) {   // what smx_set_soils and smx_load leave in the host's copy
  dst->nsoils = src->nsoils; dst->d.nsoils = src->d.nsoils;
  dst->d.scale = src->d.scale; dst->cfg.scale = src->d.scale;
}

int smx_copy_state(smx_ctx* dst, smx_ctx* src) {
  if (!dst) return -2;
  smx_ctx* ctx = dst;
  if (!src) { ctx->err = "smx_copy_state: src is null"; return -2; }
  if (dst == src) { ctx->err = "smx_copy_state: dst and src are the same context"; return -2; }
  if (src->partial() || dst->partial()) { ctx->err = "smx_copy_state: not available on a strip context (smx_create_strip): it holds only a part of the map"; return -2; }
  if (src->cfg.dimx != dst->cfg.dimx || src->cfg.dimy != dst->cfg.dimy) {
    ctx->err = "smx_copy_state: dst is " + std::to_string(dst->cfg.dimx) + "x" + std::to_string(dst->cfg.dimy) + ", src is " + std::to_string(src->cfg.dimx) + "x" +
               std::to_string(src->cfg.dimy) + ": the dims must be equal";
    return -2;
  }
  if (src->cfg.device != dst->cfg.device) { ctx->err = "smx_copy_state: dst and src live on different devices"; return -2; }
  if (!src->stream || !dst->stream) { ctx->err = "smx_copy_state: a context without a device"; return -3; }
  roctx_range rr("soilmx:copy_state");
  HIPCHK(ctx, hipSetDevice(dst->cfg.device));
  std::string why;
  if (fork_reserve(dst->fork, dst->mem, src->ncells, 0, dst->stream, why)) { ctx->err = "smx_copy_state: " + why; return -1; }
  if (fork_order(src, dst->stream, why)) { ctx->err = "smx_copy_state: " + why; return -1; }
  ForkTotals tot;
  if (int rc = fork_measure("smx_copy_state", src, dst->fork, dst->mem, dst->stream, dst->cfg.pool_capacity, tot, why)) { ctx->err = why; return rc; }
  fork_write(src, dst->fork, dst->stream, tot, nullptr, 1, fork_dst(dst, false, 0));
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipStreamSynchronize(dst->stream));
  fork_adopt(dst, src);
  return 0;
}

int smx_ensemble_fork(smx_ensemble* e, smx_ctx* src, int32_t n, uint64_t pool_capacity, const uint32_t* seeds, smx_ctx** members) {
  if (!e) return -2;
  if (!src || !members) { e->err = "smx_ensemble_fork: null argument"; return -2; }
  if (!e->stream) { e->err = "smx_ensemble_fork: the ensemble has no device (smx_ensemble_create failed)"; return -3; }
  if (n <= 0) { e->err = "smx_ensemble_fork: n = " + std::to_string(n) + ": at least one member"; return -2; }
  if (e->members.size() + (size_t)n > (size_t)SMX_ENSEMBLE_MAX_MEMBERS) {
    e->err = "smx_ensemble_fork: " + std::to_string(e->members.size()) + " members + " + std::to_string(n) + " would pass SMX_ENSEMBLE_MAX_MEMBERS (" + std::to_string((int)SMX_ENSEMBLE_MAX_MEMBERS) + ")";
    return -2;
  }
  if (src->partial()) { e->err = "smx_ensemble_fork: the source is a strip context (smx_create_strip): it holds only a part of the map"; return -2; }
  if (src->cfg.device != e->device || !src->stream) { e->err = "smx_ensemble_fork: the source lives on another device than the ensemble"; return -2; }
  smx_config cfg = src->cfg;
  cfg.scale = src->d.scale; cfg.engine = SMX_ENGINE_SERIAL; cfg.device = e->device; cfg.reserved = 0;
  if (pool_capacity) cfg.pool_capacity = pool_capacity;
  if (cfg.pool_capacity >= 0x7FFFFFFFull) { e->err = "smx_ensemble_fork: pool_capacity " + std::to_string(cfg.pool_capacity) + " is out of range"; return -2; }
  roctx_range rr("soilmx:ensemble_fork");
  HIPCHK(e, hipSetDevice(e->device));
  std::string why;
  if (fork_reserve(e->fork, e->mem, src->ncells, (uint32_t)n, e->stream, why)) { e->err = "smx_ensemble_fork: " + why; return -1; }
  if (fork_order(src, e->stream, why)) { e->err = "smx_ensemble_fork: " + why; return -1; }
  ForkTotals tot;
  if (int rc = fork_measure("smx_ensemble_fork", src, e->fork, e->mem, e->stream, cfg.pool_capacity, tot, why)) { e->err = why; return rc; }
  if (int rc = ens_reserve(e, (uint32_t)e->members.size() + (uint32_t)n)) { e->err = "smx_ensemble_fork: " + e->err; return rc; }
  std::vector<smx_ctx*> made;
  std::vector<ForkDst> tab;
  made.reserve((size_t)n); tab.reserve((size_t)n);
  int rc = 0;
  for (int32_t i = 0; i < n && rc == 0; i++) {
    smx_ctx* ctx = nullptr;
    rc = create_range(&cfg, 0, cfg.dimx, e->stream, &ctx, true);
    if (rc != 0) {
      e->err = "smx_ensemble_fork: member " + std::to_string(i) + " of " + std::to_string(n) + ": " + (ctx ? ctx->err : std::string("invalid configuration")) + " (the members made by this call were freed)";
      if (ctx) smx_destroy(ctx);
      break;
    }
    made.push_back(ctx);
    tab.push_back(fork_dst(ctx, seeds != nullptr, seeds ? seeds[i] : 0u));
  }
  if (rc == 0) {
    bool ok = hipMemcpyAsync(e->fork.tab, tab.data(), tab.size() * sizeof(ForkDst), hipMemcpyHostToDevice, e->stream) == hipSuccess;
    if (ok) fork_write(src, e->fork, e->stream, tot, e->fork.tab, (uint32_t)n, ForkDst{});
    ok = ok && hipGetLastError() == hipSuccess && hipStreamSynchronize(e->stream) == hipSuccess;
    if (!ok) { e->err = "smx_ensemble_fork: writing the members failed on the device (the members made by this call were freed)"; rc = -1; }
  }
  if (rc != 0) {
    hipStreamSynchronize(e->stream);
    for (smx_ctx* c : made) smx_destroy(c);   // (not yet members: frees what was allocated, leaves the ensemble's stream alone)
    (void)hipGetLastError();                  // an out-of-memory failure must not surface in the next tick's launch check
    return rc;
  }
  for (int32_t i = 0; i < n; i++) {
    fork_adopt(made[(size_t)i], src);
    made[(size_t)i]->ensemble = e;
    e->members.push_back(made[(size_t)i]);
    members[i] = made[(size_t)i];
  }
  return 0;
}

}  // extern "C"

// ---------------- the terrain analyses: the lake census, drainage, the stream network, spill, through-drainage, the hillslopes, the flow paths ----------------
// (smx_lakes, smx_drainage, smx_streams, smx_spill, smx_through, smx_hillslopes, smx_flowpaths, smx_catchments, smx_horizons, smx_proximity and
// their smx_ensemble_* twins; kernels: soil_lakes.h, soil_drain.h, soil_streams.h, soil_spill.h, soil_through.h, soil_hills.h,
// soil_paths.h, soil_catch.h, soil_horizon.h, soil_prox.h)
// One path per analysis for a context and for an ensemble: the maps ms[0..nm) share the planes (member i at words [off_i, off_i +
// cells_i)), one table upload, the same launches whatever the maps hold and however many there are. What the five have in common
// stands once, here: the call and its argument checks, the member table, the growth of the scratch (AnalysisScratch, soil_scratch.h),
// the drainage chain, the sweep loop and the record cut. Each *_run below says what is particular to it: which planes, which kernels
// behind the shared chain, which planes go back. Every analysis has a scratch of its own, so the results of the sibling calls are
// not touched.
struct AnalysisCall {   // who runs an analysis: a context (its one map) or an ensemble (its members)
  const char* who; bool ensemble, partial;
  DevMem& mem; hipStream_t st; smx_ctx* const* ms; uint32_t nm; std::string& err;
  AnalysisLaunch& launch;   // the owner's (smx_set_analysis_launch)
};
static AnalysisCall call_on(const char* who, smx_ctx*& ctx) { return {who, false, ctx->partial(), ctx->mem, ctx->stream, &ctx, 1u, ctx->err, ctx->launch}; }
static AnalysisCall call_on(const char* who, smx_ensemble* e) { return {who, true, false, e->mem, e->stream, e->members.data(), (uint32_t)e->members.size(), e->err, e->launch}; }

// The argument checks of the analyses' entry points, in the order they have always had -- an ensemble is asked for its device first, a
// context last; an empty ensemble is done (rc 0) before its counts pointer is looked at. false: the
// entry point returns rc. (record: the name of the public struct; threshold: smx_streams' only)
static bool analysis_begin(const AnalysisCall& c, const char* record, const char* counts_name, uint64_t struct_size, const uint32_t* threshold, const void* counts,
                           const void* out, uint32_t cap, int& rc) {
  auto no = [&](int code, const std::string& why) { c.err = std::string(c.who) + ": " + why; rc = code; return false; };
  if (c.ensemble && !c.st) return no(-3, "the ensemble has no device (smx_ensemble_create failed)");
  if (c.partial) return no(-2, "not available on a strip context (smx_create_strip): it holds only a part of the map");
  if (struct_size == 0) return no(-2, std::string("struct_size is 0 (pass sizeof(") + record + ") of the header you compiled against)");
  if (threshold && *threshold == 0) return no(-2, "threshold is 0 (a channel cell has an area of at least threshold >= 1)");
  if (c.ensemble && c.nm == 0) { rc = 0; return false; }
  if (!counts) return no(-2, std::string(counts_name) + " is null (one count per map)");
  if (!out && cap) return no(-2, "out is null while cap is " + std::to_string(cap) + " (out may be null for counting, with cap 0)");
  if (!c.st) return no(-3, "a context without a device");
  return true;
}

// The member table of a call and what its launches share: the planes' length, the records' number, the grids. A map keeps min(cap,
// the most it can hold) records: a lake per 2 x 2 block (its four cells are one lake); a basin or a segment per cell (a plateau);
// none yet for spill and through, whose basins are counted by the chain first (plan_basins).
enum CapRule { CAP_BLOCKS, CAP_CELLS, CAP_LATER };
struct AnalysisPlan {
  std::vector<LakeMember> tab;
  uint64_t words = 0, nrec = 0;
  uint32_t most = 0;                // plan_basins: the largest basin count of a map
  dim3 gt, gf, gs, gb, gr;          // tiles, LAKE_LANES cells a workgroup, the statistics' cells a workgroup; plan_basins: basins, relax sweeps
  const dim3 wg{LAKE_LANES};
};
static int plan_members(const AnalysisCall& c, uint32_t cap, CapRule rule, AnalysisPlan& pl) {
  pl.tab.resize(c.nm);
  size_t tiles = 1, flat = 1, stat = 1;
  const size_t per = lake_stats_cells(LAKE_SLOTS, LAKE_LANES);
  for (uint32_t i = 0; i < c.nm; i++) {
    const smx_ctx* x = c.ms[i];
    if (x->cfg.dimx > 65536 || x->cfg.dimy > 65536) { c.err = std::string(c.who) + ": a map of more than 65536 cells a side (the bounding boxes are 16-bit)"; return -2; }
    LakeMember& m = pl.tab[i];
    m.cells = x->d.cells; m.dimx = x->cfg.dimx; m.dimy = x->cfg.dimy; m.pad = 0u;
    m.off = (uint32_t)pl.words; m.rec0 = (uint32_t)pl.nrec;
    const uint64_t most = rule == CAP_BLOCKS ? (uint64_t)((m.dimx + 1) / 2) * (uint64_t)((m.dimy + 1) / 2) : rule == CAP_CELLS ? (uint64_t)x->ncells : 0u;
    m.cap = (uint32_t)std::min<uint64_t>(cap, most);
    pl.words += (uint64_t)x->ncells; pl.nrec += m.cap;
    if (pl.words > 0xFFFFFFFEull || pl.nrec > 0xFFFFFFFEull) { c.err = std::string(c.who) + ": more than 2^32 - 2 cells (or records) in one call"; return -2; }
    tiles = std::max<size_t>(tiles, lake_tiles(m, LAKE_TX, LAKE_TY));
    flat = std::max<size_t>(flat, (x->ncells + LAKE_LANES - 1) / LAKE_LANES);
    stat = std::max<size_t>(stat, (x->ncells + per - 1) / per);
  }
  pl.gt = dim3((unsigned)tiles, c.nm); pl.gf = dim3((unsigned)flat, c.nm); pl.gs = dim3((unsigned)stat, c.nm);
  return 0;
}
static void plan_basins(const AnalysisCall& c, AnalysisPlan& pl, const uint32_t* counts) {   // spill and through, the chain's counts back: a record for every basin
  pl.nrec = 0; pl.most = 0;
  for (LakeMember& m : pl.tab) { m.cap = *counts++; m.rec0 = (uint32_t)pl.nrec; pl.nrec += m.cap; pl.most = std::max(pl.most, m.cap); }
  pl.gb = dim3((unsigned)(((size_t)pl.most + LAKE_LANES - 1) / LAKE_LANES), pl.gt.y); pl.gr = dim3(std::min<unsigned>(pl.gf.x, c.launch.cap(LAUNCH_RELAX)), pl.gt.y);
  c.launch.grid[LAUNCH_RELAX] = pl.gr.x;
}
// the plan's table into half `half` of the pinned tables (bare: every cap 0), and `halves` halves from `half` on to the device
static void put_table(AnalysisScratch& k, const AnalysisPlan& pl, uint32_t half, bool bare) {
  LakeMember* h = k.h_tab + (size_t)half * pl.tab.size();
  memcpy(h, pl.tab.data(), pl.tab.size() * sizeof(LakeMember));
  if (bare) for (size_t i = 0; i < pl.tab.size(); i++) h[i].cap = 0u;
}
static bool send_tables(const AnalysisCall& c, AnalysisScratch& k, uint32_t half, uint32_t halves) {
  const size_t at = (size_t)half * c.nm;
  return hipMemcpyAsync(k.d_tab + at, k.h_tab + at, (size_t)halves * c.nm * sizeof(LakeMember), hipMemcpyHostToDevice, c.st) == hipSuccess;
}
static size_t counts_pad(uint32_t nm) { return ((size_t)nm * 4 + 63) & ~(size_t)63; }   // the counts in front of the records: where the records start
static size_t count_words(uint32_t nm) { return (((size_t)nm + 15) & ~(size_t)15) + 16; }   // spill and through: the counts, then SPILL_BATCH change counts
static_assert(SPILL_BATCH <= 16, "the change counts' room");

// rocPRIM's exclusive scan of one mark per plane word, and the temporary storage it asks for (folded into `most`)
static auto lake_marks(const uint32_t* A) { return rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint32_t>(0u), LakeMarkFn{A}); }
static auto stream_marks(const uint32_t* D) { return rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint32_t>(0u), StreamMarkFn{D}); }
template <class In> static bool scan_words(const AnalysisScratch& k, In in, uint32_t* out, uint64_t words, hipStream_t st) {
  size_t bytes = k.temp_bytes;
  return rocprim::exclusive_scan(k.temp, bytes, in, out, 0u, (size_t)words, rocprim::plus<uint32_t>(), st) == hipSuccess;
}
template <class In> static bool scan_bytes(const AnalysisCall& c, In in, uint64_t words, size_t& most) {
  size_t tb = 0;
  if (rocprim::exclusive_scan(nullptr, tb, in, (uint32_t*)nullptr, 0u, (size_t)words, rocprim::plus<uint32_t>(), c.st) != hipSuccess) {
    c.err = std::string(c.who) + ": sizing the prefix sum failed";
    return false;
  }
  most = std::max(most, std::max<size_t>(tb, 8));   // (a null temporary storage would make the scan a size query again)
  return true;
}

// Room for the call in its scratch. What has to grow is dropped and replaced group by group (soil_scratch.h) behind a synchronisation:
// nothing queued still uses what is dropped. On failure nothing half-sized stays behind, and the failure does not surface in the
// next launch check.
static int analysis_reserve(const AnalysisCall& c, AnalysisScratch& k, const AnalysisScratch::Need& need, const char* what, uint64_t nrec) {
  if (k.fits(need)) return 0;
  if (hipStreamSynchronize(c.st) == hipSuccess && k.reserve(c.mem, need) == hipSuccess) return 0;
  (void)hipGetLastError();
  k.drop(c.mem);
  c.err = std::string(c.who) + ": out of memory for the " + what + " scratch (" + std::to_string(need.words) + " cells, " + std::to_string(nrec) + " records)";
  return -1;
}
// a plane, or the results, back to the host where `dst` is given, behind what is queued
static bool copy_back(const AnalysisCall& c, bool ok, void* dst, const void* src, size_t bytes) {
  return ok && (!dst || hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c.st) == hipSuccess);
}
// the end of a stretch of queued work: the stream synchronised, a failure of `what` said
static int analysis_wait(const AnalysisCall& c, bool ok, const char* what) {
  const hipError_t se = hipStreamSynchronize(c.st);
  if (ok && se == hipSuccess) return 0;
  c.err = std::string(c.who) + ": " + what + " failed on the device (" + hipGetErrorString(se != hipSuccess ? se : hipGetLastError()) + ")";
  return -1;
}

// The census's labelling: A takes the root of every wet cell's lake (acc: the census's records, null for everybody else).
static void launch_lake_labels(const AnalysisPlan& pl, hipStream_t st, const LakeMember* tab, uint32_t* A, LakeAcc* acc) {
  hipLaunchKernelGGL(k_lake_tiles, pl.gt, pl.wg, 0, st, tab, A, acc);
  hipLaunchKernelGGL(k_lake_merge, pl.gt, pl.wg, 0, st, tab, A);
  hipLaunchKernelGGL(k_lake_flatten, pl.gf, pl.wg, 0, st, tab, A);
}
// The drainage chain on the planes T and R: the wet cells labelled through `bare` -- the members with cap 0, for k_lake_tiles writes
// the identities of ITS records for ranks below cap: none here --, then k_drain_recv and k_drain_resolve through `tab`, the members
// as the drainage kernels see them (acc: the basins' records or null). d_n given, with statistics: the scan of the terminal marks
// into B and k_drain_stats, T becomes the rank plane and the counts go to d_n. P given, with area: k_drain_pending and k_drain_area
// on P and AR.
static bool launch_drain_chain(const AnalysisPlan& pl, hipStream_t st, const AnalysisScratch& k, const LakeMember* bare, const LakeMember* tab, uint32_t* T, uint32_t* B,
                               uint32_t* R, BasinAcc* acc, uint32_t* d_n, uint32_t* P, uint32_t* AR) {
  bool ok = true;
  launch_lake_labels(pl, st, bare, T, nullptr);
  hipLaunchKernelGGL(k_drain_recv, pl.gt, pl.wg, 0, st, tab, T, R, acc);
  hipLaunchKernelGGL(k_drain_resolve, pl.gf, pl.wg, 0, st, tab, T);
  if (d_n) {
    ok = scan_words(k, lake_marks(T), B, pl.words, st);
    hipLaunchKernelGGL(k_drain_stats, pl.gs, pl.wg, 0, st, tab, T, B, acc, d_n);
  }
  if (P) {
    hipLaunchKernelGGL(k_drain_pending, pl.gf, pl.wg, 0, st, tab, R, P, AR);
    hipLaunchKernelGGL(k_drain_area, pl.gf, pl.wg, 0, st, tab, R, P, AR);
  }
  return ok;
}

// The sweeps whose number depends on the map: this is where a call looks at the device more than once. launch(n, chg) queues sweep
// number n (counted from 1), which counts what it changed into *chg. SPILL_BATCH sweeps go between two looks at the change counts
// (one synchronisation each), until the batch with a sweep that changed nothing. Each sweep but the last settles a basin at least,
// so giving up after most + 2 cannot happen. (`settling`: what the sweeps settle, for that message)
template <class Launch> static int sweep_until_settled(const AnalysisCall& c, AnalysisScratch& k, const AnalysisPlan& pl, uint32_t& sweeps, const char* what,
                                                       const char* settling, Launch launch) {
  uint32_t* const d_chg = k.d_cnt + (count_words(c.nm) - 16);
  uint32_t* const h_chg = k.h_cnt + (count_words(c.nm) - 16);
  for (bool done = false; !done;) {
    if ((uint64_t)sweeps >= (uint64_t)pl.most + 2u) {
      (void)hipStreamSynchronize(c.st);
      c.err = std::string(c.who) + ": the " + settling + " did not settle within " + std::to_string(sweeps) + " sweeps (" + std::to_string(pl.most) + " basins)";
      return -1;
    }
    bool ok = hipMemsetAsync(d_chg, 0, 16 * 4, c.st) == hipSuccess;
    for (uint32_t j = 0; ok && j < SPILL_BATCH; j++) launch(sweeps + j + 1u, d_chg + j);
    ok = ok && hipGetLastError() == hipSuccess;
    ok = copy_back(c, ok, h_chg, d_chg, 16 * 4);
    if (analysis_wait(c, ok, what)) return -1;
    sweeps += SPILL_BATCH; k.batches++;
    for (uint32_t j = 0; j < SPILL_BATCH; j++) done = done || h_chg[j] == 0u;
  }
  return 0;
}

// The counts and the records into the caller's arrays: map i's records at out[i * cap ...], each cut to the caller's struct_size (a
// header older than the library has the shorter record). finish(j, rec) hands out record j of the call's table, made in rec where it
// has to be made (the streams' records are finished on the device: no second copy of what may be millions of them).
template <class Rec, class Finish> static void cut_records(const AnalysisPlan& pl, const uint32_t* n, void* out, uint64_t struct_size, uint32_t cap, uint32_t* counts,
                                                           Finish finish) {
  const size_t take = struct_size < sizeof(Rec) ? (size_t)struct_size : sizeof(Rec);
  for (size_t i = 0; i < pl.tab.size(); i++) {
    counts[i] = n[i];
    const uint32_t w = std::min(n[i], std::min(pl.tab[i].cap, cap));   // (a map holds at most tab[i].cap records where cap was cut)
    for (uint32_t r = 0; r < w; r++) {
      Rec rec;
      const Rec& done = finish((size_t)pl.tab[i].rec0 + r, rec);
      memcpy(static_cast<char*>(out) + (i * cap + r) * (size_t)struct_size, &done, take);
    }
  }
}

// ---- the lake census: planes A (labels) and B (ranks); the labelling, the scan of the root marks, k_lake_stats; the counts and the
// records (and the label plane, where asked for) copied back, one synchronisation
static_assert(sizeof(smx_lake) == 64 && sizeof(LakeRec) == sizeof(smx_lake) && offsetof(smx_lake, flags) == offsetof(LakeRec, flags), "smx_lake layout");
static int lakes_run(const AnalysisCall& c, AnalysisScratch& k, smx_lake* out, uint64_t struct_size, uint32_t cap, uint32_t* nlakes, uint32_t* labels) {
  AnalysisPlan pl;
  if (int rc = plan_members(c, cap, CAP_BLOCKS, pl)) return rc;
  AnalysisScratch::Need need;
  const size_t rec_at = counts_pad(c.nm);
  need.words = (size_t)pl.words; need.planes = 2; need.members = c.nm; need.res_bytes = rec_at + (size_t)pl.nrec * sizeof(LakeAcc);
  if (!scan_bytes(c, lake_marks(nullptr), pl.words, need.temp_bytes)) return -1;
  if (int rc = analysis_reserve(c, k, need, "census", pl.nrec)) return rc;
  uint32_t* const A = k.plane[0]; uint32_t* const B = k.plane[1];
  uint32_t* d_n = reinterpret_cast<uint32_t*>(k.d_res);
  LakeAcc* acc = reinterpret_cast<LakeAcc*>(k.d_res + rec_at);
  put_table(k, pl, 0, false);
  bool ok = send_tables(c, k, 0, 1);
  if (ok) {
    launch_lake_labels(pl, c.st, k.d_tab, A, acc);
    ok = scan_words(k, lake_marks(A), B, pl.words, c.st);
    hipLaunchKernelGGL(k_lake_stats, pl.gs, pl.wg, 0, c.st, k.d_tab, A, B, acc, d_n);
  }
  ok = ok && hipGetLastError() == hipSuccess;
  ok = copy_back(c, ok, k.h_res, k.d_res, need.res_bytes);
  ok = copy_back(c, ok, labels, A, (size_t)pl.words * 4);   // (smx_lakes only: one map, off = 0)
  if (analysis_wait(c, ok, "the census")) return -1;
  const LakeAcc* a = reinterpret_cast<const LakeAcc*>(k.h_res + rec_at);
  cut_records<LakeRec>(pl, reinterpret_cast<const uint32_t*>(k.h_res), out, struct_size, cap, nlakes, [a](size_t j, LakeRec& rec) -> const LakeRec& { lake_finish(a[j], rec); return rec; });
  return 0;
}

// ---- drainage: planes T, B, R, and P and AR once an area is asked for; the chain with its statistics, and with the area where asked
// for; the counts, the records and the planes asked for copied back, one synchronisation
static_assert(sizeof(smx_basin) == 48 && sizeof(BasinRec) == sizeof(smx_basin) && offsetof(smx_basin, height_min) == offsetof(BasinRec, height_min) &&
              offsetof(smx_basin, x0) == offsetof(BasinRec, x0), "smx_basin layout");
static int drain_run(const AnalysisCall& c, AnalysisScratch& k, smx_basin* out, uint64_t struct_size, uint32_t cap, uint32_t* nbasins, uint32_t* receivers,
                     uint32_t* labels, uint32_t* area) {
  AnalysisPlan pl;
  if (int rc = plan_members(c, cap, CAP_CELLS, pl)) return rc;
  AnalysisScratch::Need need;
  const size_t rec_at = counts_pad(c.nm);
  need.words = (size_t)pl.words; need.planes = 3; need.more = area ? 2 : 0; need.members = c.nm; need.res_bytes = rec_at + (size_t)pl.nrec * sizeof(BasinAcc);
  if (!scan_bytes(c, lake_marks(nullptr), pl.words, need.temp_bytes)) return -1;
  if (int rc = analysis_reserve(c, k, need, "drainage", pl.nrec)) return rc;
  uint32_t* const T = k.plane[0]; uint32_t* const B = k.plane[1]; uint32_t* const R = k.plane[2]; uint32_t* const P = k.plane[3]; uint32_t* const AR = k.plane[4];
  uint32_t* d_n = reinterpret_cast<uint32_t*>(k.d_res);
  BasinAcc* acc = reinterpret_cast<BasinAcc*>(k.d_res + rec_at);
  put_table(k, pl, 0, false); put_table(k, pl, 1, true);
  bool ok = send_tables(c, k, 0, 2);
  if (ok) ok = launch_drain_chain(pl, c.st, k, k.d_tab + c.nm, k.d_tab, T, B, R, acc, d_n, area ? P : nullptr, AR);
  ok = ok && hipGetLastError() == hipSuccess;
  ok = copy_back(c, ok, k.h_res, k.d_res, need.res_bytes);
  // (smx_drainage only: one map, off = 0, so a plane index is a cell index)
  ok = copy_back(c, ok, receivers, R, (size_t)pl.words * 4);
  ok = copy_back(c, ok, labels, T, (size_t)pl.words * 4);
  ok = copy_back(c, ok, area, AR, (size_t)pl.words * 4);
  if (analysis_wait(c, ok, "drainage")) return -1;
  const BasinAcc* a = reinterpret_cast<const BasinAcc*>(k.h_res + rec_at);
  cut_records<BasinRec>(pl, reinterpret_cast<const uint32_t*>(k.h_res), out, struct_size, cap, nbasins, [a](size_t j, BasinRec& rec) -> const BasinRec& { drain_finish(a[j], rec); return rec; });
  return 0;
}

// ---- the stream network: the ten planes of StreamPlanes; the chain without statistics (the basins' ranks are not needed, T stays the
// terminal plane) and with the area, all of it through the bare table; k_stream_mark, k_stream_order, the scan of the start marks,
// k_stream_segments through the table with the record caps; the counts, the records and the planes asked for copied back, one
// synchronisation
static_assert(sizeof(smx_segment) == 64 && sizeof(StreamRec) == sizeof(smx_segment) && offsetof(smx_segment, down) == offsetof(StreamRec, down) &&
              offsetof(smx_segment, straight) == offsetof(StreamRec, straight) && offsetof(smx_segment, height_first) == offsetof(StreamRec, height_first), "smx_segment layout");
static int streams_run(const AnalysisCall& c, AnalysisScratch& k, uint32_t threshold, smx_segment* out, uint64_t struct_size, uint32_t cap, uint32_t* nstreams,
                       uint32_t* order, uint32_t* segments, uint32_t* reach, uint32_t* heads) {
  AnalysisPlan pl;
  if (int rc = plan_members(c, cap, CAP_CELLS, pl)) return rc;
  AnalysisScratch::Need need;
  const size_t rec_at = counts_pad(c.nm);
  need.words = (size_t)pl.words; need.planes = 10; need.members = c.nm; need.res_bytes = rec_at + (size_t)pl.nrec * sizeof(StreamRec);
  if (!scan_bytes(c, stream_marks(nullptr), pl.words, need.temp_bytes)) return -1;
  if (int rc = analysis_reserve(c, k, need, "stream", pl.nrec)) return rc;
  const StreamPlanes p{k.plane[0], k.plane[1], k.plane[2], k.plane[3], k.plane[4], k.plane[5], k.plane[6], k.plane[7], k.plane[8], k.plane[9]};
  uint32_t* d_n = reinterpret_cast<uint32_t*>(k.d_res);
  StreamRec* recs = reinterpret_cast<StreamRec*>(k.d_res + rec_at);
  const LakeMember* bare = k.d_tab + c.nm;
  put_table(k, pl, 0, false); put_table(k, pl, 1, true);
  bool ok = send_tables(c, k, 0, 2);
  if (ok) {
    launch_drain_chain(pl, c.st, k, bare, bare, p.T, nullptr, p.R, nullptr, nullptr, p.P, p.AR);
    hipLaunchKernelGGL(k_stream_mark, pl.gf, pl.wg, 0, c.st, bare, threshold, p);
    hipLaunchKernelGGL(k_stream_order, pl.gf, pl.wg, 0, c.st, bare, threshold, p);
    ok = scan_words(k, stream_marks(p.D), p.B, pl.words, c.st);
    hipLaunchKernelGGL(k_stream_segments, pl.gf, pl.wg, 0, c.st, k.d_tab, segments ? 1 : 0, p, recs, d_n);
  }
  ok = ok && hipGetLastError() == hipSuccess;
  ok = copy_back(c, ok, k.h_res, k.d_res, need.res_bytes);
  // (smx_streams only: one map, off = 0, so a plane index is a cell index)
  ok = copy_back(c, ok, order, p.O, (size_t)pl.words * 4);
  ok = copy_back(c, ok, segments, p.SG, (size_t)pl.words * 4);
  ok = copy_back(c, ok, reach, p.RE, (size_t)pl.words * 4);
  ok = copy_back(c, ok, heads, p.H, (size_t)pl.words * 4);
  if (analysis_wait(c, ok, "the stream network")) return -1;
  const StreamRec* a = reinterpret_cast<const StreamRec*>(k.h_res + rec_at);   // (finished on the device: handed out as they are)
  cut_records<StreamRec>(pl, reinterpret_cast<const uint32_t*>(k.h_res), out, struct_size, cap, nstreams, [a](size_t j, StreamRec&) -> const StreamRec& { return a[j]; });
  return 0;
}

// ---- spill: planes T, B, R, the list plane Q and the f64 plane H. The chain with its statistics and no records (T becomes the rank
// plane), the counts back: the FIRST synchronisation -- the basins' table, the result region, is sized by them. Then k_spill_init,
// k_spill_pass<0>, k_spill_pass<1>, the scan of the boundary marks, k_spill_list, k_spill_point; k_spill_relax in the sweep loop;
// k_spill_store; the table and the plane back, the last synchronisation.
static_assert(sizeof(smx_spill_record) == 64 && sizeof(SpillRec) == sizeof(smx_spill_record) && offsetof(smx_spill_record, pour_height) == offsetof(SpillRec, pour_height) &&
              offsetof(smx_spill_record, storage_q40) == offsetof(SpillRec, storage_q40) && offsetof(smx_spill_record, flags) == offsetof(SpillRec, flags), "smx_spill_record layout");
static int spill_run(const AnalysisCall& c, AnalysisScratch& k, smx_spill_record* out, uint64_t struct_size, uint32_t cap, uint32_t* nbasins, double* filled) {
  k.sweeps[0] = 0; k.batches = 0;
  AnalysisPlan pl;
  if (int rc = plan_members(c, cap, CAP_LATER, pl)) return rc;
  AnalysisScratch::Need need;
  need.words = (size_t)pl.words; need.planes = 4; need.f64 = true; need.members = c.nm; need.count_words = count_words(c.nm);
  if (!scan_bytes(c, lake_marks(nullptr), pl.words, need.temp_bytes) || !scan_bytes(c, (const uint32_t*)nullptr, pl.words, need.temp_bytes)) return -1;
  if (int rc = analysis_reserve(c, k, need, "spill", 0)) return rc;
  const SpillPlanes p{k.plane[0], k.plane[1], k.plane[2], k.plane[3], k.h64};
  // the bare table (no records) for the drainage chain; behind it, once the counts are known, the table with the basins
  put_table(k, pl, 0, false);
  bool ok = send_tables(c, k, 0, 1);
  if (ok) ok = launch_drain_chain(pl, c.st, k, k.d_tab, k.d_tab, p.T, p.B, p.R, nullptr, k.d_cnt, nullptr, nullptr);
  ok = ok && hipGetLastError() == hipSuccess;
  ok = copy_back(c, ok, k.h_cnt, k.d_cnt, (size_t)c.nm * 4);
  if (analysis_wait(c, ok, "the drainage chain")) return -1;
  plan_basins(c, pl, k.h_cnt);
  need.res_bytes = (size_t)pl.nrec * sizeof(SpillAcc);
  if (int rc = analysis_reserve(c, k, need, "spill", pl.nrec)) return rc;   // (the stream is idle)
  SpillAcc* acc = reinterpret_cast<SpillAcc*>(k.d_res);
  const LakeMember* full = k.d_tab + c.nm;
  put_table(k, pl, 1, false);
  ok = send_tables(c, k, 1, 1);
  if (ok) {
    hipLaunchKernelGGL(k_spill_init, pl.gb, pl.wg, 0, c.st, full, acc);
    hipLaunchKernelGGL(k_spill_pass<0>, pl.gt, pl.wg, 0, c.st, full, p, acc);
    hipLaunchKernelGGL(k_spill_pass<1>, pl.gt, pl.wg, 0, c.st, full, p, acc);
    ok = scan_words(k, (const uint32_t*)p.R, p.B, pl.words, c.st);
    hipLaunchKernelGGL(k_spill_list, pl.gf, pl.wg, 0, c.st, full, p);
    hipLaunchKernelGGL(k_spill_point, pl.gb, pl.wg, 0, c.st, full, p, acc);
  }
  if (!ok) return analysis_wait(c, false, "the spill analysis");
  if (sweep_until_settled(c, k, pl, k.sweeps[0], "the spill analysis", "fill levels",
                          [&](uint32_t n, uint32_t* chg) { hipLaunchKernelGGL(k_spill_relax, pl.gr, pl.wg, 0, c.st, full, n, p, acc, chg); }))
    return -1;
  hipLaunchKernelGGL(k_spill_store, pl.gs, pl.wg, 0, c.st, full, p, acc, filled ? 1 : 0);
  ok = hipGetLastError() == hipSuccess;
  ok = copy_back(c, ok, k.h_res, k.d_res, need.res_bytes);
  ok = copy_back(c, ok, filled, p.H, (size_t)pl.words * 8);   // (smx_spill only: one map, off = 0)
  if (analysis_wait(c, ok, "the spill analysis")) return -1;
  const SpillAcc* a = reinterpret_cast<const SpillAcc*>(k.h_res);
  cut_records<SpillRec>(pl, k.h_cnt, out, struct_size, cap, nbasins, [a](size_t j, SpillRec& rec) -> const SpillRec& { spill_finish(a[j], rec); return rec; });
  return 0;
}

// ---- through-drainage: spill's planes and one more -- T, B, R (the receivers), M (the boundary marks, later the pending words), Q (the
// boundary list, later the area), the f64 plane H. The chain with its statistics and no records, the counts back: the FIRST
// synchronisation; the result region holds the two basins' tables, spill's in front. Then k_spill_init, k_through_init,
// k_spill_pass<0>, k_spill_pass<1> (their boundary marks go to M: R stays the receivers), the scan, k_spill_list, k_spill_point,
// k_through_count; k_spill_relax in the sweep loop, k_through_hops likewise; k_through_exit; k_drain_pending where the area is asked
// for (P takes M's plane and AR takes Q's: the marks and the list are done with); k_through_link<0>, <1>, k_through_accumulate,
// k_through_outlet, k_through_plane and k_through_area where their planes are asked for; the tables and the planes back, the last
// synchronisation.
static_assert(sizeof(smx_through_record) == 64 && sizeof(ThroughRec) == sizeof(smx_through_record) && offsetof(smx_through_record, exit_height) == offsetof(ThroughRec, exit_height) &&
              offsetof(smx_through_record, hops) == offsetof(ThroughRec, hops) && offsetof(smx_through_record, through_cells) == offsetof(ThroughRec, through_cells), "smx_through_record layout");
static_assert(sizeof(SpillAcc) % alignof(ThroughAcc) == 0, "the second table of the result region is aligned");
static int through_run(const AnalysisCall& c, AnalysisScratch& k, smx_through_record* out, uint64_t struct_size, uint32_t cap, uint32_t* nbasins, uint32_t* through_area,
                       uint32_t* outlets) {
  k.sweeps[0] = k.sweeps[1] = 0; k.batches = 0;
  AnalysisPlan pl;
  if (int rc = plan_members(c, cap, CAP_LATER, pl)) return rc;
  AnalysisScratch::Need need;
  need.words = (size_t)pl.words; need.planes = 5; need.f64 = true; need.members = c.nm; need.count_words = count_words(c.nm);
  if (!scan_bytes(c, lake_marks(nullptr), pl.words, need.temp_bytes) || !scan_bytes(c, (const uint32_t*)nullptr, pl.words, need.temp_bytes)) return -1;
  if (int rc = analysis_reserve(c, k, need, "through-drainage", 0)) return rc;
  uint32_t* const T = k.plane[0]; uint32_t* const B = k.plane[1]; uint32_t* const R = k.plane[2]; uint32_t* const M = k.plane[3]; uint32_t* const Q = k.plane[4];
  const SpillPlanes sp{T, B, M, Q, k.h64};     // what the spill chain's kernels see: their R is M
  const ThroughPlanes p{T, B, M, Q, k.h64};
  uint32_t* const P = M;                       // behind k_through_exit
  uint32_t* const AR = through_area ? Q : nullptr;
  put_table(k, pl, 0, false);
  bool ok = send_tables(c, k, 0, 1);
  if (ok) ok = launch_drain_chain(pl, c.st, k, k.d_tab, k.d_tab, T, B, R, nullptr, k.d_cnt, nullptr, nullptr);
  ok = ok && hipGetLastError() == hipSuccess;
  ok = copy_back(c, ok, k.h_cnt, k.d_cnt, (size_t)c.nm * 4);
  if (analysis_wait(c, ok, "the drainage chain")) return -1;
  plan_basins(c, pl, k.h_cnt);
  need.res_bytes = (size_t)pl.nrec * (sizeof(SpillAcc) + sizeof(ThroughAcc));
  if (int rc = analysis_reserve(c, k, need, "through-drainage", pl.nrec)) return rc;   // (the stream is idle)
  const size_t acc_at = (size_t)pl.nrec * sizeof(SpillAcc);
  SpillAcc* sacc = reinterpret_cast<SpillAcc*>(k.d_res);
  ThroughAcc* acc = reinterpret_cast<ThroughAcc*>(k.d_res + acc_at);
  const LakeMember* full = k.d_tab + c.nm;
  put_table(k, pl, 1, false);
  ok = send_tables(c, k, 1, 1);
  if (ok) {
    hipLaunchKernelGGL(k_spill_init, pl.gb, pl.wg, 0, c.st, full, sacc);
    hipLaunchKernelGGL(k_through_init, pl.gb, pl.wg, 0, c.st, full, acc);
    hipLaunchKernelGGL(k_spill_pass<0>, pl.gt, pl.wg, 0, c.st, full, sp, sacc);
    hipLaunchKernelGGL(k_spill_pass<1>, pl.gt, pl.wg, 0, c.st, full, sp, sacc);
    ok = scan_words(k, (const uint32_t*)M, B, pl.words, c.st);
    hipLaunchKernelGGL(k_spill_list, pl.gf, pl.wg, 0, c.st, full, sp);
    hipLaunchKernelGGL(k_spill_point, pl.gb, pl.wg, 0, c.st, full, sp, sacc);
    hipLaunchKernelGGL(k_through_count, pl.gs, pl.wg, 0, c.st, full, T, acc);
  }
  if (!ok) return analysis_wait(c, false, "the through-drainage");
  // the fill levels first and the hop counts behind them
  if (sweep_until_settled(c, k, pl, k.sweeps[0], "the through-drainage", "fill levels",
                          [&](uint32_t n, uint32_t* chg) { hipLaunchKernelGGL(k_spill_relax, pl.gr, pl.wg, 0, c.st, full, n, sp, sacc, chg); }))
    return -1;
  if (sweep_until_settled(c, k, pl, k.sweeps[1], "the through-drainage", "hop counts",
                          [&](uint32_t, uint32_t* chg) { hipLaunchKernelGGL(k_through_hops, pl.gr, pl.wg, 0, c.st, full, p, sacc, acc, chg); }))
    return -1;
  hipLaunchKernelGGL(k_through_exit, pl.gr, pl.wg, 0, c.st, full, p, sacc, acc);
  if (AR) hipLaunchKernelGGL(k_drain_pending, pl.gf, pl.wg, 0, c.st, full, R, P, AR);
  hipLaunchKernelGGL(k_through_link<0>, pl.gb, pl.wg, 0, c.st, full, p, sacc, acc);
  hipLaunchKernelGGL(k_through_link<1>, pl.gb, pl.wg, 0, c.st, full, p, sacc, acc);
  hipLaunchKernelGGL(k_through_accumulate, pl.gb, pl.wg, 0, c.st, full, acc, AR);
  hipLaunchKernelGGL(k_through_outlet, pl.gb, pl.wg, 0, c.st, full, sacc, acc);
  if (outlets) hipLaunchKernelGGL(k_through_plane, pl.gf, pl.wg, 0, c.st, full, T, acc, B);   // (B is done with)
  if (AR) hipLaunchKernelGGL(k_through_area, pl.gf, pl.wg, 0, c.st, full, R, P, AR);
  ok = hipGetLastError() == hipSuccess;
  ok = copy_back(c, ok, k.h_res, k.d_res, need.res_bytes);
  // (smx_through only: one map, off = 0)
  ok = copy_back(c, ok, through_area, AR, (size_t)pl.words * 4);
  ok = copy_back(c, ok, outlets, B, (size_t)pl.words * 4);
  if (analysis_wait(c, ok, "the through-drainage")) return -1;
  const SpillAcc* sa = reinterpret_cast<const SpillAcc*>(k.h_res);
  const ThroughAcc* a = reinterpret_cast<const ThroughAcc*>(k.h_res + acc_at);
  cut_records<ThroughRec>(pl, k.h_cnt, out, struct_size, cap, nbasins, [sa, a](size_t j, ThroughRec& rec) -> const ThroughRec& { through_finish(sa[j], a[j], rec); return rec; });
  return 0;
}

// ---- the hillslopes: the ten planes of StreamPlanes and the f64 plane. The streams chain through the bare table, k_stream_segments
// with its plane and no record: SG is complete. Then k_hill_init through the table with the record caps (J takes R's plane, S and G
// take P's and AR's), k rounds of k_hill_jump between that set and (T, O, H) -- k is known before the launch from the path bound
// min(threshold, the largest map's cells) - 1 --, k_hill_fold on the set the last round wrote; entry goes to RE's plane, hillslope to
// the other set's J, hand to the f64 plane, the steps are the settled set itself. The counts, the records and the planes asked for
// copied back, one synchronisation.
static_assert(sizeof(smx_hillslope) == 64 && sizeof(HillRec) == sizeof(smx_hillslope) && offsetof(smx_hillslope, straight_sum) == offsetof(HillRec, straight_sum) &&
              offsetof(smx_hillslope, hand_max) == offsetof(HillRec, hand_max) && offsetof(smx_hillslope, bank_cells) == offsetof(HillRec, bank_cells) &&
              offsetof(smx_hillslope, farthest_cell) == offsetof(HillRec, farthest_cell), "smx_hillslope layout");
static int hills_run(const AnalysisCall& c, AnalysisScratch& k, uint32_t threshold, smx_hillslope* out, uint64_t struct_size, uint32_t cap, uint32_t* nsegments,
                     uint32_t* entry, uint32_t* hillslope, uint32_t* straight, uint32_t* diagonal, double* hand) {
  AnalysisPlan pl;
  if (int rc = plan_members(c, cap, CAP_CELLS, pl)) return rc;
  AnalysisScratch::Need need;
  const size_t rec_at = counts_pad(c.nm);
  need.words = (size_t)pl.words; need.planes = 10; need.f64 = true; need.members = c.nm; need.res_bytes = rec_at + (size_t)pl.nrec * sizeof(HillAcc);
  if (!scan_bytes(c, stream_marks(nullptr), pl.words, need.temp_bytes)) return -1;
  if (int rc = analysis_reserve(c, k, need, "hillslope", pl.nrec)) return rc;
  const StreamPlanes p{k.plane[0], k.plane[1], k.plane[2], k.plane[3], k.plane[4], k.plane[5], k.plane[6], k.plane[7], k.plane[8], k.plane[9]};
  const HillSet set[2] = {{p.R, p.P, p.AR}, {p.T, p.O, p.H}};
  uint64_t largest = 0;
  for (uint32_t i = 0; i < c.nm; i++) largest = std::max<uint64_t>(largest, c.ms[i]->ncells);
  const uint32_t rounds = hill_rounds(hill_bound(threshold, largest));
  const HillSet& last = set[rounds & 1u];
  uint32_t* const d_entry = p.RE; uint32_t* const d_hill = set[(rounds + 1u) & 1u].J;
  uint32_t* d_n = reinterpret_cast<uint32_t*>(k.d_res);
  HillAcc* acc = reinterpret_cast<HillAcc*>(k.d_res + rec_at);
  const LakeMember* bare = k.d_tab + c.nm;
  put_table(k, pl, 0, false); put_table(k, pl, 1, true);
  bool ok = send_tables(c, k, 0, 2);
  if (ok) {
    launch_drain_chain(pl, c.st, k, bare, bare, p.T, nullptr, p.R, nullptr, nullptr, p.P, p.AR);
    hipLaunchKernelGGL(k_stream_mark, pl.gf, pl.wg, 0, c.st, bare, threshold, p);
    hipLaunchKernelGGL(k_stream_order, pl.gf, pl.wg, 0, c.st, bare, threshold, p);
    ok = scan_words(k, stream_marks(p.D), p.B, pl.words, c.st);
    hipLaunchKernelGGL(k_stream_segments, pl.gf, pl.wg, 0, c.st, bare, 1, p, (StreamRec*)nullptr, d_n);   // (cap 0: no record is written)
    hipLaunchKernelGGL(k_hill_init, pl.gf, pl.wg, 0, c.st, k.d_tab, p.SG, set[0], acc);
    for (uint32_t r = 0; r < rounds; r++) hipLaunchKernelGGL(k_hill_jump, pl.gf, pl.wg, 0, c.st, bare, set[r & 1u], set[(r + 1u) & 1u]);
    hipLaunchKernelGGL(k_hill_fold, pl.gs, pl.wg, 0, c.st, k.d_tab, last, p.SG, p.D, p.B, acc, d_n, entry ? d_entry : nullptr, hillslope ? d_hill : nullptr,
                       hand ? k.h64 : nullptr);
  }
  ok = ok && hipGetLastError() == hipSuccess;
  ok = copy_back(c, ok, k.h_res, k.d_res, need.res_bytes);
  // (smx_hillslopes only: one map, off = 0, so a plane index is a cell index)
  ok = copy_back(c, ok, entry, d_entry, (size_t)pl.words * 4);
  ok = copy_back(c, ok, hillslope, d_hill, (size_t)pl.words * 4);
  ok = copy_back(c, ok, straight, last.S, (size_t)pl.words * 4);
  ok = copy_back(c, ok, diagonal, last.G, (size_t)pl.words * 4);
  ok = copy_back(c, ok, hand, k.h64, (size_t)pl.words * 8);
  if (analysis_wait(c, ok, "the hillslopes")) return -1;
  const HillAcc* a = reinterpret_cast<const HillAcc*>(k.h_res + rec_at);
  cut_records<HillRec>(pl, reinterpret_cast<const uint32_t*>(k.h_res), out, struct_size, cap, nsegments, [a](size_t j, HillRec& rec) -> const HillRec& { hill_finish(a[j], rec); return rec; });
  return 0;
}

// ---- the flow paths: ten planes and the f64 plane, which holds the 64-bit words UP. The drainage chain with its statistics through
// the bare table (T becomes the rank plane, the counts go to d_n, no basin record is written), k_drain_pending (its AR plane is the
// first set's J, overwritten next), k_path_init through the table with the record caps (B's plane becomes FH), k rounds of
// k_hill_jump between the sets (4, 5, 6) and (7, 8, 9) -- k is known before the launch from the cells of the largest map --, then on
// the set the last round wrote: k_path_fold, k_path_up, k_path_lengths, the scan of the lengths, k_path_stem. The other set is dead
// by then: its planes are FS, L and PA. stem goes over T, the terminal over J, the drop over UP, upstream and source to the planes
// of R and P, dead behind k_path_up; the steps are the settled set itself; the profile is scattered into the result region behind
// the records. The counts (the basins, then the profiles' lengths), the records, the profile and the planes asked for copied back,
// one synchronisation.
static_assert(sizeof(smx_flowpath) == 64 && sizeof(PathRec) == sizeof(smx_flowpath) && offsetof(smx_flowpath, source_cell) == offsetof(PathRec, source_cell) &&
              offsetof(smx_flowpath, profile_at) == offsetof(PathRec, profile_at) && offsetof(smx_flowpath, straight_sum) == offsetof(PathRec, straight_sum) &&
              offsetof(smx_flowpath, drop_source) == offsetof(PathRec, drop_source) && offsetof(smx_flowpath, drop_max) == offsetof(PathRec, drop_max),
              "smx_flowpath layout");
static int paths_run(const AnalysisCall& c, AnalysisScratch& k, smx_flowpath* out, uint64_t struct_size, uint32_t cap, uint32_t* nbasins, uint32_t* terminal,
                     uint32_t* straight, uint32_t* diagonal, double* drop, uint32_t* upstream, uint32_t* source, uint32_t* stem, uint32_t* profile,
                     uint32_t profile_cap, uint32_t* nprofile) {
  AnalysisPlan pl;
  if (int rc = plan_members(c, cap, CAP_CELLS, pl)) return rc;
  AnalysisScratch::Need need;
  const size_t rec_at = counts_pad(2 * c.nm), prof_at = rec_at + (size_t)pl.nrec * sizeof(PathAcc);
  const uint32_t pcap = profile ? (uint32_t)std::min<uint64_t>(profile_cap, pl.words) : 0u;   // (a profile has at most a cell per cell)
  need.words = (size_t)pl.words; need.planes = 10; need.f64 = true; need.members = c.nm; need.res_bytes = prof_at + (size_t)pcap * 4;
  if (!scan_bytes(c, lake_marks(nullptr), pl.words, need.temp_bytes) || !scan_bytes(c, (const uint32_t*)nullptr, pl.words, need.temp_bytes)) return -1;
  if (int rc = analysis_reserve(c, k, need, "flow path", pl.nrec)) return rc;
  const HillSet set[2] = {{k.plane[4], k.plane[5], k.plane[6]}, {k.plane[7], k.plane[8], k.plane[9]}};
  uint64_t largest = 0;
  for (uint32_t i = 0; i < c.nm; i++) largest = std::max<uint64_t>(largest, c.ms[i]->ncells);
  const uint32_t rounds = hill_rounds(largest - 1u);   // (a path has at most cells - 1 steps)
  const HillSet& spare = set[(rounds + 1u) & 1u];
  PathPlanes p;
  p.T = k.plane[0]; p.FH = k.plane[1]; p.R = k.plane[2]; p.P = k.plane[3]; p.FS = spare.J; p.L = spare.S; p.PA = spare.G;
  p.UP = reinterpret_cast<uint64_t*>(k.h64); p.s = set[rounds & 1u];
  uint32_t* d_n = reinterpret_cast<uint32_t*>(k.d_res);
  PathAcc* acc = reinterpret_cast<PathAcc*>(k.d_res + rec_at);
  PathOut o;
  o.want_terminal = terminal ? 1u : 0u; o.want_stem = stem ? 1u : 0u; o.want_drop = drop ? 1u : 0u; o.profile_cap = pcap;
  o.upstream = upstream ? p.R : nullptr; o.source = source ? p.P : nullptr; o.profile = pcap ? reinterpret_cast<uint32_t*>(k.d_res + prof_at) : nullptr;
  const LakeMember* bare = k.d_tab + c.nm;
  put_table(k, pl, 0, false); put_table(k, pl, 1, true);
  bool ok = send_tables(c, k, 0, 2);
  if (ok) {
    ok = launch_drain_chain(pl, c.st, k, bare, bare, p.T, p.FH, p.R, nullptr, d_n, nullptr, nullptr);
    hipLaunchKernelGGL(k_drain_pending, pl.gf, pl.wg, 0, c.st, bare, p.R, p.P, set[0].J);
    hipLaunchKernelGGL(k_path_init, pl.gf, pl.wg, 0, c.st, k.d_tab, p.R, set[0], p.FH, acc);
    for (uint32_t r = 0; r < rounds; r++) hipLaunchKernelGGL(k_hill_jump, pl.gf, pl.wg, 0, c.st, bare, set[r & 1u], set[(r + 1u) & 1u]);
    hipLaunchKernelGGL(k_path_fold, pl.gs, pl.wg, 0, c.st, k.d_tab, p, acc);
    hipLaunchKernelGGL(k_path_up, pl.gf, pl.wg, 0, c.st, bare, p);
    hipLaunchKernelGGL(k_path_lengths, pl.gf, pl.wg, 0, c.st, bare, p, d_n);
    ok = ok && scan_words(k, (const uint32_t*)p.L, p.PA, pl.words, c.st);
    hipLaunchKernelGGL(k_path_stem, pl.gf, pl.wg, 0, c.st, k.d_tab, p, acc, d_n, d_n + c.nm, o);
  }
  ok = ok && hipGetLastError() == hipSuccess;
  ok = copy_back(c, ok, k.h_res, k.d_res, need.res_bytes);
  // (smx_flowpaths only: one map, off = 0, so a plane index is a cell index)
  ok = copy_back(c, ok, terminal, p.s.J, (size_t)pl.words * 4);
  ok = copy_back(c, ok, straight, p.s.S, (size_t)pl.words * 4);
  ok = copy_back(c, ok, diagonal, p.s.G, (size_t)pl.words * 4);
  ok = copy_back(c, ok, drop, k.h64, (size_t)pl.words * 8);
  ok = copy_back(c, ok, upstream, p.R, (size_t)pl.words * 4);
  ok = copy_back(c, ok, source, p.P, (size_t)pl.words * 4);
  ok = copy_back(c, ok, stem, p.T, (size_t)pl.words * 4);
  if (analysis_wait(c, ok, "the flow paths")) return -1;
  const uint32_t* n = reinterpret_cast<const uint32_t*>(k.h_res);
  if (nprofile) *nprofile = n[c.nm];
  if (pcap) memcpy(profile, k.h_res + prof_at, (size_t)std::min(pcap, n[c.nm]) * 4);
  const PathAcc* a = reinterpret_cast<const PathAcc*>(k.h_res + rec_at);
  cut_records<PathRec>(pl, n, out, struct_size, cap, nbasins, [a](size_t j, PathRec& rec) -> const PathRec& { path_finish(a[j], rec); return rec; });
  return 0;
}

// ---- the catchments: ten planes and the f64 plane. The caller's list goes into the result region with the tables' upload; the mark
// plane M (plane 3) is filled and k_catch_mark scatters the list into it for every member. The drainage chain with its statistics
// through the bare table and WITHOUT its area step (T becomes the rank plane, no basin record is written), k_catch_init through the
// table with the record caps (n a member), k rounds of k_hill_jump between the sets (4, 5, 6) and (7, 8, 9) -- k is known before the
// launch from the cells of the largest map --, k_catch_fold on the set the last round wrote and, with bins, k_catch_hist on the
// zeroed tables. The gauge plane goes to the other set's J, the drop to the f64 plane, the steps are the settled set itself. The
// region holds the chain's counts, the records, the tables and the list; all but the list copied back with the planes asked for,
// one synchronisation. The records are cut per map with area folded over the gauges' forest (catch_area).
static_assert(sizeof(smx_catchment) == 64 && sizeof(CatchRec) == sizeof(smx_catchment) && offsetof(smx_catchment, area) == offsetof(CatchRec, area) &&
              offsetof(smx_catchment, basin) == offsetof(CatchRec, basin) && offsetof(smx_catchment, farthest_cell) == offsetof(CatchRec, farthest_cell) &&
              offsetof(smx_catchment, straight_sum) == offsetof(CatchRec, straight_sum) && offsetof(smx_catchment, drop_max) == offsetof(CatchRec, drop_max) &&
              offsetof(smx_catchment, drop_sum_q40) == offsetof(CatchRec, drop_sum_q40) && (uint32_t)SMX_CATCHMENT_MAX_BINS == CATCH_MAX_BINS,
              "smx_catchment layout");
static int catch_run(const AnalysisCall& c, AnalysisScratch& k, const uint32_t* cells, uint32_t n, smx_catchment* out, uint64_t struct_size, uint32_t* hist,
                     uint32_t nbins, double bin_height, uint32_t* gauge, uint32_t* straight, uint32_t* diagonal, double* drop) {
  AnalysisPlan pl;
  if (int rc = plan_members(c, n, CAP_CELLS, pl)) return rc;   // (n distinct cells inside every member: every member keeps n records)
  AnalysisScratch::Need need;
  const size_t rec_at = counts_pad(c.nm), hist_at = rec_at + (size_t)pl.nrec * sizeof(CatchAcc);
  const size_t hist_bytes = (size_t)pl.nrec * nbins * 4, list_at = hist_at + ((hist_bytes + 63) & ~(size_t)63);
  need.words = (size_t)pl.words; need.planes = 10; need.f64 = true; need.members = c.nm; need.res_bytes = list_at + (size_t)n * 4;
  if (!scan_bytes(c, lake_marks(nullptr), pl.words, need.temp_bytes)) return -1;
  if (int rc = analysis_reserve(c, k, need, "catchment", pl.nrec)) return rc;
  const HillSet set[2] = {{k.plane[4], k.plane[5], k.plane[6]}, {k.plane[7], k.plane[8], k.plane[9]}};
  uint64_t largest = 0;
  for (uint32_t i = 0; i < c.nm; i++) largest = std::max<uint64_t>(largest, c.ms[i]->ncells);
  const uint32_t rounds = hill_rounds(largest - 1u);   // (a path has at most cells - 1 steps)
  uint32_t* const B = k.plane[1];
  const CatchPlanes first{k.plane[0], k.plane[2], k.plane[3], set[0]}, last{k.plane[0], k.plane[2], k.plane[3], set[rounds & 1u]};
  uint32_t* const d_gauge = set[(rounds + 1u) & 1u].J;
  uint32_t* d_n = reinterpret_cast<uint32_t*>(k.d_res);
  CatchAcc* acc = reinterpret_cast<CatchAcc*>(k.d_res + rec_at);
  uint32_t* d_hist = reinterpret_cast<uint32_t*>(k.d_res + hist_at);
  uint32_t* d_list = reinterpret_cast<uint32_t*>(k.d_res + list_at);
  const LakeMember* bare = k.d_tab + c.nm;
  memcpy(k.h_res + list_at, cells, (size_t)n * 4);
  put_table(k, pl, 0, false); put_table(k, pl, 1, true);
  bool ok = send_tables(c, k, 0, 2);
  ok = ok && hipMemcpyAsync(d_list, k.h_res + list_at, (size_t)n * 4, hipMemcpyHostToDevice, c.st) == hipSuccess;
  ok = ok && hipMemsetAsync(first.M, 0xFF, (size_t)pl.words * 4, c.st) == hipSuccess;
  ok = ok && (!nbins || hipMemsetAsync(d_hist, 0, hist_bytes, c.st) == hipSuccess);
  if (ok) {
    hipLaunchKernelGGL(k_catch_mark, dim3((unsigned)(((size_t)n + LAKE_LANES - 1) / LAKE_LANES), c.nm), pl.wg, 0, c.st, bare, d_list, n, first.M);
    ok = launch_drain_chain(pl, c.st, k, bare, bare, first.T, B, first.R, nullptr, d_n, nullptr, nullptr);
    hipLaunchKernelGGL(k_catch_init, pl.gf, pl.wg, 0, c.st, k.d_tab, first, acc);
    for (uint32_t r = 0; r < rounds; r++) hipLaunchKernelGGL(k_hill_jump, pl.gf, pl.wg, 0, c.st, bare, set[r & 1u], set[(r + 1u) & 1u]);
    hipLaunchKernelGGL(k_catch_fold, pl.gs, pl.wg, 0, c.st, k.d_tab, last, acc, gauge ? d_gauge : nullptr, drop ? k.h64 : nullptr);
    if (nbins) hipLaunchKernelGGL(k_catch_hist, pl.gs, pl.wg, 0, c.st, k.d_tab, last, d_hist, nbins, bin_height);
  }
  ok = ok && hipGetLastError() == hipSuccess;
  ok = copy_back(c, ok, k.h_res, k.d_res, hist_at + hist_bytes);
  // (smx_catchments only: one map, off = 0, so a plane index is a cell index)
  ok = copy_back(c, ok, gauge, d_gauge, (size_t)pl.words * 4);
  ok = copy_back(c, ok, straight, last.s.S, (size_t)pl.words * 4);
  ok = copy_back(c, ok, diagonal, last.s.G, (size_t)pl.words * 4);
  ok = copy_back(c, ok, drop, k.h64, (size_t)pl.words * 8);
  if (analysis_wait(c, ok, "the catchments")) return -1;
  const CatchAcc* a = reinterpret_cast<const CatchAcc*>(k.h_res + rec_at);
  const size_t take = struct_size < sizeof(CatchRec) ? (size_t)struct_size : sizeof(CatchRec);
  std::vector<CatchRec> recs(n);
  std::vector<uint32_t> work(2 * (size_t)n);
  for (uint32_t i = 0; i < c.nm; i++) {
    for (uint32_t r = 0; r < n; r++) catch_finish(a[(size_t)pl.tab[i].rec0 + r], recs[r]);
    catch_area(recs.data(), n, work.data(), work.data() + n);
    for (uint32_t r = 0; r < n; r++) memcpy(reinterpret_cast<char*>(out) + ((size_t)i * n + r) * (size_t)struct_size, &recs[r], take);
  }
  if (nbins) memcpy(hist, k.h_res + hist_at, hist_bytes);
  return 0;
}

// ---- the horizons: no chain and no u32 plane of the common kind. Everything that is a double lives in the f64 plane, one stretch
// behind the other: the heights H (a double per cell), the fine and the coarse maxima of every member, the members' maxima MM (ordered
// images, zeroed), and only where asked for the sky plane and the slopes of all directions (nd doubles per cell). The u32 planes --
// the steps of all directions, open, lit -- are carved from the temporary storage, which no scan needs here; a records-only call keeps
// neither slopes nor steps. The members go into the tables twice: as everywhere with cap = nd and rec0 = i * nd, and the view of
// their tiles (soil_horizon.h). The region holds the suns (uploaded with the tables), the records and the sun counts (zeroed: the
// fold's identities); k_horizon_heights, k_horizon_scan with a z per direction, k_horizon_sky where sky, open or lit is asked for;
// the records, the counts and the planes asked for copied back, one synchronisation.
static_assert(sizeof(smx_horizon_record) == 64 && sizeof(HorizonRec) == sizeof(smx_horizon_record) && offsetof(smx_horizon_record, ux) == offsetof(HorizonRec, ux) &&
              offsetof(smx_horizon_record, bounded) == offsetof(HorizonRec, bounded) && offsetof(smx_horizon_record, step_max_cell) == offsetof(HorizonRec, step_max_cell) &&
              offsetof(smx_horizon_record, step_sum) == offsetof(HorizonRec, step_sum) && offsetof(smx_horizon_record, slope_max) == offsetof(HorizonRec, slope_max) &&
              sizeof(smx_sun) == sizeof(HorizonSun) && offsetof(smx_sun, tangent) == offsetof(HorizonSun, tangent) && (uint32_t)SMX_HORIZON_MAX_SUNS == HORIZON_MAX_SUNS &&
              (uint32_t)SMX_HORIZON_DIRECTIONS == HORIZON_DIRS,
              "smx_horizon_record / smx_sun layout");
static int horizons_run(const AnalysisCall& c, AnalysisScratch& k, uint32_t mask, uint32_t reach, smx_horizon_record* out, uint64_t struct_size, const smx_sun* suns,
                        uint32_t nsuns, uint32_t* lit_cells, double* slope, uint32_t* step, double* sky, uint32_t* open, uint32_t* lit) {
  const uint32_t nd = horizon_count(mask);
  AnalysisPlan pl;
  if (int rc = plan_members(c, nd, CAP_CELLS, pl)) return rc;
  std::vector<LakeMember> tiles(pl.tab);
  uint64_t nfine = 0, ncoarse = 0;
  unsigned most = 1;
  for (uint32_t i = 0; i < c.nm; i++) {   // (a fine tile holds a cell at least: no more tiles than cells, the offsets fit)
    pl.tab[i].cap = nd; pl.tab[i].rec0 = i * nd;
    tiles[i].off = (uint32_t)nfine; tiles[i].rec0 = (uint32_t)ncoarse; tiles[i].cap = i;
    nfine += horizon_tiles(pl.tab[i], HORIZON_FINE);
    const uint32_t nc = horizon_tiles(pl.tab[i], HORIZON_COARSE);
    ncoarse += nc; most = std::max<unsigned>(most, nc);
  }
  pl.nrec = (uint64_t)c.nm * nd;
  const bool folded = sky || open || lit, kept = slope || step || folded;
  const size_t W = (size_t)pl.words;
  const size_t fm_at = W, cm_at = fm_at + (size_t)nfine, mm_at = cm_at + (size_t)ncoarse, sky_at = mm_at + c.nm, s_at = sky_at + (sky ? W : 0);
  const size_t open_at = kept ? (size_t)nd * W : 0, lit_at = open_at + (open ? W : 0);
  const size_t rec_at = ((size_t)nsuns * sizeof(HorizonSun) + 63) & ~(size_t)63, cnt_at = rec_at + (size_t)pl.nrec * sizeof(HorizonAcc);
  AnalysisScratch::Need need;
  need.words = s_at + (kept ? (size_t)nd * W : 0); need.planes = 0; need.f64 = true; need.members = c.nm;
  need.temp_bytes = (lit_at + (lit ? W : 0)) * 4;
  need.res_bytes = cnt_at + (size_t)c.nm * nsuns * 4;
  if (int rc = analysis_reserve(c, k, need, "horizon", pl.nrec)) return rc;
  uint32_t* const U = static_cast<uint32_t*>(k.temp);
  HorizonPlanes p;
  p.H = k.h64; p.FM = k.h64 + fm_at; p.CM = k.h64 + cm_at; p.MM = reinterpret_cast<uint64_t*>(k.h64 + mm_at);
  p.S = kept ? k.h64 + s_at : nullptr; p.K = kept ? U : nullptr;
  p.acc = reinterpret_cast<HorizonAcc*>(k.d_res + rec_at); p.lit_cells = reinterpret_cast<uint32_t*>(k.d_res + cnt_at);
  p.suns = reinterpret_cast<const HorizonSun*>(k.d_res); p.nsuns = nsuns; p.words = pl.words;
  double* const d_sky = sky ? k.h64 + sky_at : nullptr;
  uint32_t* const d_open = open ? U + open_at : nullptr;
  uint32_t* const d_lit = lit ? U + lit_at : nullptr;
  if (nsuns) memcpy(k.h_res, suns, (size_t)nsuns * sizeof(HorizonSun));
  put_table(k, pl, 0, false);
  memcpy(k.h_tab + c.nm, tiles.data(), (size_t)c.nm * sizeof(LakeMember));
  bool ok = send_tables(c, k, 0, 2);
  ok = ok && (!nsuns || hipMemcpyAsync(k.d_res, k.h_res, (size_t)nsuns * sizeof(HorizonSun), hipMemcpyHostToDevice, c.st) == hipSuccess);
  ok = ok && hipMemsetAsync(k.d_res + rec_at, 0, need.res_bytes - rec_at, c.st) == hipSuccess;
  ok = ok && hipMemsetAsync(p.MM, 0, (size_t)c.nm * 8, c.st) == hipSuccess;
  if (ok) {
    hipLaunchKernelGGL(k_horizon_heights, dim3(most, c.nm), pl.wg, 0, c.st, k.d_tab, p);
    hipLaunchKernelGGL(k_horizon_scan, dim3(pl.gf.x, c.nm, nd), pl.wg, 0, c.st, k.d_tab, p, mask, reach);
    if (folded) hipLaunchKernelGGL(k_horizon_sky, pl.gf, pl.wg, 0, c.st, k.d_tab, p, mask, d_sky, d_open, d_lit);
  }
  ok = ok && hipGetLastError() == hipSuccess;
  ok = copy_back(c, ok, k.h_res + rec_at, k.d_res + rec_at, need.res_bytes - rec_at);
  // (smx_horizons only: one map, off = 0, so a plane index is a cell index)
  ok = copy_back(c, ok, slope, p.S, (size_t)nd * W * 8);
  ok = copy_back(c, ok, step, p.K, (size_t)nd * W * 4);
  ok = copy_back(c, ok, sky, d_sky, W * 8);
  ok = copy_back(c, ok, open, d_open, W * 4);
  ok = copy_back(c, ok, lit, d_lit, W * 4);
  if (analysis_wait(c, ok, "the horizons")) return -1;
  const HorizonAcc* a = reinterpret_cast<const HorizonAcc*>(k.h_res + rec_at);
  const size_t take = struct_size < sizeof(HorizonRec) ? (size_t)struct_size : sizeof(HorizonRec);
  for (size_t r = 0; r < (size_t)pl.nrec; r++) {
    HorizonRec rec;
    horizon_finish(a[r], horizon_nth(mask, (uint32_t)(r % nd)), rec);
    memcpy(reinterpret_cast<char*>(out) + r * (size_t)struct_size, &rec, take);
  }
  if (nsuns) memcpy(lit_cells, k.h_res + cnt_at, (size_t)c.nm * nsuns * 4);
  return 0;
}

// ---- proximity: eight planes and no chain. M (0) the marks, BD (1) the rank scan in WATER mode and the envelopes' depths behind it,
// P (2) the columns' candidates, S and T (3, 4) the envelopes of the PROX_BANDS bands, then nearest, dist2 and group (5, 6, 7), written only where a plane or
// the histogram asks for them. LIST mode: the list goes into the result region with the tables' upload, M is filled and k_prox_mark
// scatters the list into it for every member; WATER mode: the census's labelling through the bare table, the scan of the root marks
// and k_prox_mark turning roots into ranks. Then k_prox_columns, k_prox_envelope, k_prox_query and, with bins, k_prox_hist on the
// zeroed rows. The region holds the counts, the records, the rows and the list; all but the list copied back with the planes asked
// for, one synchronisation.
static_assert(sizeof(smx_proximity_record) == 64 && sizeof(ProxRec) == sizeof(smx_proximity_record) && offsetof(smx_proximity_record, dist2_max) == offsetof(ProxRec, dist2_max) &&
              offsetof(smx_proximity_record, flags) == offsetof(ProxRec, flags) && offsetof(smx_proximity_record, dist2_sum) == offsetof(ProxRec, dist2_sum) &&
              offsetof(smx_proximity_record, x0) == offsetof(ProxRec, x0) && offsetof(smx_proximity_record, reserved) == offsetof(ProxRec, reserved) &&
              (uint32_t)SMX_PROXIMITY_MAX_BINS == PROX_MAX_BINS && (uint32_t)SMX_PROXIMITY_MAX_SIDE == PROX_MAX_SIDE, "smx_proximity_record layout");
static int prox_run(const AnalysisCall& c, AnalysisScratch& k, const uint32_t* cells, uint32_t n, smx_proximity_record* out, uint64_t struct_size, uint32_t cap,
                    uint32_t* nrecords, uint32_t* hist, uint32_t nbins, uint32_t bin_width, uint32_t* nearest, uint32_t* group, uint32_t* dist2) {
  const bool list = cells != nullptr;
  AnalysisPlan pl;
  if (int rc = plan_members(c, list ? n : cap, list ? CAP_CELLS : CAP_BLOCKS, pl)) return rc;   // (LIST: n distinct cells inside every member: every member keeps n records)
  unsigned columns = 1, rows = 1, marks = 1;
  for (const LakeMember& m : pl.tab) {
    columns = std::max(columns, (unsigned)m.dimx);
    rows = std::max(rows, (unsigned)(((uint64_t)m.dimy * prox_bands(m, PROX_BANDS) + PROX_ENV_LANES - 1) / PROX_ENV_LANES));
    marks = std::max(marks, (unsigned)prox_mark_blocks(m, list, n, LAKE_LANES));
  }
  AnalysisScratch::Need need;
  const size_t rec_at = counts_pad(c.nm), hist_at = rec_at + (size_t)pl.nrec * sizeof(ProxAcc);
  const size_t hist_bytes = (size_t)pl.nrec * nbins * 4, list_at = hist_at + ((hist_bytes + 63) & ~(size_t)63);
  need.words = (size_t)pl.words; need.planes = 8; need.members = c.nm; need.res_bytes = list_at + (size_t)n * 4;
  if (!list && !scan_bytes(c, lake_marks(nullptr), pl.words, need.temp_bytes)) return -1;
  if (int rc = analysis_reserve(c, k, need, "proximity", pl.nrec)) return rc;
  const ProxPlanes p{k.plane[0], k.plane[1], k.plane[2], k.plane[3], k.plane[4]};
  uint32_t* const d_nearest = nearest ? k.plane[5] : nullptr;
  uint32_t* const d_dist2 = dist2 || nbins ? k.plane[6] : nullptr;
  uint32_t* const d_group = group || nbins ? k.plane[7] : nullptr;
  uint32_t* d_n = reinterpret_cast<uint32_t*>(k.d_res);
  ProxAcc* acc = reinterpret_cast<ProxAcc*>(k.d_res + rec_at);
  uint32_t* d_hist = reinterpret_cast<uint32_t*>(k.d_res + hist_at);
  uint32_t* d_list = reinterpret_cast<uint32_t*>(k.d_res + list_at);
  const LakeMember* bare = k.d_tab + c.nm;
  if (list) memcpy(k.h_res + list_at, cells, (size_t)n * 4);
  put_table(k, pl, 0, false); put_table(k, pl, 1, true);
  bool ok = send_tables(c, k, 0, 2);
  ok = ok && (!list || hipMemcpyAsync(d_list, k.h_res + list_at, (size_t)n * 4, hipMemcpyHostToDevice, c.st) == hipSuccess);
  ok = ok && (!list || hipMemsetAsync(p.M, 0xFF, (size_t)pl.words * 4, c.st) == hipSuccess);
  ok = ok && (!nbins || !hist_bytes || hipMemsetAsync(d_hist, 0, hist_bytes, c.st) == hipSuccess);
  if (ok && !list) {
    launch_lake_labels(pl, c.st, bare, p.M, nullptr);
    ok = scan_words(k, lake_marks(p.M), p.BD, pl.words, c.st);
  }
  if (ok) {
    hipLaunchKernelGGL(k_prox_mark, dim3(marks, c.nm), pl.wg, 0, c.st, k.d_tab, p, list ? d_list : nullptr, n, acc, d_n);
    hipLaunchKernelGGL(k_prox_columns, dim3(columns, c.nm), pl.wg, 0, c.st, k.d_tab, p);
    hipLaunchKernelGGL(k_prox_envelope, dim3(rows, c.nm), dim3(PROX_ENV_LANES), 0, c.st, k.d_tab, p, PROX_BANDS);
    hipLaunchKernelGGL(k_prox_query, pl.gs, pl.wg, 0, c.st, k.d_tab, p, PROX_BANDS, acc, d_nearest, d_dist2, d_group);
    if (nbins && hist_bytes) hipLaunchKernelGGL(k_prox_hist, pl.gs, pl.wg, 0, c.st, k.d_tab, d_dist2, d_group, d_hist, nbins, bin_width);
  }
  ok = ok && hipGetLastError() == hipSuccess;
  ok = copy_back(c, ok, k.h_res, k.d_res, hist_at + hist_bytes);
  // (smx_proximity only: one map, off = 0, so a plane index is a cell index)
  ok = copy_back(c, ok, nearest, d_nearest, (size_t)pl.words * 4);
  ok = copy_back(c, ok, dist2, d_dist2, (size_t)pl.words * 4);
  ok = copy_back(c, ok, group, d_group, (size_t)pl.words * 4);
  if (analysis_wait(c, ok, "proximity")) return -1;
  uint32_t* const counts = reinterpret_cast<uint32_t*>(k.h_res);
  if (list) for (uint32_t i = 0; i < c.nm; i++) counts[i] = n;   // (LIST: a record per listed cell, no count comes back)
  const ProxAcc* a = reinterpret_cast<const ProxAcc*>(k.h_res + rec_at);
  const uint32_t* rows_back = reinterpret_cast<const uint32_t*>(k.h_res + hist_at);
  for (uint32_t i = 0; nbins && i < c.nm; i++) {   // the rows of the records that are written
    const uint32_t w = std::min(counts[i], std::min(pl.tab[i].cap, cap));
    if (w) memcpy(hist + (size_t)i * cap * nbins, rows_back + (size_t)pl.tab[i].rec0 * nbins, (size_t)w * nbins * 4);
  }
  cut_records<ProxRec>(pl, counts, out, struct_size, cap, nrecords, [a](size_t j, ProxRec& rec) -> const ProxRec& { prox_finish(a[j], rec); return rec; });
  return 0;
}

// ---- dispersed flow: planes T, B, R of the chain, P, RC, the list plane Q, and the 64-bit plane AQ in the f64 plane's place. The
// drainage chain with its statistics and ITS records (first_cell, cells and flags of a dispersal record are the basin's), then
// k_disp_pending. k_disp_flow in the round loop: DISP_BATCH launches, then ONE word back -- a bit per launch that found cells in
// the range of a member, however many members; a launch that found none ends the loop (every launch retires all cells listed before it and the graph strictly descends in
// h: giving up after cells + 2 launches cannot happen). k_disp_fold, k_disp_peak; the counts, the two tables and the planes asked
// for copied back, the last synchronisation. The counter words: DISP_RING per member, then the batch's word.
static_assert(sizeof(smx_dispersal_record) == 64 && sizeof(DispRec) == sizeof(smx_dispersal_record) && offsetof(smx_dispersal_record, peak_cell) == offsetof(DispRec, peak_cell) &&
              offsetof(smx_dispersal_record, inflow_q24) == offsetof(DispRec, inflow_q24) && offsetof(smx_dispersal_record, peak_q24) == offsetof(DispRec, peak_q24) &&
              offsetof(smx_dispersal_record, givers) == offsetof(DispRec, givers), "smx_dispersal_record layout");
static_assert(sizeof(BasinAcc) % alignof(DispAcc) == 0, "the second table of the result region is aligned");
static int disp_run(const AnalysisCall& c, AnalysisScratch& k, uint32_t exponent, smx_dispersal_record* out, uint64_t struct_size, uint32_t cap, uint32_t* nbasins,
                    uint64_t* area, uint32_t* donors, uint32_t* receivers) {
  k.sweeps[0] = 0; k.batches = 0;
  AnalysisPlan pl;
  if (int rc = plan_members(c, cap, CAP_CELLS, pl)) return rc;
  AnalysisScratch::Need need;
  const size_t rec_at = counts_pad(c.nm), disp_at = rec_at + (size_t)pl.nrec * sizeof(BasinAcc);
  need.words = (size_t)pl.words; need.planes = 6; need.f64 = true; need.members = c.nm; need.count_words = (size_t)c.nm * DISP_RING + 16;
  need.res_bytes = disp_at + (size_t)pl.nrec * sizeof(DispAcc);
  if (!scan_bytes(c, lake_marks(nullptr), pl.words, need.temp_bytes)) return -1;
  if (int rc = analysis_reserve(c, k, need, "dispersal", pl.nrec)) return rc;
  const DispPlanes p{k.plane[0], k.plane[2], k.plane[3], k.plane[4], k.plane[5], reinterpret_cast<uint64_t*>(k.h64)};
  uint32_t* const B = k.plane[1];
  uint32_t* d_n = reinterpret_cast<uint32_t*>(k.d_res);
  BasinAcc* bacc = reinterpret_cast<BasinAcc*>(k.d_res + rec_at);
  DispAcc* acc = reinterpret_cast<DispAcc*>(k.d_res + disp_at);
  uint32_t* const ring = k.d_cnt;
  uint32_t* const d_busy = k.d_cnt + (size_t)c.nm * DISP_RING;
  uint32_t* const h_busy = k.h_cnt + (size_t)c.nm * DISP_RING;
  uint64_t largest = 0;
  for (uint32_t i = 0; i < c.nm; i++) largest = std::max<uint64_t>(largest, c.ms[i]->ncells);
  const dim3 gw(std::min<unsigned>(pl.gf.x, c.launch.cap(LAUNCH_FLOW)), pl.gf.y);
  c.launch.grid[LAUNCH_FLOW] = gw.x;
  put_table(k, pl, 0, false); put_table(k, pl, 1, true);
  bool ok = send_tables(c, k, 0, 2);
  ok = ok && hipMemsetAsync(ring, 0, (size_t)c.nm * DISP_RING * 4, c.st) == hipSuccess;
  if (ok) {
    ok = launch_drain_chain(pl, c.st, k, k.d_tab + c.nm, k.d_tab, p.T, B, p.R, bacc, d_n, nullptr, nullptr);
    if (ok) hipLaunchKernelGGL(k_disp_pending, pl.gt, pl.wg, 0, c.st, k.d_tab, p, acc, ring);
  }
  if (!ok) return analysis_wait(c, false, "the dispersal");
  uint64_t launched = 0;
  for (bool done = false; !done;) {
    if (launched >= largest + 2u) {
      (void)hipStreamSynchronize(c.st);
      c.err = std::string(c.who) + ": the ready list did not run empty within " + std::to_string(launched) + " launches (" + std::to_string(largest) + " cells)";
      return -1;
    }
    ok = hipMemsetAsync(d_busy, 0, 4, c.st) == hipSuccess;
    for (uint32_t j = 0; ok && j < DISP_BATCH; j++) hipLaunchKernelGGL(k_disp_flow, gw, pl.wg, 0, c.st, k.d_tab, (uint32_t)((launched + j) % 3u), exponent, p, acc, ring, d_busy, 1u << j);
    ok = ok && hipGetLastError() == hipSuccess;
    ok = copy_back(c, ok, h_busy, d_busy, 4);
    if (analysis_wait(c, ok, "the dispersal")) return -1;
    launched += DISP_BATCH; k.batches++;
    // (bit j: launch j of the batch found cells in some member's range. Once every list is empty it stays empty, so the set bits are
    // the batch's first launches, and a clear bit ends the loop.)
    k.sweeps[0] += (uint32_t)__builtin_popcount(*h_busy);
    done = *h_busy != (DISP_BATCH == 32u ? 0xFFFFFFFFu : (1u << (DISP_BATCH & 31u)) - 1u);
  }
  hipLaunchKernelGGL(k_disp_fold, pl.gs, pl.wg, 0, c.st, k.d_tab, p, acc);
  hipLaunchKernelGGL(k_disp_peak, pl.gf, pl.wg, 0, c.st, k.d_tab, p, acc, donors ? 1u : 0u, receivers ? 1u : 0u);
  ok = hipGetLastError() == hipSuccess;
  ok = copy_back(c, ok, k.h_res, k.d_res, need.res_bytes);
  // (smx_dispersal only: one map, off = 0)
  ok = copy_back(c, ok, area, p.AQ, (size_t)pl.words * 8);
  ok = copy_back(c, ok, donors, p.P, (size_t)pl.words * 4);
  ok = copy_back(c, ok, receivers, p.RC, (size_t)pl.words * 4);
  if (analysis_wait(c, ok, "the dispersal")) return -1;
  const BasinAcc* b = reinterpret_cast<const BasinAcc*>(k.h_res + rec_at);
  const DispAcc* a = reinterpret_cast<const DispAcc*>(k.h_res + disp_at);
  cut_records<DispRec>(pl, reinterpret_cast<const uint32_t*>(k.h_res), out, struct_size, cap, nbasins,
                       [a, b](size_t j, DispRec& rec) -> const DispRec& { disp_finish(b[j], a[j], rec); return rec; });
  return 0;
}

extern "C" {
int smx_lakes(smx_ctx* ctx, smx_lake* out, uint64_t struct_size, uint32_t cap, uint32_t* nlakes, uint32_t* labels) {
  if (!ctx) return -2;
  const AnalysisCall c = call_on("smx_lakes", ctx);
  int rc;
  if (!analysis_begin(c, "smx_lake", "nlakes", struct_size, nullptr, nlakes, out, cap, rc)) return rc;
  roctx_range rr("soilmx:lakes");
  HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
  return lakes_run(c, ctx->lakes, out, struct_size, cap, nlakes, labels);
}
int smx_ensemble_lakes(smx_ensemble* e, smx_lake* out, uint64_t struct_size, uint32_t cap_per_member, uint32_t* nlakes) {
  if (!e) return -2;
  const AnalysisCall c = call_on("smx_ensemble_lakes", e);
  int rc;
  if (!analysis_begin(c, "smx_lake", "nlakes", struct_size, nullptr, nlakes, out, cap_per_member, rc)) return rc;
  roctx_range rr("soilmx:ensemble_lakes");
  HIPCHK(e, hipSetDevice(e->device));
  return lakes_run(c, e->lakes, out, struct_size, cap_per_member, nlakes, nullptr);
}
int smx_drainage(smx_ctx* ctx, smx_basin* out, uint64_t struct_size, uint32_t cap, uint32_t* nbasins, uint32_t* receivers, uint32_t* labels, uint32_t* area) {
  if (!ctx) return -2;
  const AnalysisCall c = call_on("smx_drainage", ctx);
  int rc;
  if (!analysis_begin(c, "smx_basin", "nbasins", struct_size, nullptr, nbasins, out, cap, rc)) return rc;
  roctx_range rr("soilmx:drainage");
  HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
  return drain_run(c, ctx->drain, out, struct_size, cap, nbasins, receivers, labels, area);
}
int smx_ensemble_drainage(smx_ensemble* e, smx_basin* out, uint64_t struct_size, uint32_t cap_per_member, uint32_t* nbasins) {
  if (!e) return -2;
  const AnalysisCall c = call_on("smx_ensemble_drainage", e);
  int rc;
  if (!analysis_begin(c, "smx_basin", "nbasins", struct_size, nullptr, nbasins, out, cap_per_member, rc)) return rc;
  roctx_range rr("soilmx:ensemble_drainage");
  HIPCHK(e, hipSetDevice(e->device));
  return drain_run(c, e->drain, out, struct_size, cap_per_member, nbasins, nullptr, nullptr, nullptr);
}
int smx_streams(smx_ctx* ctx, uint32_t threshold, smx_segment* out, uint64_t struct_size, uint32_t cap, uint32_t* nstreams, uint32_t* order, uint32_t* segments,
                uint32_t* reach, uint32_t* heads) {
  if (!ctx) return -2;
  const AnalysisCall c = call_on("smx_streams", ctx);
  int rc;
  if (!analysis_begin(c, "smx_segment", "nstreams", struct_size, &threshold, nstreams, out, cap, rc)) return rc;
  roctx_range rr("soilmx:streams");
  HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
  return streams_run(c, ctx->streams, threshold, out, struct_size, cap, nstreams, order, segments, reach, heads);
}
int smx_ensemble_streams(smx_ensemble* e, uint32_t threshold, smx_segment* out, uint64_t struct_size, uint32_t cap_per_member, uint32_t* nstreams) {
  if (!e) return -2;
  const AnalysisCall c = call_on("smx_ensemble_streams", e);
  int rc;
  if (!analysis_begin(c, "smx_segment", "nstreams", struct_size, &threshold, nstreams, out, cap_per_member, rc)) return rc;
  roctx_range rr("soilmx:ensemble_streams");
  HIPCHK(e, hipSetDevice(e->device));
  return streams_run(c, e->streams, threshold, out, struct_size, cap_per_member, nstreams, nullptr, nullptr, nullptr, nullptr);
}
int smx_spill(smx_ctx* ctx, smx_spill_record* out, uint64_t struct_size, uint32_t cap, uint32_t* nbasins, double* filled) {
  if (!ctx) return -2;
  const AnalysisCall c = call_on("smx_spill", ctx);
  int rc;
  if (!analysis_begin(c, "smx_spill_record", "nbasins", struct_size, nullptr, nbasins, out, cap, rc)) return rc;
  roctx_range rr("soilmx:spill");
  HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
  return spill_run(c, ctx->spill, out, struct_size, cap, nbasins, filled);
}
int smx_ensemble_spill(smx_ensemble* e, smx_spill_record* out, uint64_t struct_size, uint32_t cap_per_member, uint32_t* nbasins) {
  if (!e) return -2;
  const AnalysisCall c = call_on("smx_ensemble_spill", e);
  int rc;
  if (!analysis_begin(c, "smx_spill_record", "nbasins", struct_size, nullptr, nbasins, out, cap_per_member, rc)) return rc;
  roctx_range rr("soilmx:ensemble_spill");
  HIPCHK(e, hipSetDevice(e->device));
  return spill_run(c, e->spill, out, struct_size, cap_per_member, nbasins, nullptr);
}
int smx_through(smx_ctx* ctx, smx_through_record* out, uint64_t struct_size, uint32_t cap, uint32_t* nbasins, uint32_t* through_area, uint32_t* outlets) {
  if (!ctx) return -2;
  const AnalysisCall c = call_on("smx_through", ctx);
  int rc;
  if (!analysis_begin(c, "smx_through_record", "nbasins", struct_size, nullptr, nbasins, out, cap, rc)) return rc;
  roctx_range rr("soilmx:through");
  HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
  return through_run(c, ctx->through, out, struct_size, cap, nbasins, through_area, outlets);
}
int smx_ensemble_through(smx_ensemble* e, smx_through_record* out, uint64_t struct_size, uint32_t cap_per_member, uint32_t* nbasins) {
  if (!e) return -2;
  const AnalysisCall c = call_on("smx_ensemble_through", e);
  int rc;
  if (!analysis_begin(c, "smx_through_record", "nbasins", struct_size, nullptr, nbasins, out, cap_per_member, rc)) return rc;
  roctx_range rr("soilmx:ensemble_through");
  HIPCHK(e, hipSetDevice(e->device));
  return through_run(c, e->through, out, struct_size, cap_per_member, nbasins, nullptr, nullptr);
}
int smx_hillslopes(smx_ctx* ctx, uint32_t threshold, smx_hillslope* out, uint64_t struct_size, uint32_t cap, uint32_t* nsegments, uint32_t* entry,
                   uint32_t* hillslope, uint32_t* straight, uint32_t* diagonal, double* hand) {
  if (!ctx) return -2;
  const AnalysisCall c = call_on("smx_hillslopes", ctx);
  int rc;
  if (!analysis_begin(c, "smx_hillslope", "nsegments", struct_size, &threshold, nsegments, out, cap, rc)) return rc;
  roctx_range rr("soilmx:hillslopes");
  HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
  return hills_run(c, ctx->hills, threshold, out, struct_size, cap, nsegments, entry, hillslope, straight, diagonal, hand);
}
int smx_ensemble_hillslopes(smx_ensemble* e, uint32_t threshold, smx_hillslope* out, uint64_t struct_size, uint32_t cap_per_member, uint32_t* nsegments) {
  if (!e) return -2;
  const AnalysisCall c = call_on("smx_ensemble_hillslopes", e);
  int rc;
  if (!analysis_begin(c, "smx_hillslope", "nsegments", struct_size, &threshold, nsegments, out, cap_per_member, rc)) return rc;
  roctx_range rr("soilmx:ensemble_hillslopes");
  HIPCHK(e, hipSetDevice(e->device));
  return hills_run(c, e->hills, threshold, out, struct_size, cap_per_member, nsegments, nullptr, nullptr, nullptr, nullptr, nullptr);
}
int smx_flowpaths(smx_ctx* ctx, smx_flowpath* out, uint64_t struct_size, uint32_t cap, uint32_t* nbasins, uint32_t* terminal, uint32_t* straight, uint32_t* diagonal,
                  double* drop, uint32_t* upstream, uint32_t* source, uint32_t* stem, uint32_t* profile, uint32_t profile_cap, uint32_t* nprofile) {
  if (!ctx) return -2;
  const AnalysisCall c = call_on("smx_flowpaths", ctx);
  int rc;
  if (!analysis_begin(c, "smx_flowpath", "nbasins", struct_size, nullptr, nbasins, out, cap, rc)) return rc;
  if (!profile && profile_cap) { ctx->err = "smx_flowpaths: profile is null while profile_cap is " + std::to_string(profile_cap); return -2; }
  roctx_range rr("soilmx:flowpaths");
  HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
  return paths_run(c, ctx->paths, out, struct_size, cap, nbasins, terminal, straight, diagonal, drop, upstream, source, stem, profile, profile_cap, nprofile);
}
int smx_ensemble_flowpaths(smx_ensemble* e, smx_flowpath* out, uint64_t struct_size, uint32_t cap_per_member, uint32_t* nbasins) {
  if (!e) return -2;
  const AnalysisCall c = call_on("smx_ensemble_flowpaths", e);
  int rc;
  if (!analysis_begin(c, "smx_flowpath", "nbasins", struct_size, nullptr, nbasins, out, cap_per_member, rc)) return rc;
  roctx_range rr("soilmx:ensemble_flowpaths");
  HIPCHK(e, hipSetDevice(e->device));
  return paths_run(c, e->paths, out, struct_size, cap_per_member, nbasins, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0u, nullptr);
}
// the checks of the two catchment calls behind analysis_begin's: the list, the records' room and the bins. Nothing is launched and
// nothing written before all of them hold. (The list is read last: a call refused for its sizes never looks at it.)
static bool catch_args_ok(const AnalysisCall& c, const uint32_t* cells, uint32_t n, const void* out, const uint32_t* hist, uint32_t nbins, double bin_height, int& rc) {
  auto no = [&](const std::string& why) { c.err = std::string(c.who) + ": " + why; rc = -2; return false; };
  if (!cells) return no("cells is null (the list of gauge cells)");
  if (n == 0) return no("n is 0 (at least one gauge)");
  if (!out) return no("out is null (" + std::to_string(n) + " records per map)");
  if (nbins > CATCH_MAX_BINS) return no("nbins is " + std::to_string(nbins) + " (0 to " + std::to_string(CATCH_MAX_BINS) + ")");
  if (nbins && !hist) return no("hist is null while nbins is " + std::to_string(nbins));
  if (nbins && !(bin_height > 0.0 && std::isfinite(bin_height))) return no("bin_height is " + std::to_string(bin_height) + " (finite and positive)");
  if ((uint64_t)n * nbins >= (1ull << 31)) return no("n * nbins is " + std::to_string((uint64_t)n * nbins) + " (below 2^31)");
  uint64_t least = ~0ull; uint32_t which = 0;
  for (uint32_t i = 0; i < c.nm; i++) if ((uint64_t)c.ms[i]->ncells < least) { least = c.ms[i]->ncells; which = i; }
  for (uint32_t i = 0; i < n; i++)
    if (cells[i] >= least)
      return no("cells[" + std::to_string(i) + "] is " + std::to_string(cells[i]) + ", outside " + (c.ensemble ? "member " + std::to_string(which) : std::string("the map")) + " (" +
                std::to_string(least) + " cells)");
  std::vector<uint64_t> seen((size_t)((least + 63) / 64), 0ull);   // a bit per cell of the smallest member: O(n) for a list of any length
  for (uint32_t i = 0; i < n; i++) {
    uint64_t& w = seen[cells[i] >> 6];
    const uint64_t bit = 1ull << (cells[i] & 63u);
    if (w & bit) {
      uint32_t of = 0u;
      while (cells[of] != cells[i]) of++;
      return no("cells[" + std::to_string(i) + "] repeats cells[" + std::to_string(of) + "] (cell " + std::to_string(cells[i]) + "): the gauges are distinct");
    }
    w |= bit;
  }
  return true;
}
int smx_catchments(smx_ctx* ctx, const uint32_t* cells, uint32_t n, smx_catchment* out, uint64_t struct_size, uint32_t* hist, uint32_t nbins, double bin_height,
                   uint32_t* gauge, uint32_t* straight, uint32_t* diagonal, double* drop) {
  if (!ctx) return -2;
  const AnalysisCall c = call_on("smx_catchments", ctx);
  int rc;
  if (!analysis_begin(c, "smx_catchment", "cells", struct_size, nullptr, &rc, nullptr, 0u, rc)) return rc;   // (no counts and no cap: n records a map)
  if (!catch_args_ok(c, cells, n, out, hist, nbins, bin_height, rc)) return rc;
  roctx_range rr("soilmx:catchments");
  HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
  return catch_run(c, ctx->catchments, cells, n, out, struct_size, hist, nbins, bin_height, gauge, straight, diagonal, drop);
}
int smx_ensemble_catchments(smx_ensemble* e, const uint32_t* cells, uint32_t n, smx_catchment* out, uint64_t struct_size, uint32_t* hist, uint32_t nbins,
                            double bin_height) {
  if (!e) return -2;
  const AnalysisCall c = call_on("smx_ensemble_catchments", e);
  int rc;
  if (!analysis_begin(c, "smx_catchment", "cells", struct_size, nullptr, &rc, nullptr, 0u, rc)) return rc;
  if (!catch_args_ok(c, cells, n, out, hist, nbins, bin_height, rc)) return rc;
  roctx_range rr("soilmx:ensemble_catchments");
  HIPCHK(e, hipSetDevice(e->device));
  return catch_run(c, e->catchments, cells, n, out, struct_size, hist, nbins, bin_height, nullptr, nullptr, nullptr, nullptr);
}
// the checks of the two horizon calls beside analysis_begin's: the mask, the records' room, the suns. Nothing is launched and nothing
// written before all of them hold. They need no device: a context asks them first, so that a context without one still names the offender.
static bool horizon_args_ok(const AnalysisCall& c, uint32_t mask, const void* out, const smx_sun* suns, uint32_t nsuns, const uint32_t* lit_cells, const uint32_t* lit, int& rc) {
  auto no = [&](const std::string& why) { c.err = std::string(c.who) + ": " + why; rc = -2; return false; };
  if (!out) return no("out is null (a record per selected direction and map)");
  if (mask == 0u) return no("directions is 0 (a mask of at least one of the 16 lattice directions)");
  if (mask >> HORIZON_DIRS) return no("directions is " + std::to_string(mask) + ": a bit above 15 is set (16 lattice directions)");
  if (nsuns > HORIZON_MAX_SUNS) return no("nsuns is " + std::to_string(nsuns) + " (0 to " + std::to_string(HORIZON_MAX_SUNS) + ")");
  if (nsuns && !suns) return no("suns is null while nsuns is " + std::to_string(nsuns));
  if (nsuns && !lit_cells) return no("lit_cells is null while nsuns is " + std::to_string(nsuns) + " (a count per sun and map)");
  if (lit && !nsuns) return no("lit is asked for while nsuns is 0");
  for (uint32_t i = 0; i < nsuns; i++) {
    if (suns[i].direction >= HORIZON_DIRS || !((mask >> suns[i].direction) & 1u))
      return no("suns[" + std::to_string(i) + "].direction is " + std::to_string(suns[i].direction) + ", not a direction of the mask " + std::to_string(mask));
    if (!(suns[i].tangent >= 0.0 && std::isfinite(suns[i].tangent)))
      return no("suns[" + std::to_string(i) + "].tangent is " + std::to_string(suns[i].tangent) + " (finite and not negative: the tangent of the sun's elevation)");
  }
  return true;
}
int smx_horizons(smx_ctx* ctx, uint32_t directions, uint32_t reach, smx_horizon_record* out, uint64_t struct_size, const smx_sun* suns, uint32_t nsuns,
                 uint32_t* lit_cells, double* slope, uint32_t* step, double* sky, uint32_t* open, uint32_t* lit) {
  if (!ctx) return -2;
  const AnalysisCall c = call_on("smx_horizons", ctx);
  int rc;
  if (c.partial || struct_size == 0) { analysis_begin(c, "smx_horizon_record", "lit_cells", struct_size, nullptr, &rc, nullptr, 0u, rc); return rc; }
  if (!horizon_args_ok(c, directions, out, suns, nsuns, lit_cells, lit, rc)) return rc;
  if (!analysis_begin(c, "smx_horizon_record", "lit_cells", struct_size, nullptr, &rc, nullptr, 0u, rc)) return rc;   // (no counts and no cap: nd records a map)
  roctx_range rr("soilmx:horizons");
  HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
  return horizons_run(c, ctx->horizons, directions, reach, out, struct_size, suns, nsuns, lit_cells, slope, step, sky, open, lit);
}
int smx_ensemble_horizons(smx_ensemble* e, uint32_t directions, uint32_t reach, smx_horizon_record* out, uint64_t struct_size, const smx_sun* suns, uint32_t nsuns,
                          uint32_t* lit_cells) {
  if (!e) return -2;
  const AnalysisCall c = call_on("smx_ensemble_horizons", e);
  int rc;
  if (!analysis_begin(c, "smx_horizon_record", "lit_cells", struct_size, nullptr, &rc, nullptr, 0u, rc)) return rc;   // (an empty ensemble: 0 before anything is looked at)
  if (!horizon_args_ok(c, directions, out, suns, nsuns, lit_cells, nullptr, rc)) return rc;
  roctx_range rr("soilmx:ensemble_horizons");
  HIPCHK(e, hipSetDevice(e->device));
  return horizons_run(c, e->horizons, directions, reach, out, struct_size, suns, nsuns, lit_cells, nullptr, nullptr, nullptr, nullptr, nullptr);
}
// the checks of the two proximity calls beside analysis_begin's: the mode, the list, the records' room, the bins and the members'
// sides. Nothing is launched and nothing written before all of them hold; they need no device. (The list is read last: a call
// refused for its sizes never looks at it.)
static bool prox_args_ok(const AnalysisCall& c, const uint32_t* cells, uint32_t n, const void* out, uint32_t cap, const uint32_t* nrecords, const uint32_t* hist, uint32_t nbins,
                         uint32_t bin_width, int& rc) {
  auto no = [&](const std::string& why) { c.err = std::string(c.who) + ": " + why; rc = -2; return false; };
  if (!nrecords) return no("nrecords is null (one count per map)");
  if (!cells && n) return no("cells is null while n is " + std::to_string(n) + " (a list, or null and 0 for the wet cells)");
  if (cells && !n) return no("n is 0 while cells is given (at least one listed cell, or null and 0 for the wet cells)");
  if (cells && cap < n) return no("cap is " + std::to_string(cap) + " while n is " + std::to_string(n) + " (a record per listed cell)");
  if (!out && cap) return no("out is null while cap is " + std::to_string(cap) + " (out may be null for counting, with cap 0)");
  if (nbins > PROX_MAX_BINS) return no("nbins is " + std::to_string(nbins) + " (0 to " + std::to_string(PROX_MAX_BINS) + ")");
  if (nbins && !hist) return no("hist is null while nbins is " + std::to_string(nbins));
  if (nbins && !bin_width) return no("bin_width is 0 while nbins is " + std::to_string(nbins) + " (at least 1)");
  if ((uint64_t)cap * nbins >= (1ull << 31)) return no("cap * nbins is " + std::to_string((uint64_t)cap * nbins) + " (below 2^31)");
  uint64_t least = ~0ull; uint32_t which = 0;
  for (uint32_t i = 0; i < c.nm; i++) {
    const smx_ctx* x = c.ms[i];
    if ((uint32_t)x->cfg.dimx > PROX_MAX_SIDE || (uint32_t)x->cfg.dimy > PROX_MAX_SIDE)
      return no((c.ensemble ? "member " + std::to_string(i) : std::string("the map")) + " is " + std::to_string(x->cfg.dimx) + " x " + std::to_string(x->cfg.dimy) +
                " (at most " + std::to_string(PROX_MAX_SIDE) + " cells a side: dist2 stays below 2^31)");
    if ((uint64_t)x->ncells < least) { least = x->ncells; which = i; }
  }
  for (uint32_t i = 0; i < n; i++)
    if (cells[i] >= least)
      return no("cells[" + std::to_string(i) + "] is " + std::to_string(cells[i]) + ", outside " + (c.ensemble ? "member " + std::to_string(which) : std::string("the map")) + " (" +
                std::to_string(least) + " cells)");
  // the first position that repeats an earlier one. A short list is sorted with its positions (nothing of the map's size is touched
  // for sixteen sites); a longer one sets a bit per cell of the smallest member, O(n) for a list of any length. (At 4096^2 sorting
  // 65 536 entries added 2.5 ms to a call, the 2 MB of bits far less: the sort is for lists a 4096th of the map and shorter.)
  uint32_t rep = 0xFFFFFFFFu;
  if ((uint64_t)n * 4096u < least) {
    std::vector<uint64_t> key(n);
    for (uint32_t i = 0; i < n; i++) key[i] = ((uint64_t)cells[i] << 32) | i;
    std::sort(key.begin(), key.end());
    for (uint32_t i = 1; i < n; i++)   // (of a run of equal cells the second entry is its first repeat)
      if ((key[i] >> 32) == (key[i - 1] >> 32) && (i < 2 || (key[i - 2] >> 32) != (key[i] >> 32))) rep = std::min(rep, (uint32_t)key[i]);
  } else {
    std::vector<uint64_t> seen(n ? (size_t)((least + 63) / 64) : 0u, 0ull);
    for (uint32_t i = 0; i < n && rep == 0xFFFFFFFFu; i++) {
      uint64_t& w = seen[cells[i] >> 6];
      const uint64_t bit = 1ull << (cells[i] & 63u);
      if (w & bit) rep = i;
      w |= bit;
    }
  }
  if (rep != 0xFFFFFFFFu) {
    uint32_t of = 0u;
    while (cells[of] != cells[rep]) of++;
    return no("cells[" + std::to_string(rep) + "] repeats cells[" + std::to_string(of) + "] (cell " + std::to_string(cells[rep]) + "): the sites are distinct");
  }
  return true;
}
int smx_proximity(smx_ctx* ctx, const uint32_t* cells, uint32_t n, smx_proximity_record* out, uint64_t struct_size, uint32_t cap, uint32_t* nrecords, uint32_t* hist,
                  uint32_t nbins, uint32_t bin_width, uint32_t* nearest, uint32_t* group, uint32_t* dist2) {
  if (!ctx) return -2;
  const AnalysisCall c = call_on("smx_proximity", ctx);
  int rc;
  const uint32_t some_count = 0u;   // (a counts pointer for the checks in front of it: a strip context and struct_size 0 are refused before it is looked at)
  if (c.partial || struct_size == 0) { analysis_begin(c, "smx_proximity_record", "nrecords", struct_size, nullptr, &some_count, nullptr, 0u, rc); return rc; }
  if (!prox_args_ok(c, cells, n, out, cap, nrecords, hist, nbins, bin_width, rc)) return rc;
  if (!analysis_begin(c, "smx_proximity_record", "nrecords", struct_size, nullptr, nrecords, out, cap, rc)) return rc;
  roctx_range rr("soilmx:proximity");
  HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
  return prox_run(c, ctx->proximity, cells, n, out, struct_size, cap, nrecords, hist, nbins, bin_width, nearest, group, dist2);
}
int smx_ensemble_proximity(smx_ensemble* e, const uint32_t* cells, uint32_t n, smx_proximity_record* out, uint64_t struct_size, uint32_t cap_per_member, uint32_t* nrecords,
                           uint32_t* hist, uint32_t nbins, uint32_t bin_width) {
  if (!e) return -2;
  const AnalysisCall c = call_on("smx_ensemble_proximity", e);
  int rc;
  const uint32_t some_count = 0u;   // (nrecords is prox_args_ok's to check, behind the empty ensemble)
  if (!analysis_begin(c, "smx_proximity_record", "nrecords", struct_size, nullptr, &some_count, nullptr, 0u, rc)) return rc;   // (an empty ensemble: 0 before anything is looked at)
  if (!prox_args_ok(c, cells, n, out, cap_per_member, nrecords, hist, nbins, bin_width, rc)) return rc;
  roctx_range rr("soilmx:ensemble_proximity");
  HIPCHK(e, hipSetDevice(e->device));
  return prox_run(c, e->proximity, cells, n, out, struct_size, cap_per_member, nrecords, hist, nbins, bin_width, nullptr, nullptr, nullptr);
}
int smx_dispersal(smx_ctx* ctx, uint32_t exponent, smx_dispersal_record* out, uint64_t struct_size, uint32_t cap, uint32_t* nbasins, uint64_t* area, uint32_t* donors,
                  uint32_t* receivers) {
  if (!ctx) return -2;
  const AnalysisCall c = call_on("smx_dispersal", ctx);
  int rc;
  if (!analysis_begin(c, "smx_dispersal_record", "nbasins", struct_size, nullptr, nbasins, out, cap, rc)) return rc;
  if (exponent > DISP_MAX_EXPONENT) { ctx->err = "smx_dispersal: exponent is " + std::to_string(exponent) + " (0 to 16)"; return -2; }
  roctx_range rr("soilmx:dispersal");
  HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
  return disp_run(c, ctx->disp, exponent, out, struct_size, cap, nbasins, area, donors, receivers);
}
int smx_ensemble_dispersal(smx_ensemble* e, uint32_t exponent, smx_dispersal_record* out, uint64_t struct_size, uint32_t cap_per_member, uint32_t* nbasins) {
  if (!e) return -2;
  const AnalysisCall c = call_on("smx_ensemble_dispersal", e);
  int rc;
  if (exponent > DISP_MAX_EXPONENT) { e->err = "smx_ensemble_dispersal: exponent is " + std::to_string(exponent) + " (0 to 16)"; return -2; }
  if (!analysis_begin(c, "smx_dispersal_record", "nbasins", struct_size, nullptr, nbasins, out, cap_per_member, rc)) return rc;
  roctx_range rr("soilmx:ensemble_dispersal");
  HIPCHK(e, hipSetDevice(e->device));
  return disp_run(c, e->disp, exponent, out, struct_size, cap_per_member, nbasins, nullptr, nullptr, nullptr);
}
// (sweeps launched, batches) of the last spill call; (level sweeps, hop sweeps, batches) of the last through call
static int sweeps_of(const AnalysisScratch& k, std::string& err, const char* who, uint32_t* a, uint32_t* b, uint32_t* batches) {
  if (!a || !b || !batches) { err = std::string(who) + ": a null argument"; return -2; }
  *a = k.sweeps[0]; *b = k.sweeps[1]; *batches = k.batches;
  return 0;
}
int smx_get_spill_sweeps(smx_ctx* ctx, uint32_t* sweeps, uint32_t* batches) {
  uint32_t none;
  return ctx ? sweeps_of(ctx->spill, ctx->err, "smx_get_spill_sweeps", sweeps, &none, batches) : -2;
}
int smx_ensemble_get_spill_sweeps(smx_ensemble* e, uint32_t* sweeps, uint32_t* batches) {
  uint32_t none;
  return e ? sweeps_of(e->spill, e->err, "smx_ensemble_get_spill_sweeps", sweeps, &none, batches) : -2;
}
int smx_get_through_sweeps(smx_ctx* ctx, uint32_t* level_sweeps, uint32_t* hop_sweeps, uint32_t* batches) {
  return ctx ? sweeps_of(ctx->through, ctx->err, "smx_get_through_sweeps", level_sweeps, hop_sweeps, batches) : -2;
}
int smx_ensemble_get_through_sweeps(smx_ensemble* e, uint32_t* level_sweeps, uint32_t* hop_sweeps, uint32_t* batches) {
  return e ? sweeps_of(e->through, e->err, "smx_ensemble_get_through_sweeps", level_sweeps, hop_sweeps, batches) : -2;
}
// (rounds that found cells in their range, batches) of the last dispersal call
int smx_get_dispersal_rounds(smx_ctx* ctx, uint32_t* rounds, uint32_t* batches) {
  uint32_t none;
  return ctx ? sweeps_of(ctx->disp, ctx->err, "smx_get_dispersal_rounds", rounds, &none, batches) : -2;
}
int smx_ensemble_get_dispersal_rounds(smx_ensemble* e, uint32_t* rounds, uint32_t* batches) {
  uint32_t none;
  return e ? sweeps_of(e->disp, e->err, "smx_ensemble_get_dispersal_rounds", rounds, &none, batches) : -2;
}

// The launch shape of the analyses' strided launches, on a context and on an ensemble: stored whole or not at all.
static int set_analysis_launch(AnalysisLaunch& a, std::string& err, const char* who, int32_t flow_blocks, int32_t relax_blocks, int32_t strata_blocks) {
  static const char* const name[3] = {"flow_blocks", "relax_blocks", "strata_blocks"};
  const int32_t v[3] = {flow_blocks, relax_blocks, strata_blocks};
  for (int i = 0; i < 3; i++)
    if (v[i] < 0 || (uint32_t)v[i] > AnalysisLaunch::most(i)) {
      err = std::string(who) + ": " + name[i] + " is " + std::to_string(v[i]) + ", outside 0.." + std::to_string(AnalysisLaunch::most(i)) + " (0: the default; nothing was changed)";
      return -2;
    }
  for (int i = 0; i < 3; i++) a.set[i] = v[i];
  return 0;
}
static int get_analysis_launch(const AnalysisLaunch& a, int32_t* blocks, uint32_t* last_grid) {
  for (int i = 0; i < 3; i++) {
    if (blocks) blocks[i] = (int32_t)a.cap(i);
    if (last_grid) last_grid[i] = a.grid[i];
  }
  return 0;
}
int smx_set_analysis_launch(smx_ctx* ctx, int32_t flow_blocks, int32_t relax_blocks, int32_t strata_blocks) {
  return ctx ? set_analysis_launch(ctx->launch, ctx->err, "smx_set_analysis_launch", flow_blocks, relax_blocks, strata_blocks) : -2;
}
int smx_ensemble_set_analysis_launch(smx_ensemble* e, int32_t flow_blocks, int32_t relax_blocks, int32_t strata_blocks) {
  return e ? set_analysis_launch(e->launch, e->err, "smx_ensemble_set_analysis_launch", flow_blocks, relax_blocks, strata_blocks) : -2;
}
int smx_get_analysis_launch(smx_ctx* ctx, int32_t* blocks, uint32_t* last_grid) { return ctx ? get_analysis_launch(ctx->launch, blocks, last_grid) : -2; }
int smx_ensemble_get_analysis_launch(smx_ensemble* e, int32_t* blocks, uint32_t* last_grid) { return e ? get_analysis_launch(e->launch, blocks, last_grid) : -2; }

// ---------------- reading the strata (smx_soil_totals / smx_ensemble_soil_totals / smx_soil_thickness / smx_cores; kernels: soil_strata.h) ----------------
static_assert(sizeof(smx_soil_total) == 48 && sizeof(StrataRec) == sizeof(smx_soil_total) && offsetof(smx_soil_total, flags) == offsetof(StrataRec, flags) &&
              (int)SMX_TOTALS_MAX_TYPES == STRATA_MAX_TYPES, "smx_soil_total layout");
static size_t strata_blocks(uint64_t items, size_t most) { return (size_t)std::max<uint64_t>(1, std::min<uint64_t>((items + STRATA_LANES - 1) / STRATA_LANES, most)); }
static size_t strata_pad(size_t bytes) { return (bytes + 63) & ~(size_t)63; }
static StrataMap strata_map(const smx_ctx* c) {
  StrataMap m;
  m.cells = c->d.cells; m.pool = c->d.pool; m.cap = c->cfg.pool_capacity; m.ncells = c->ncells; m.rec0 = 0u; m.index = 0u;
  return m;
}
// room for `buf`, `sec` and `host` bytes (0: not needed by this call); a failure leaves no scratch, no sticky error and a text
static int strata_room(const char* who, StrataScratch& k, DevMem& mem, size_t buf, size_t sec, size_t host, std::string& err) {
  // (every call that uses the scratch has waited for its stream before it returned: nothing queued still reads what is dropped)
  const bool ok = mem.grow(k.d_buf, k.buf_cap, buf, buf) == hipSuccess && mem.grow(k.d_sec, k.sec_cap, sec, sec) == hipSuccess &&
                  mem.grow(k.h_buf, k.h_cap, host, host, true) == hipSuccess;
  if (ok) return 0;
  (void)hipGetLastError();
  mem.drop(k.d_buf); mem.drop(k.d_sec); mem.drop(k.h_buf);
  k = StrataScratch();
  err = std::string(who) + ": out of memory for the scratch (" + std::to_string(buf + sec) + " bytes on the device, " + std::to_string(host) + " pinned)";
  return -1;
}
static std::string strata_bad_text(const char* who, const smx_ctx* c, uint64_t word, int member) {
  const unsigned long long cell = strata_bad_cell(word), dy = (unsigned long long)c->cfg.dimy;
  return std::string(who) + ": corrupt section chain" + (member >= 0 ? " in member " + std::to_string(member) : std::string()) + ", cell " + std::to_string(cell) +
         " (x " + std::to_string(cell / dy) + ", y " + std::to_string(cell % dy) + "): it leaves the pool or has more links than the pool holds (nothing was written)";
}

// One path for both totals calls: one table upload, one memset of the results, one launch, the results back, one synchronisation.
static int totals_run(const char* who, StrataScratch& k, AnalysisLaunch& launch, DevMem& mem, hipStream_t st, smx_ctx* const* ms, uint32_t nm, bool ensemble, smx_soil_total* out,
                      uint64_t struct_size, uint32_t ntypes, uint64_t* other_sections, std::string& err) {
  const size_t tab_bytes = strata_pad((size_t)nm * sizeof(StrataMap)), nrec = (size_t)nm * ntypes;
  const size_t res_bytes = (size_t)nm * 16 + nrec * sizeof(StrataRec);   // error words, counts of other sections, records
  if (int rc = strata_room(who, k, mem, tab_bytes + res_bytes, 0, tab_bytes + res_bytes, err)) return rc;
  StrataMap* tab = reinterpret_cast<StrataMap*>(k.h_buf);
  uint64_t most = 0;
  for (uint32_t i = 0; i < nm; i++) {
    tab[i] = strata_map(ms[i]);
    tab[i].rec0 = i * ntypes; tab[i].index = i;
    most = std::max<uint64_t>(most, ms[i]->ncells);
  }
  uint64_t* d_bad = reinterpret_cast<uint64_t*>(k.d_buf + tab_bytes);
  uint64_t* d_other = d_bad + nm;
  StrataRec* d_acc = reinterpret_cast<StrataRec*>(d_other + nm);
  bool ok = hipMemcpyAsync(k.d_buf, k.h_buf, (size_t)nm * sizeof(StrataMap), hipMemcpyHostToDevice, st) == hipSuccess &&
            hipMemsetAsync(d_bad, 0, res_bytes, st) == hipSuccess;
  if (ok) {
    const size_t bx = strata_blocks(most, std::max<size_t>(1, launch.cap(LAUNCH_STRATA) / nm));
    launch.grid[LAUNCH_STRATA] = (uint32_t)bx;
    hipLaunchKernelGGL(k_strata_totals, dim3((unsigned)bx, nm), dim3(STRATA_LANES), 0, st, reinterpret_cast<const StrataMap*>(k.d_buf), ntypes, d_acc, d_other, d_bad);
    ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(k.h_buf + tab_bytes, d_bad, res_bytes, hipMemcpyDeviceToHost, st) == hipSuccess;
  }
  const hipError_t se = hipStreamSynchronize(st);
  if (!ok || se != hipSuccess) { err = std::string(who) + ": the totals failed on the device (" + hipGetErrorString(se != hipSuccess ? se : hipGetLastError()) + ")"; return -1; }
  const uint64_t* bad = reinterpret_cast<const uint64_t*>(k.h_buf + tab_bytes);
  const uint64_t* oth = bad + nm;
  const StrataRec* acc = reinterpret_cast<const StrataRec*>(oth + nm);
  for (uint32_t i = 0; i < nm; i++)
    if (bad[i]) { err = strata_bad_text(who, ms[i], bad[i], ensemble ? (int)i : -1); return -5; }
  const size_t take = struct_size < sizeof(smx_soil_total) ? (size_t)struct_size : sizeof(smx_soil_total);
  for (size_t r = 0; r < nrec; r++) memcpy(reinterpret_cast<char*>(out) + r * (size_t)struct_size, acc + r, take);
  if (other_sections) memcpy(other_sections, oth, (size_t)nm * 8);
  return 0;
}
int smx_soil_totals(smx_ctx* ctx, smx_soil_total* out, uint64_t struct_size, uint32_t ntypes, uint64_t* other_sections) {
  if (!ctx) return -2;
  FULLMAP("smx_soil_totals")
  if (!out) { ctx->err = "smx_soil_totals: out is null"; return -2; }
  if (struct_size == 0) { ctx->err = "smx_soil_totals: struct_size is 0 (pass sizeof(smx_soil_total) of the header you compiled against)"; return -2; }
  if (ntypes < 1u || ntypes > (uint32_t)SMX_TOTALS_MAX_TYPES) { ctx->err = "smx_soil_totals: ntypes is " + std::to_string(ntypes) + ", outside 1..64"; return -2; }
  if (!ctx->stream) { ctx->err = "smx_soil_totals: a context without a device"; return -3; }
  roctx_range rr("soilmx:soil_totals");
  HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
  return totals_run("smx_soil_totals", ctx->strata, ctx->launch, ctx->mem, ctx->stream, &ctx, 1u, false, out, struct_size, ntypes, other_sections, ctx->err);
}
int smx_ensemble_soil_totals(smx_ensemble* e, smx_soil_total* out, uint64_t struct_size, uint32_t ntypes, uint64_t* other_sections) {
  if (!e) return -2;
  if (!e->stream) { e->err = "smx_ensemble_soil_totals: the ensemble has no device (smx_ensemble_create failed)"; return -3; }
  if (struct_size == 0) { e->err = "smx_ensemble_soil_totals: struct_size is 0 (pass sizeof(smx_soil_total) of the header you compiled against)"; return -2; }
  if (ntypes < 1u || ntypes > (uint32_t)SMX_TOTALS_MAX_TYPES) { e->err = "smx_ensemble_soil_totals: ntypes is " + std::to_string(ntypes) + ", outside 1..64"; return -2; }
  const uint32_t nm = (uint32_t)e->members.size();
  if (nm == 0) return 0;
  if (!out) { e->err = "smx_ensemble_soil_totals: out is null (ntypes records per member)"; return -2; }
  roctx_range rr("soilmx:ensemble_soil_totals");
  HIPCHK(e, hipSetDevice(e->device));
  return totals_run("smx_ensemble_soil_totals", e->strata, e->launch, e->mem, e->stream, e->members.data(), nm, true, out, struct_size, ntypes, other_sections, e->err);
}

int smx_soil_thickness(smx_ctx* ctx, const uint32_t* types, int32_t ntypes, double* thickness, double* cover, uint32_t* sections) {
  if (!ctx) return -2;
  FULLMAP("smx_soil_thickness")
  if (!types) { ctx->err = "smx_soil_thickness: types is null"; return -2; }
  if (ntypes < 1 || ntypes > STRATA_MAX_LIST) { ctx->err = "smx_soil_thickness: ntypes is " + std::to_string(ntypes) + ", outside 1..8"; return -2; }
  StrataTypes ty{};
  ty.n = (uint32_t)ntypes;
  for (int32_t a = 0; a < ntypes; a++) {
    ty.t[a] = types[a];
    for (int32_t b = 0; b < a; b++)
      if (types[a] == types[b]) { ctx->err = "smx_soil_thickness: type " + std::to_string(types[a]) + " is listed twice (entries " + std::to_string(b) + " and " + std::to_string(a) + ")"; return -2; }
  }
  if (!ctx->stream) { ctx->err = "smx_soil_thickness: a context without a device"; return -3; }
  roctx_range rr("soilmx:soil_thickness");
  HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
  StrataScratch& k = ctx->strata;
  const size_t vals = (size_t)ntypes * ctx->ncells;
  const size_t at_cover = thickness ? vals * 8 : 0, at_sec = at_cover + (cover ? vals * 8 : 0), sec_bytes = at_sec + (sections ? vals * 4 : 0);
  if (int rc = strata_room("smx_soil_thickness", k, ctx->mem, 64, sec_bytes, 64, ctx->err)) return rc;
  uint64_t* d_bad = reinterpret_cast<uint64_t*>(k.d_buf);
  double* d_th = thickness ? reinterpret_cast<double*>(k.d_sec) : nullptr;
  double* d_cv = cover ? reinterpret_cast<double*>(k.d_sec + at_cover) : nullptr;
  uint32_t* d_n = sections ? reinterpret_cast<uint32_t*>(k.d_sec + at_sec) : nullptr;
  HIPCHK(ctx, hipMemsetAsync(d_bad, 0, 8, ctx->stream));
  const unsigned nb = (unsigned)strata_blocks(ctx->ncells, ctx->launch.cap(LAUNCH_STRATA));
  ctx->launch.grid[LAUNCH_STRATA] = nb;
  hipLaunchKernelGGL(k_strata_thickness, dim3(nb), dim3(STRATA_LANES), 0, ctx->stream, strata_map(ctx), ty, d_th, d_cv, d_n, d_bad);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipMemcpyAsync(k.h_buf, d_bad, 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // the verdict first: a bad chain writes nothing to the caller
  const uint64_t bad = *reinterpret_cast<const uint64_t*>(k.h_buf);
  if (bad) { ctx->err = strata_bad_text("smx_soil_thickness", ctx, bad, -1); return -5; }
  if (thickness) HIPCHK(ctx, hipMemcpyAsync(thickness, d_th, vals * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (cover) HIPCHK(ctx, hipMemcpyAsync(cover, d_cv, vals * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (sections) HIPCHK(ctx, hipMemcpyAsync(sections, d_n, vals * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return 0;
}

int smx_cores(smx_ctx* ctx, const uint32_t* cells, uint32_t n, uint32_t* count, uint64_t cap, uint64_t* total, uint32_t* type, double* size, double* floor,
              double* sat) {
  if (!ctx) return -2;
  FULLMAP("smx_cores")
  if (!total) { ctx->err = "smx_cores: total is null"; return -2; }
  if (n == 0) { *total = 0; return 0; }
  if (!cells || !count) { ctx->err = std::string("smx_cores: ") + (cells ? "count" : "cells") + " is null"; return -2; }
  if (cap && (!type || !size || !floor || !sat)) { ctx->err = "smx_cores: a section array is null while cap is " + std::to_string(cap); return -2; }
  for (uint32_t i = 0; i < n; i++)
    if (cells[i] >= ctx->ncells) {
      ctx->err = "smx_cores: cells[" + std::to_string(i) + "] is " + std::to_string(cells[i]) + ", outside the map of " + std::to_string(ctx->ncells) + " cells";
      return -2;
    }
  if (!ctx->stream) { ctx->err = "smx_cores: a context without a device"; return -3; }
  roctx_range rr("soilmx:cores");
  HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
  StrataScratch& k = ctx->strata;
  hipStream_t st = ctx->stream;
  const size_t at_list = 64, at_count = at_list + strata_pad((size_t)n * 4), at_base = at_count + strata_pad((size_t)n * 4), at_temp = at_base + strata_pad((size_t)n * 8);
  size_t tb = 0;
  {
    const auto in = rocprim::make_transform_iterator(static_cast<const uint32_t*>(nullptr), CoreWidenFn{});
    HIPCHK(ctx, rocprim::exclusive_scan(nullptr, tb, in, static_cast<uint64_t*>(nullptr), 0ull, (size_t)n, rocprim::plus<uint64_t>(), st));
  }
  if (tb == 0) tb = 8;   // (a null temporary storage would make the scan a size query again)
  if (int rc = strata_room("smx_cores", k, ctx->mem, at_temp + tb, 0, 64, ctx->err)) return rc;
  uint64_t* d_word = reinterpret_cast<uint64_t*>(k.d_buf);   // [0] the error word, [1] the total
  uint32_t* d_list = reinterpret_cast<uint32_t*>(k.d_buf + at_list);
  uint32_t* d_count = reinterpret_cast<uint32_t*>(k.d_buf + at_count);
  uint64_t* d_base = reinterpret_cast<uint64_t*>(k.d_buf + at_base);
  const StrataMap m = strata_map(ctx);
  const unsigned nb = (unsigned)strata_blocks(n, ctx->launch.cap(LAUNCH_STRATA));
  ctx->launch.grid[LAUNCH_STRATA] = nb;
  HIPCHK(ctx, hipMemsetAsync(d_word, 0, 16, st));
  HIPCHK(ctx, hipMemcpyAsync(d_list, cells, (size_t)n * 4, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_core_count, dim3(nb), dim3(STRATA_LANES), 0, st, m, d_list, (uint64_t)n, d_count, d_word);
  {
    const auto in = rocprim::make_transform_iterator(static_cast<const uint32_t*>(d_count), CoreWidenFn{});
    HIPCHK(ctx, rocprim::exclusive_scan(k.d_buf + at_temp, tb, in, d_base, 0ull, (size_t)n, rocprim::plus<uint64_t>(), st));
  }
  hipLaunchKernelGGL(k_core_total, dim3(1), dim3(1), 0, st, d_count, d_base, (uint64_t)n, d_word + 1);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipMemcpyAsync(k.h_buf, d_word, 16, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));   // the verdict and the total first: they size what follows
  const uint64_t bad = reinterpret_cast<const uint64_t*>(k.h_buf)[0], tot = reinterpret_cast<const uint64_t*>(k.h_buf)[1];
  if (bad) { ctx->err = strata_bad_text("smx_cores", ctx, bad, -1); return -5; }
  *total = tot;
  HIPCHK(ctx, hipMemcpyAsync(count, d_count, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  if (tot > cap || tot == 0) {
    HIPCHK(ctx, hipStreamSynchronize(st));
    return tot > cap ? 1 : 0;
  }
  const size_t t8 = strata_pad((size_t)tot * 8);
  if (int rc = strata_room("smx_cores", k, ctx->mem, 0, 3 * t8 + (size_t)tot * 4, 0, ctx->err)) { hipStreamSynchronize(st); return rc; }
  double* d_size = reinterpret_cast<double*>(k.d_sec);
  double* d_floor = reinterpret_cast<double*>(k.d_sec + t8);
  double* d_sat = reinterpret_cast<double*>(k.d_sec + 2 * t8);
  uint32_t* d_type = reinterpret_cast<uint32_t*>(k.d_sec + 3 * t8);
  hipLaunchKernelGGL(k_core_scatter, dim3(nb), dim3(STRATA_LANES), 0, st, m, d_list, (uint64_t)n, d_count, d_base, tot, d_type, d_size, d_floor, d_sat);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipMemcpyAsync(type, d_type, (size_t)tot * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipMemcpyAsync(size, d_size, (size_t)tot * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipMemcpyAsync(floor, d_floor, (size_t)tot * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipMemcpyAsync(sat, d_sat, (size_t)tot * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  return 0;
}

// ---------------- the sediment budget (smx_budget / smx_ensemble_budget; kernels: soil_budget.h) ----------------
// One path for both calls, through the analyses' driver: the chain's call is the BASE alone (plan_members, the tables, the planes T, B
// and R, launch_drain_chain with its statistics -- once, whatever the member count) on the owner's stream and scratch, behind the
// work queued on the base's stream. The maps of NOW go into a table of their own in the result region, which holds, in this order:
// the base's basin count, the error words (the base's, then one per member), that table, the base's basin records, the members'
// budget records and their soil records. One upload, two memsets, the chain, k_budget_fold and k_budget_where for all members, the
// region back, one synchronisation; the planes (smx_budget only) are copied out behind the verdict and waited for once more.
static_assert(sizeof(smx_budget_basin) == 96 && sizeof(BudgetBasinRec) == sizeof(smx_budget_basin) && offsetof(smx_budget_basin, eroded_q40) == offsetof(BudgetBasinRec, eroded_q40) &&
              offsetof(smx_budget_basin, cut_max) == offsetof(BudgetBasinRec, cut_max) && offsetof(smx_budget_basin, cut_cell) == offsetof(BudgetBasinRec, cut_cell) &&
              offsetof(smx_budget_basin, flags) == offsetof(BudgetBasinRec, flags), "smx_budget_basin layout");
static_assert(sizeof(smx_budget_soil) == 64 && sizeof(BudgetSoilRec) == sizeof(smx_budget_soil) && offsetof(smx_budget_soil, cells_gained) == offsetof(BudgetSoilRec, cells_gained) &&
              offsetof(smx_budget_soil, flags) == offsetof(BudgetSoilRec, flags) && (int)SMX_TOTALS_MAX_TYPES == BUDGET_MAX_TYPES, "smx_budget_soil layout");
static int budget_run(const AnalysisCall& c, BudgetScratch& ks, smx_ctx* base, smx_budget_basin* out, uint64_t struct_size, uint32_t cap, uint32_t* nbasins,
                      smx_budget_soil* soils, uint64_t soil_struct_size, uint32_t ntypes, double* dground, double* dheight, int64_t* dsolid, int64_t* dwater) {
  AnalysisScratch& k = ks.a;
  const AnalysisCall cb{c.who, false, false, c.mem, c.st, &base, 1u, c.err, c.launch};   // the chain's call: the base alone
  AnalysisPlan pl;
  if (int rc = plan_members(cb, cap, CAP_CELLS, pl)) return rc;
  const uint32_t nm = c.nm, bcap = pl.tab[0].cap, nt = soils ? ntypes : 0u;
  if ((uint64_t)nm * bcap > 0xFFFFFFFEull) { c.err = std::string(c.who) + ": more than 2^32 - 2 records in one call"; return -2; }
  const size_t bad_at = counts_pad(1), tab_at = bad_at + strata_pad((size_t)(1u + nm) * 8), basin_at = tab_at + strata_pad((size_t)nm * sizeof(BudgetMap));
  const size_t acc_at = basin_at + strata_pad((size_t)bcap * sizeof(BasinAcc)), soil_at = acc_at + (size_t)nm * bcap * sizeof(BudgetAcc);
  const size_t res_bytes = soil_at + (size_t)nm * nt * sizeof(BudgetSoilRec);
  AnalysisScratch::Need need;
  need.words = (size_t)pl.words; need.planes = 3; need.members = 1; need.res_bytes = res_bytes;
  if (!scan_bytes(cb, lake_marks(nullptr), pl.words, need.temp_bytes)) return -1;
  if (int rc = analysis_reserve(cb, k, need, "budget", (uint64_t)nm * bcap)) return rc;
  double* const want64[4] = {dground, dheight, reinterpret_cast<double*>(dsolid), reinterpret_cast<double*>(dwater)};
  size_t nplanes = 0;
  for (double* w : want64) nplanes += w ? 1 : 0;
  const size_t plane_bytes = (size_t)pl.words * 8;
  // (every call that uses the planes has waited for its stream before it returned: nothing queued still writes what is dropped)
  if (c.mem.grow(ks.d_planes, ks.planes_cap, nplanes * plane_bytes, nplanes * plane_bytes) != hipSuccess) {
    (void)hipGetLastError();
    c.err = std::string(c.who) + ": out of memory for the planes (" + std::to_string(nplanes * plane_bytes) + " bytes on the device)";
    return -1;
  }
  double* d64[4] = {nullptr, nullptr, nullptr, nullptr};
  for (size_t j = 0, at = 0; j < 4; j++)
    if (want64[j]) d64[j] = reinterpret_cast<double*>(ks.d_planes + (at++) * plane_bytes);
  const BudgetPlanes planes{d64[0], d64[1], reinterpret_cast<int64_t*>(d64[2]), reinterpret_cast<int64_t*>(d64[3])};
  std::string why;
  if (fork_order(base, c.st, why)) { c.err = std::string(c.who) + ": " + why; return -1; }
  uint32_t* const T = k.plane[0]; uint32_t* const B = k.plane[1]; uint32_t* const R = k.plane[2];
  uint32_t* const d_n = reinterpret_cast<uint32_t*>(k.d_res);
  uint64_t* const d_bad = reinterpret_cast<uint64_t*>(k.d_res + bad_at);
  BudgetMap* const d_maps = reinterpret_cast<BudgetMap*>(k.d_res + tab_at);
  BasinAcc* const d_basin = reinterpret_cast<BasinAcc*>(k.d_res + basin_at);
  BudgetAcc* const d_acc = reinterpret_cast<BudgetAcc*>(k.d_res + acc_at);
  BudgetSoilRec* const d_soil = reinterpret_cast<BudgetSoilRec*>(k.d_res + soil_at);
  BudgetMap* const h_maps = reinterpret_cast<BudgetMap*>(k.h_res + tab_at);
  for (uint32_t i = 0; i < nm; i++) {
    const smx_ctx* x = c.ms[i];
    h_maps[i] = BudgetMap{x->d.cells, x->d.pool, (uint64_t)x->cfg.pool_capacity, i * bcap, i * nt, i, 0u};
  }
  const BudgetBase bb{base->d.cells, base->d.pool, (uint64_t)base->cfg.pool_capacity, base->cfg.dimx, base->cfg.dimy, bcap, nt};
  put_table(k, pl, 0, false); put_table(k, pl, 1, true);
  bool ok = send_tables(cb, k, 0, 2);
  ok = ok && hipMemcpyAsync(d_maps, h_maps, (size_t)nm * sizeof(BudgetMap), hipMemcpyHostToDevice, c.st) == hipSuccess;
  ok = ok && hipMemsetAsync(d_bad, 0, tab_at - bad_at, c.st) == hipSuccess;
  ok = ok && (res_bytes == acc_at || hipMemsetAsync(d_acc, 0, res_bytes - acc_at, c.st) == hipSuccess);
  if (ok) ok = launch_drain_chain(pl, c.st, k, k.d_tab + 1, k.d_tab, T, B, R, d_basin, d_n, nullptr, nullptr);
  if (ok && (bcap || nt || nplanes)) {   // (a counting call asks for nothing the columns hold: the chain alone)
    hipLaunchKernelGGL(k_budget_fold, dim3(budget_tiles(bb.dimx, bb.dimy, BUDGET_TX, BUDGET_TY), nm), pl.wg, 0, c.st, bb, d_maps, T, d_acc, d_soil, d_bad, planes);
    if (bcap) hipLaunchKernelGGL(k_budget_where, dim3(pl.gf.x, nm), pl.wg, 0, c.st, bb, d_maps, T, d_acc);
  }
  ok = ok && hipGetLastError() == hipSuccess;
  ok = copy_back(c, ok, k.h_res, k.d_res, res_bytes);
  if (analysis_wait(c, ok, "the budget")) return -1;
  const uint64_t* bad = reinterpret_cast<const uint64_t*>(k.h_res + bad_at);
  for (uint32_t i = 0; i <= nm; i++) {
    if (!bad[i]) continue;
    const unsigned long long cell = strata_bad_cell(bad[i]), dy = (unsigned long long)base->cfg.dimy;
    c.err = std::string(c.who) + ": corrupt section chain in " + (i == 0 ? std::string("the base map") : c.ensemble ? "member " + std::to_string(i - 1) : std::string("the context's map")) +
            ", cell " + std::to_string(cell) + " (x " + std::to_string(cell / dy) + ", y " + std::to_string(cell % dy) +
            "): it leaves the pool or has more links than the pool holds (nothing was written)";
    return -5;
  }
  const uint32_t n = *reinterpret_cast<const uint32_t*>(k.h_res), w = std::min(n, std::min(bcap, cap));
  const BasinAcc* b = reinterpret_cast<const BasinAcc*>(k.h_res + basin_at);
  const BudgetAcc* a = reinterpret_cast<const BudgetAcc*>(k.h_res + acc_at);
  const BudgetSoilRec* s = reinterpret_cast<const BudgetSoilRec*>(k.h_res + soil_at);
  const size_t take = struct_size < sizeof(BudgetBasinRec) ? (size_t)struct_size : sizeof(BudgetBasinRec);
  const size_t stake = soil_struct_size < sizeof(BudgetSoilRec) ? (size_t)soil_struct_size : sizeof(BudgetSoilRec);
  *nbasins = n;
  for (size_t i = 0; i < nm; i++) {
    for (uint32_t r = 0; r < w; r++) {
      BudgetBasinRec rec;
      budget_finish(b[r], a[i * bcap + r], rec);
      memcpy(reinterpret_cast<char*>(out) + (i * cap + r) * (size_t)struct_size, &rec, take);
    }
    for (uint32_t t = 0; t < nt; t++) memcpy(reinterpret_cast<char*>(soils) + (i * nt + t) * (size_t)soil_struct_size, s + i * nt + t, stake);
  }
  if (!nplanes) return 0;
  ok = true;
  for (size_t j = 0; j < 4; j++) ok = copy_back(c, ok, want64[j], d64[j], plane_bytes);
  return analysis_wait(c, ok, "copying the planes");
}
// the checks of the two calls behind analysis_begin's: what the base has to be
static bool budget_base_ok(const AnalysisCall& c, smx_ctx* base, int device, const smx_budget_soil* soils, uint64_t soil_struct_size, uint32_t ntypes, int& rc) {
  auto no = [&](int code, const std::string& why) { c.err = std::string(c.who) + ": " + why; rc = code; return false; };
  if (base->partial()) return no(-2, "the base is a strip context (smx_create_strip): it holds only a part of the map");
  if (base->cfg.device != device) return no(-2, "the base lives on another device");
  if (soils && soil_struct_size == 0) return no(-2, "soil_struct_size is 0 (pass sizeof(smx_budget_soil) of the header you compiled against)");
  if (soils && (ntypes < 1u || ntypes > (uint32_t)SMX_TOTALS_MAX_TYPES)) return no(-2, "ntypes is " + std::to_string(ntypes) + ", outside 1..64");
  for (uint32_t i = 0; i < c.nm; i++) {
    const smx_ctx* x = c.ms[i];
    const std::string who = c.ensemble ? "member " + std::to_string(i) : std::string("the context");
    if (x == base) return no(-2, "the base is " + who + " itself");
    if (x->cfg.dimx != base->cfg.dimx || x->cfg.dimy != base->cfg.dimy)
      return no(-2, who + " is " + std::to_string(x->cfg.dimx) + "x" + std::to_string(x->cfg.dimy) + ", the base is " + std::to_string(base->cfg.dimx) + "x" + std::to_string(base->cfg.dimy));
  }
  if (!base->stream) return no(-3, "the base has no device");
  return true;
}
int smx_budget(smx_ctx* ctx, smx_ctx* base, smx_budget_basin* out, uint64_t struct_size, uint32_t cap, uint32_t* nbasins, smx_budget_soil* soils,
               uint64_t soil_struct_size, uint32_t ntypes, double* dground, double* dheight, int64_t* dsolid, int64_t* dwater) {
  if (!ctx) return -2;
  if (!base) { ctx->err = "smx_budget: base is null"; return -2; }
  const AnalysisCall c = call_on("smx_budget", ctx);
  int rc;
  if (!analysis_begin(c, "smx_budget_basin", "nbasins", struct_size, nullptr, nbasins, out, cap, rc)) return rc;
  if (!budget_base_ok(c, base, ctx->cfg.device, soils, soil_struct_size, ntypes, rc)) return rc;
  roctx_range rr("soilmx:budget");
  HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
  return budget_run(c, ctx->budget, base, out, struct_size, cap, nbasins, soils, soil_struct_size, ntypes, dground, dheight, dsolid, dwater);
}
int smx_ensemble_budget(smx_ensemble* e, smx_ctx* base, smx_budget_basin* out, uint64_t struct_size, uint32_t cap_per_member, uint32_t* nbasins,
                        smx_budget_soil* soils, uint64_t soil_struct_size, uint32_t ntypes) {
  if (!e) return -2;
  if (!base) { e->err = "smx_ensemble_budget: base is null"; return -2; }
  const AnalysisCall c = call_on("smx_ensemble_budget", e);
  int rc;
  if (!analysis_begin(c, "smx_budget_basin", "nbasins", struct_size, nullptr, nbasins, out, cap_per_member, rc)) return rc;
  if (!budget_base_ok(c, base, e->device, soils, soil_struct_size, ntypes, rc)) return rc;
  roctx_range rr("soilmx:ensemble_budget");
  HIPCHK(e, hipSetDevice(e->device));
  return budget_run(c, e->budget, base, out, struct_size, cap_per_member, nbasins, soils, soil_struct_size, ntypes, nullptr, nullptr, nullptr, nullptr);
}

// ---------------- point operations ----------------
static int point_op(smx_ctx* ctx, const PointOp& o, double* out) {
  hipLaunchKernelGGL(k_point_op, dim3(1), dim3(64), 0, ctx->stream, ctx->d, o, ctx->d_scratch);
  if (out) HIPCHK(ctx, hipMemcpyAsync(out, ctx->d_scratch, 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return 0;
}
static bool inb(smx_ctx* ctx, int x, int y) {
  if (x < 0 || y < 0 || x >= ctx->cfg.dimx || y >= ctx->cfg.dimy) { ctx->err = "cell out of bounds"; return false; }
  if (ctx->partial()) { ctx->err = "point operations are not available on a strip context (smx_create_strip)"; return false; }
  return true;
}
int smx_add(smx_ctx* ctx, int32_t x, int32_t y, double size, uint32_t type) {
  if (!inb(ctx, x, y)) return -2;
  PointOp o{}; o.op = 0; o.x = x; o.y = y; o.a = size; o.type = type; return point_op(ctx, o, nullptr);
}
int smx_remove(smx_ctx* ctx, int32_t x, int32_t y, double h, double* remainder) {
  if (!inb(ctx, x, y)) return -2;
  PointOp o{}; o.op = 1; o.x = x; o.y = y; o.a = h; double r = 0; int rc = point_op(ctx, o, &r); if (remainder) *remainder = r; return rc;
}
int smx_particle_cascade(smx_ctx* ctx, float px, float py, int32_t transferloop) {
  FULLMAP("smx_particle_cascade")
  if (!(px == px) || !(py == py) || !inb(ctx, (int)roundf(px), (int)roundf(py))) { ctx->err = "cell out of bounds"; return -2; }
  PointOp o{}; o.op = 2; o.px = px; o.py = py; o.k = transferloop; return point_op(ctx, o, nullptr);
}
int smx_water_cascade(smx_ctx* ctx, int32_t x, int32_t y, int32_t spill) {
  if (!inb(ctx, x, y)) return -2;
  PointOp o{}; o.op = 3; o.x = x; o.y = y; o.k = spill; return point_op(ctx, o, nullptr);
}
int smx_seep(smx_ctx* ctx, int32_t x, int32_t y) {
  if (!inb(ctx, x, y)) return -2;
  PointOp o{}; o.op = 4; o.x = x; o.y = y; return point_op(ctx, o, nullptr);
}

int smx_top(smx_ctx* ctx, int32_t x, int32_t y, uint32_t* type, double* size, double* floor, double* sat, int32_t* empty) {
  if (!inb(ctx, x, y)) return -2;
  Sec r;
  HIPCHK(ctx, hipMemcpyAsync(&r, ctx->d.cells + ((size_t)x * ctx->cfg.dimy + y), sizeof(Sec), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  const bool e = r.type == EMPTY;
  if (empty) *empty = e ? 1 : 0;
  if (type) *type = e ? 0u : r.type;
  if (size) *size = r.size;
  if (floor) *floor = r.floor;
  if (sat) *sat = r.sat;
  return 0;
}

// ---------------- observability ----------------
int smx_digest(smx_ctx* ctx, double* sumh, uint64_t* nsec, uint64_t* typehash) {   // (a strip context digests the range it holds)
  const size_t n = ctx->lcells;
  const uint64_t cap = ctx->cfg.pool_capacity;
  std::vector<Sec> cells(n);
  HIPCHK(ctx, hipMemcpyAsync(cells.data(), ctx->cells_alloc, n * sizeof(Sec), hipMemcpyDeviceToHost, ctx->stream));
  // {type, prev} = the last 8 bytes of every 32-byte pool record: one strided 2D copy instead of the whole pool
  std::vector<uint64_t> tp(cap);
  HIPCHK(ctx, hipMemcpy2DAsync(tp.data(), 8, reinterpret_cast<const char*>(ctx->d.pool) + 24, sizeof(Sec), 8, cap, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  double sh = 0.0; uint64_t ns = 0, h = 1469598103934665603ull;
  for (size_t c = 0; c < n; c++) {
    const Sec& t = cells[c];
    if (t.type == EMPTY) { sh += 0.0; continue; }
    sh += t.floor + t.size;
    h = (h ^ (uint64_t)t.type) * 1099511628211ull; ns++;
    uint32_t pv = t.prev; uint64_t guard = 0;
    while (pv != NIL) {
      if (pv >= cap || ++guard > cap) { ctx->err = "smx_digest: corrupt section chain"; return -5; }
      const uint64_t w = tp[pv];
      h = (h ^ (uint64_t)(uint32_t)w) * 1099511628211ull; ns++;
      pv = (uint32_t)(w >> 32);
    }
  }
  if (sumh) *sumh = sh;
  if (nsec) *nsec = ns;
  if (typehash) *typehash = h;
  return 0;
}
// The structs behind the two getters have grown (round 2: three streaming-kernel timers; round 4: two speculative-engine counters;
// round 5: step-kernel launch totals). A caller says how large ITS struct is and gets exactly that prefix; the unsized entry points
// keep writing the layout they had when they were introduced (16 / 18 words), so a binary built against an older header is never
// written past its struct.
int smx_get_counters_sized(smx_ctx* ctx, smx_counters* out, uint64_t struct_size) {
  unsigned long long c[C_COUNT];
  RandState r;
  HIPCHK(ctx, hipMemcpyAsync(c, ctx->d.ctr, sizeof(c), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(&r, ctx->d.rnd, sizeof(r), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  smx_counters t;
  memset(&t, 0, sizeof(t));
  t.steps_water_top = c[C_STEPS_WATER_TOP]; t.steps_water_all = c[C_STEPS_WATER_ALL]; t.steps_wind = c[C_STEPS_WIND];
  t.nested_particles = c[C_NESTED]; t.floods = c[C_FLOODS]; t.cascade_calls = c[C_CASCADE_CALLS];
  t.cascade_transfers = c[C_CASCADE_TRANSFERS]; t.wcascade_calls = c[C_WCASCADE_CALLS];
  t.grid_active_cells = c[C_GRID_ACTIVE]; t.rand_calls = r.calls;
  t.pool_free = ctx->cfg.pool_capacity - c[C_LIVE_SECTIONS]; t.pool_overflow = c[C_POOL_OVERFLOW];
  t.spec_rounds = ctx->spec_rounds; t.spec_aborts = ctx->spec_aborts;
  t.reserved[0] = ctx->spec_fallbacks; t.reserved[1] = ctx->spec_executed;
  t.spec_subphases_cut = ctx->spec_subphases_cut; t.spec_serial_particles = ctx->spec_serial_particles;
  t.flood_nested_steps = c[C_FLOOD_NESTED_STEPS]; t.grid_nested_steps = c[C_GRID_NESTED_STEPS];
  memcpy(out, &t, struct_size < sizeof(t) ? (size_t)struct_size : sizeof(t));
  return 0;
}
int smx_get_counters(smx_ctx* ctx, smx_counters* out) { return smx_get_counters_sized(ctx, out, 16 * sizeof(uint64_t)); }   // the layout of rounds 1-3
int smx_get_timing_sized(smx_ctx* ctx, smx_timing* out, uint64_t struct_size) {
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  drain_events(ctx);
  memcpy(out, &ctx->timing, struct_size < sizeof(ctx->timing) ? (size_t)struct_size : sizeof(ctx->timing));
  return 0;
}
int smx_get_timing(smx_ctx* ctx, smx_timing* out) { return smx_get_timing_sized(ctx, out, 144); }   // the layout of rounds 2-4
int smx_timing_reset(smx_ctx* ctx) {
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  drain_events(ctx);
  memset(&ctx->timing, 0, sizeof(ctx->timing));
  return 0;
}

}  // extern "C"

#include "soil_strips_host.h"

// ---------------- LBM wind: lbmwind.h:75-197 + shader/LBM/*.cs, shader/move.cs -> soil_lbm.h ----------------
extern "C" {
void smx_lbm_destroy(smx_lbm* l) {
  if (!l) return;
  hipSetDevice(l->device);
  if (l->stream) hipStreamSynchronize(l->stream);
  l->mem.clear();
  if (l->ev0) hipEventDestroy(l->ev0); if (l->ev1) hipEventDestroy(l->ev1);
  if (l->stream) hipStreamDestroy(l->stream);
  delete l;
}
const char* smx_lbm_last_error(smx_lbm* l) { return l ? l->err.c_str() : "null handle"; }
int smx_lbm_create(int32_t nx, int32_t ny, int32_t nz, int32_t device, smx_lbm** out) {
  if (!out) return -2;
  smx_lbm* l = new smx_lbm;
  *out = l;
  if (nx < 2 || ny < 2 || nz < 2) { l->err = "smx_lbm_create: every dimension must be >= 2"; return -2; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { l->err = "no HIP device visible (soilmx has no CPU fallback)"; return -3; }
  l->device = device; l->d.nx = nx; l->d.ny = ny; l->d.nz = nz; l->d.n = (unsigned long long)nx * ny * nz;
  l->k = make_lbm_consts();
  HIPCHK(l, hipSetDevice(device));
  HIPCHK(l, hipStreamCreate(&l->stream));
  HIPCHK(l, hipEventCreate(&l->ev0)); HIPCHK(l, hipEventCreate(&l->ev1));
  const size_t n = (size_t)l->d.n;
  HIPCHK(l, l->mem.dev(l->f[0], n * LQ)); HIPCHK(l, l->mem.dev(l->f[1], n * LQ));
  HIPCHK(l, l->mem.dev(l->B, n)); HIPCHK(l, l->mem.dev(l->rho, n)); HIPCHK(l, l->mem.dev(l->v, n));
  HIPCHK(l, hipMemsetAsync(l->f[0], 0, n * LQ * 4, l->stream)); HIPCHK(l, hipMemsetAsync(l->f[1], 0, n * LQ * 4, l->stream));
  HIPCHK(l, hipMemsetAsync(l->B, 0, n * 4, l->stream)); HIPCHK(l, hipMemsetAsync(l->rho, 0, n * 4, l->stream)); HIPCHK(l, hipMemsetAsync(l->v, 0, n * 16, l->stream));
  HIPCHK(l, hipStreamSynchronize(l->stream));
  return 0;
}
static unsigned lbm_grid(const smx_lbm* l) { const unsigned long long nb = (l->d.n + 255ull) / 256ull; return (unsigned)((nb + 7ull) / 8ull * 8ull); }
int smx_lbm_set_boundary(smx_lbm* l, const float* b) {
  HIPCHK(l, hipSetDevice(l->device));
  HIPCHK(l, hipMemcpyAsync(l->B, b, (size_t)l->d.n * 4, hipMemcpyHostToDevice, l->stream));
  HIPCHK(l, hipStreamSynchronize(l->stream));
  return 0;
}
int smx_lbm_boundary_from_map(smx_lbm* l, smx_ctx* ctx, float sx, float sy, float sz) {
  if (!ctx) { l->err = "smx_lbm_boundary_from_map: no map"; return -2; }
  if (ctx->partial()) { l->err = "smx_lbm_boundary_from_map: the map context holds only a strip"; return -2; }
  if (ctx->cfg.device != l->device) { l->err = "smx_lbm_boundary_from_map: map and lattice live on different devices"; return -2; }
  if ((int)(sx * (float)(l->d.nx - 1)) >= ctx->cfg.dimx || (int)(sz * (float)(l->d.nz - 1)) >= ctx->cfg.dimy || sx < 0.f || sz < 0.f) {
    l->err = "smx_lbm_boundary_from_map: the scaled lattice does not fit the map"; return -2;
  }
  HIPCHK(l, ctx->mem.grow(ctx->d_plane, ctx->plane_cap, ctx->ncells * 8, ctx->ncells * 8));   // (failures are the lattice's: the caller reads smx_lbm_last_error)
  hipLaunchKernelGGL(k_heights, dim3((unsigned)((ctx->ncells + 255) / 256)), dim3(256), 0, ctx->stream, ctx->d, (double*)ctx->d_plane);
  HIPCHK(l, hipStreamSynchronize(ctx->stream));
  hipLaunchKernelGGL(k_lbm_boundary_from_heights, dim3((unsigned)((l->d.n + 255ull) / 256ull)), dim3(256), 0, l->stream, l->d, (const double*)ctx->d_plane,
                     ctx->cfg.dimy, sx, sy, sz, ctx->cfg.scale, l->B);
  HIPCHK(l, hipStreamSynchronize(l->stream));
  return 0;
}
int smx_lbm_initialize(smx_lbm* l) {
  HIPCHK(l, hipSetDevice(l->device));
  l->cur = 0;
  hipLaunchKernelGGL(k_lbm_init, dim3(lbm_grid(l)), dim3(256), 0, l->stream, l->d, l->k, l->B, l->f[0], l->rho, l->v);
  HIPCHK(l, hipGetLastError());
  return 0;
}
int smx_lbm_step(smx_lbm* l, int32_t n) {
  HIPCHK(l, hipSetDevice(l->device));
  if (n <= 0) return 0;
  HIPCHK(l, hipEventRecord(l->ev0, l->stream));
  static const int variant = (env_flag("SMX_LBM_NT") ? 1 : 0) | (env_flag("SMX_LBM_XCD") ? 2 : 0);   // measured switches (profiles/r02_lbm_bench.log); results do not depend on them
  for (int s = 0; s < n; s++) {
    const dim3 g(lbm_grid(l)), t(256);
    float *fa = l->f[l->cur], *fb = l->f[l->cur ^ 1];
    switch (variant) {
      case 0: hipLaunchKernelGGL((k_lbm_step<false, false>), g, t, 0, l->stream, l->d, l->k, l->B, fa, fb, l->rho, l->v); break;
      case 1: hipLaunchKernelGGL((k_lbm_step<true, false>), g, t, 0, l->stream, l->d, l->k, l->B, fa, fb, l->rho, l->v); break;
      case 2: hipLaunchKernelGGL((k_lbm_step<false, true>), g, t, 0, l->stream, l->d, l->k, l->B, fa, fb, l->rho, l->v); break;
      default: hipLaunchKernelGGL((k_lbm_step<true, true>), g, t, 0, l->stream, l->d, l->k, l->B, fa, fb, l->rho, l->v); break;
    }
    l->cur ^= 1;
  }
  HIPCHK(l, hipEventRecord(l->ev1, l->stream));
  HIPCHK(l, hipGetLastError());
  HIPCHK(l, hipEventSynchronize(l->ev1));
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, l->ev0, l->ev1) == hipSuccess) { l->ms_steps += ms; l->steps += (unsigned long long)n; }
  return 0;
}
int smx_lbm_get_timing(smx_lbm* l, double* ms_steps, uint64_t* steps, int32_t reset) {
  if (ms_steps) *ms_steps = l->ms_steps;
  if (steps) *steps = l->steps;
  if (reset) { l->ms_steps = 0.0; l->steps = 0; }
  return 0;
}
int smx_lbm_read(smx_lbm* l, float* rho, float* v4, float* f_aos) {
  HIPCHK(l, hipSetDevice(l->device));
  const size_t n = (size_t)l->d.n;
  if (rho) HIPCHK(l, hipMemcpyAsync(rho, l->rho, n * 4, hipMemcpyDeviceToHost, l->stream));
  if (v4) HIPCHK(l, hipMemcpyAsync(v4, l->v, n * 16, hipMemcpyDeviceToHost, l->stream));
  if (f_aos) {                                                // the spare lattice is scratch between steps (a step writes every slot of it)
    float* tmp = l->f[l->cur ^ 1];
    hipLaunchKernelGGL(k_lbm_to_aos, dim3((unsigned)((n * LQ + 255) / 256)), dim3(256), 0, l->stream, l->d, l->f[l->cur], tmp);
    HIPCHK(l, hipMemcpyAsync(f_aos, tmp, n * LQ * 4, hipMemcpyDeviceToHost, l->stream));
  }
  HIPCHK(l, hipStreamSynchronize(l->stream));
  return 0;
}
int smx_lbm_write_f(smx_lbm* l, const float* f_aos) {
  HIPCHK(l, hipSetDevice(l->device));
  const size_t n = (size_t)l->d.n;
  float* stage = nullptr;
  HIPCHK(l, l->mem.dev(stage, n * LQ));
  hipError_t e = hipMemcpyAsync(stage, f_aos, n * LQ * 4, hipMemcpyHostToDevice, l->stream);
  hipLaunchKernelGGL(k_lbm_from_aos, dim3((unsigned)((n * LQ + 255) / 256)), dim3(256), 0, l->stream, l->d, stage, l->f[l->cur]);
  if (e == hipSuccess) e = hipStreamSynchronize(l->stream);
  l->mem.drop(stage);
  if (e != hipSuccess) { l->err = hipGetErrorString(e); return -1; }
  return 0;
}
int smx_lbm_move(smx_lbm* l, float* pos4, int32_t n) {
  HIPCHK(l, hipSetDevice(l->device));
  if (n <= 0) return 0;
  float4* d = nullptr;
  HIPCHK(l, l->mem.dev(d, (size_t)n));
  hipError_t e = hipMemcpyAsync(d, pos4, (size_t)n * 16, hipMemcpyHostToDevice, l->stream);
  hipLaunchKernelGGL(k_lbm_move, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, l->stream, l->d, l->v, d, n);
  if (e == hipSuccess) e = hipMemcpyAsync(pos4, d, (size_t)n * 16, hipMemcpyDeviceToHost, l->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(l->stream);
  l->mem.drop(d);
  if (e != hipSuccess) { l->err = hipGetErrorString(e); return -1; }
  return 0;
}
}  // extern "C"
