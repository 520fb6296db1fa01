// soil_serial.h -- the exact SERIAL engine: the generator, the access policy (one walker, reference order, direct access), the walkers.
#pragma once
#include "soil_core.h"

namespace smx {

// glibc rand() (stdlib/random_r.c, TYPE_3), THE definition of the generator: the kernels, the library's host driver and the host
// build of tests/hostsim all step it through these. `calls` counts rand() calls, which only the caller knows: none of them touch it
// except rand_seed, which starts the count.
SMX_HD uint32_t rand_step(RandState& r) {       // one raw step; rand() returns it >> 1
  const uint32_t i = r.idx;
  const uint32_t v = r.ring[i % 31] + r.ring[(i - 3) % 31];
  r.ring[i % 31] = v;
  r.idx = i + 1;
  return v;
}
SMX_HD void rand_skip(RandState& r, uint64_t n) { for (uint64_t i = 0; i < n; i++) rand_step(r); }
SMX_HD void rand_seed(RandState& r, uint32_t seed) {   // srandom_r
  if (seed == 0) seed = 1;
  int32_t word = (int32_t)seed;
  r.ring[0] = (uint32_t)word;
  for (int i = 1; i < 31; i++) {
    long hi = word / 127773, lo = word % 127773;
    word = (int32_t)(16807 * lo - 2836 * hi);
    if (word < 0) word += 2147483647;
    r.ring[i] = (uint32_t)word;
  }
  r.idx = 34;
  rand_skip(r, 310);                            // (the warm-up steps are no rand() calls)
  r.calls = 0;
}

struct SerialPolicy {
  static constexpr bool READ_ONLY = false;
  static constexpr bool DEFER_NESTED = false;
  static constexpr bool EXCLUSIVE = true;       // this thread owns every cell it touches while it acts (soil_core.h push_frame)
  unsigned long long live;       // live sections, cached in a register for the kernel's lifetime
  uint32_t nfree;                // entries on the free-node stack
  SMX_D explicit SerialPolicy(const DevState& s) : live(s.ctr[C_LIVE_SECTIONS]), nfree(*s.free_count) {}
  SMX_D void finish(const DevState& s) { s.ctr[C_LIVE_SECTIONS] = live; *s.free_count = nfree; }

  template <int N> struct Pre {};
  SMX_D void save_blk(const Blk&) {}
  SMX_D void load_blk(Blk&) {}
  SMX_D bool touch(const DevState&, size_t, size_t) { return true; }
  template <int N> SMX_D void prefetch(const DevState&, const size_t (&)[N], const size_t (&)[N], Pre<N>&) {}
  template <int N> SMX_D bool acquire_log(const DevState&, const size_t (&)[N], const Pre<N>&, const Sec (&)[N]) { return true; }
  SMX_D void pre_write_node(const DevState&, uint32_t) {}
  // fire-and-forget on the 32-bit word that holds the flag byte (the plane is allocated in whole words): a walker that first
  // LOADS the byte to see whether it must change pays a memory round trip per call
  SMX_D void set_flag(const DevState& s, size_t c, uint8_t f) {
    SMX_OR32_ASYNC(reinterpret_cast<uint32_t*>(s.flags + (c & ~(size_t)3)), (uint32_t)f << (8u * (uint32_t)(c & 3)));
  }
  SMX_D void set_flag_async(const DevState& s, size_t c, uint8_t f) { set_flag(s, c, f); }
  SMX_D void clear_flag(const DevState& s, size_t c, uint8_t f) {
    SMX_AND32_ASYNC(reinterpret_cast<uint32_t*>(s.flags + (c & ~(size_t)3)), ~((uint32_t)f << (8u * (uint32_t)(c & 3))));
  }
  // secpool::get / unget (layermap.h:89-111): get() fails exactly when live sections == capacity
  SMX_D bool can_get(const DevState& s) const { return live < s.pool_capacity; }
  SMX_D void live_add(const DevState&, int d) { live += (long long)d; }
  SMX_D uint32_t node_alloc(const DevState& s) {
    if (nfree == 0) return NIL;
    nfree--;
    return s.freelist[nfree];
  }
  SMX_D void node_free(const DevState& s, uint32_t e) { s.freelist[nfree] = e; nfree++; }
  SMX_D int rand1(const DevState& s) {          // glibc rand()
    RandState& r = *s.rnd;
    const uint32_t v = rand_step(r);
    r.calls++;
    return (int)(v >> 1);
  }
  SMX_D void rand2(const DevState& s, int& first, int& second) { first = rand1(s); second = rand1(s); }
  SMX_D void add_counter(const DevState& s, int which, unsigned long long v) { if (v) s.ctr[which] += v; }
};

// The walkers of the exact engine, one lane in reference order. k_*_serial (soilmx.hip) run them on a context's own DevState, the
// ensemble kernels (k_ens_*) on one member's entry of a device table, one wavefront per member, tests/hostsim on a host thread: one
// definition of the step for all three. `sh`: the soil table (LDS on the device, s.soils on the host).
SMX_D void serial_water_walk(const DevState& s, const SoilP* sh, int n) {
  SerialPolicy pol(s);
  Sim<SerialPolicy> sim(s, sh, pol);
  Frame st[MAX_FRAMES];
  int depth = 0;
  for (int i = 0; i < n; i++) {                            // SoilMachine.cpp:288-298
    int ry, rx;
    pol.rand2(s, ry, rx);                                  // water.h:13, g++ order: 1st draw -> y, 2nd -> x
    Water p;
    sim.water_init(p, rx % s.dimx, ry % s.dimy);
    sim.water_drive(p, true, true, st, depth);
  }
  sim.flush_counters();
  pol.finish(s);
}

SMX_D void serial_wind_walk(const DevState& s, const SoilP* sh, int n) {
  SerialPolicy pol(s);
  Sim<SerialPolicy> sim(s, sh, pol);
  for (int i = 0; i < n; i++) {                            // SoilMachine.cpp:304-307
    int ry, rx;
    pol.rand2(s, ry, rx);                                  // wind.h:15
    Wind p;
    sim.wind_init(p, rx % s.dimx, ry % s.dimy);
    sim.wind_run(p);
  }
  sim.flush_counters();
  pol.finish(s);
}

SMX_D void serial_grid_walk(const DevState& s, const SoilP* sh) {
  SerialPolicy pol(s);
  Sim<SerialPolicy> sim(s, sh, pol);
  sim.grid_mode = true;
  Frame st[MAX_FRAMES];
  int depth = 0;
  const size_t n = (size_t)s.dimx * s.dimy;
  size_t c = sim.next_active(0);
  unsigned long long visited = 0;
  Water dummy;
  dummy.pos = {0.f, 0.f}; dummy.speed = {0.f, 0.f}; dummy.volume = 0.0; dummy.sediment = 0.0; dummy.evaprate = 0.0;
  dummy.spill = 0; dummy.ix = dummy.iy = 0; dummy.friction = 0.f; dummy.surface = dummy.contains = 0;
  while (c < n) {
    const int x = (int)(c / s.dimy), y = (int)(c % s.dimy);
    sim.seep(x, y);                                        // water.h:339
    sim.push_frame(st, depth, x, y, 3);                    // water.h:340 WaterParticle::cascade(ivec2(x,y), .., 3)
    sim.water_drive(dummy, false, false, st, depth);
    visited++;
    c = sim.next_active(c + 1);
  }
  // every non-active cell still "calls" WaterParticle::cascade once in the reference (counter parity)
  sim.n_wcasc += n - visited;
  sim.flush_counters();
  pol.add_counter(s, C_GRID_ACTIVE, visited);
  pol.finish(s);
}

}  // namespace smx
