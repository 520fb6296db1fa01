// soil_scratch.h -- the scratch of one terrain analysis (host code only): the lake census, drainage, the stream network, spill and
// through-drainage each keep ONE AnalysisScratch with their context or ensemble, allocated by the first call, grown on demand, kept.
//
// Five groups, each with its own capacity, so that a call which needs more of one thing replaces that thing alone:
//   planes   `planes` u32 planes of `words` words, and an f64 plane of as many doubles where `f64` is set
//   more     `more` further u32 planes behind them (plane[planes ..]), allocated only once a call asks for them (drainage's P and AR)
//   temp     rocPRIM's temporary storage
//   tables   two member tables (2 * members entries: the members as the call's own kernels see them and, behind them, a second
//            view of the same members), device and pinned; with them `count_words` count words, device and pinned, where asked for
//   result   one region of `res_bytes` bytes, device and pinned: the records, or whatever the call carves from it
// A group that fits is not touched; one that does not loses its old blocks BEFORE the new ones are asked for (peak memory). After a
// failed allocation EVERYTHING is dropped: every pointer is null and every capacity 0, nothing half-sized stays behind. reserve()
// calls no stream function: the CALLER synchronises the stream before a reserve that grows (fits() tells), so that nothing queued
// still uses what is dropped. Depends on DevMem (soil_devmem.h) and hipError_t only; the type of a table entry is the template's
// parameter (soilmx.hip: LakeMember of soil_lakes.h; tests/devmem_host: a stand-in of its size).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "soil_devmem.h"

template <class Member> struct AnalysisScratchOf {
  static constexpr int MAX_PLANES = 10;
  struct Need {
    size_t words = 0; int planes = 0, more = 0; bool f64 = false;
    size_t temp_bytes = 0;
    uint32_t members = 0; size_t count_words = 0;
    size_t res_bytes = 0;
  };
  uint32_t* plane[MAX_PLANES] = {}; double* h64 = nullptr; size_t words = 0, more_words = 0;
  void* temp = nullptr; size_t temp_bytes = 0;
  Member* d_tab = nullptr; Member* h_tab = nullptr; uint32_t* d_cnt = nullptr; uint32_t* h_cnt = nullptr; uint32_t tab_cap = 0;
  char* d_res = nullptr; char* h_res = nullptr; size_t res_cap = 0;
  uint32_t sweeps[2] = {0, 0}, batches = 0;   // of the last call (spill: sweeps[0]; through: the level sweeps and the hop sweeps)

  bool fits(const Need& n) const {
    return n.words <= words && (n.more == 0 || n.words <= more_words) && n.temp_bytes <= temp_bytes && n.members <= tab_cap && n.res_bytes <= res_cap;
  }
  hipError_t reserve(DevMem& mem, const Need& n) {
    hipError_t e = hipSuccess;
    if (n.words > words) {
      for (int i = 0; i < n.planes; i++) mem.drop(plane[i]);
      mem.drop(h64); words = 0;
      for (int i = 0; i < n.planes && e == hipSuccess; i++) e = mem.dev(plane[i], n.words);
      if (e == hipSuccess && n.f64) e = mem.dev(h64, n.words);
      if (e == hipSuccess) words = n.words;
    }
    if (e == hipSuccess && n.more && n.words > more_words) {
      for (int i = n.planes; i < n.planes + n.more; i++) mem.drop(plane[i]);
      more_words = 0;
      for (int i = n.planes; i < n.planes + n.more && e == hipSuccess; i++) e = mem.dev(plane[i], n.words);
      if (e == hipSuccess) more_words = n.words;
    }
    if (e == hipSuccess) e = mem.grow(temp, temp_bytes, n.temp_bytes, n.temp_bytes);
    if (e == hipSuccess && n.members > tab_cap) {
      mem.drop(d_tab); mem.drop(h_tab); mem.drop(d_cnt); mem.drop(h_cnt); tab_cap = 0;
      e = mem.dev(d_tab, 2 * (size_t)n.members);
      if (e == hipSuccess) e = mem.pinned(h_tab, 2 * (size_t)n.members);
      if (e == hipSuccess && n.count_words) e = mem.dev(d_cnt, n.count_words);
      if (e == hipSuccess && n.count_words) e = mem.pinned(h_cnt, n.count_words);
      if (e == hipSuccess) tab_cap = n.members;
    }
    if (e == hipSuccess && n.res_bytes > res_cap) {
      mem.drop(d_res); mem.drop(h_res); res_cap = 0;
      e = mem.dev(d_res, n.res_bytes);
      if (e == hipSuccess) e = mem.pinned(h_res, n.res_bytes);
      if (e == hipSuccess) res_cap = n.res_bytes;
    }
    if (e != hipSuccess) drop(mem);
    return e;
  }
  // the one list of what the scratch holds: whoever adds a buffer adds it here
  void drop(DevMem& mem) {
    for (uint32_t*& q : plane) mem.drop(q);
    mem.drop(h64); mem.drop(temp); mem.drop(d_tab); mem.drop(h_tab); mem.drop(d_cnt); mem.drop(h_cnt); mem.drop(d_res); mem.drop(h_res);
    *this = AnalysisScratchOf();
  }
};
