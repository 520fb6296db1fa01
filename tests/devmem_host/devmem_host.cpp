// tests/devmem_host -- soil_devmem.h compiled for the host (TEST INFRASTRUCTURE ONLY). The four HIP allocation calls are stand-ins
// that count live blocks and bytes, log every call in order and fail the k-th allocation on demand; a rig of pointer / capacity
// slots around one DevMem is driven from Python (tests/devmem_host_lib.py, tests/test_devmem_host.py).
#include <stdint.h>
#include <stdlib.h>
#include <map>
#include <vector>

enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2 };

namespace {
enum Op { OP_MALLOC = 0, OP_HOST_MALLOC = 1, OP_FREE = 2, OP_HOST_FREE = 3 };
struct Call { int op; uint64_t id, bytes; int ok; };           // id: serial number of the block (0: none)
struct Live { uint64_t id, bytes; bool pinned; };
std::map<void*, Live> g_live;
std::vector<Call> g_log;
uint64_t g_next_id = 1, g_allocs = 0, g_fail_at = 0, g_wrong_free = 0, g_unknown_free = 0;

hipError_t alloc(void** p, size_t bytes, bool pinned) {
  *p = (void*)(uintptr_t)0xDEAD0000;                           // (a careless caller would keep this on failure)
  g_allocs++;
  if (g_fail_at && g_allocs == g_fail_at) { g_log.push_back({pinned ? OP_HOST_MALLOC : OP_MALLOC, 0, bytes, 0}); return hipErrorOutOfMemory; }
  void* q = malloc(1);                                         // a unique address; nobody touches the memory
  g_live[q] = {g_next_id, bytes, pinned};
  g_log.push_back({pinned ? OP_HOST_MALLOC : OP_MALLOC, g_next_id++, bytes, 1});
  *p = q;
  return hipSuccess;
}
hipError_t release(void* p, bool pinned) {
  if (!p) { g_log.push_back({pinned ? OP_HOST_FREE : OP_FREE, 0, 0, 1}); return hipSuccess; }
  auto it = g_live.find(p);
  if (it == g_live.end()) { g_unknown_free++; return hipSuccess; }
  if (it->second.pinned != pinned) g_wrong_free++;
  g_log.push_back({pinned ? OP_HOST_FREE : OP_FREE, it->second.id, it->second.bytes, 1});
  g_live.erase(it);
  free(p);
  return hipSuccess;
}
}  // namespace
hipError_t hipMalloc(void** p, size_t bytes) { return alloc(p, bytes, false); }
hipError_t hipHostMalloc(void** p, size_t bytes) { return alloc(p, bytes, true); }
hipError_t hipFree(void* p) { return release(p, false); }
hipError_t hipHostFree(void* p) { return release(p, true); }

#include "../../soilmachine_amd/csrc/soil_devmem.h"
struct LakeMember { uint64_t w[4]; };   // a stand-in of soil_lakes.h's, of its size: the scratch only allocates tables of them
#include "../../soilmachine_amd/csrc/soil_scratch.h"
using AnalysisScratch = AnalysisScratchOf<LakeMember>;

// slots 0 .. 7 hold uint32_t* (count = elements of 4 bytes), slots 8 .. 15 hold void* (count = bytes); `a`: the scratch of one terrain
// analysis on the same owner (as_*)
struct Rig {
  uint32_t* w[8] = {}; void* v[8] = {}; uint32_t wcap[8] = {}; size_t vcap[8] = {};
  AnalysisScratch a;
  DevMem* m = new DevMem();   // (declared last and deleted by hand: dm_delete measures what the destructor frees)
};

extern "C" {
void dm_reset() { g_log.clear(); g_allocs = 0; g_fail_at = 0; g_wrong_free = 0; g_unknown_free = 0; }
void dm_fail_at(uint64_t k) { g_fail_at = k ? g_allocs + k : 0; }   // the k-th allocation call from now fails (0: none)
uint64_t dm_live_blocks() { return g_live.size(); }
uint64_t dm_live_bytes() { uint64_t b = 0; for (auto& kv : g_live) b += kv.second.bytes; return b; }
uint64_t dm_wrong_free() { return g_wrong_free; }
uint64_t dm_unknown_free() { return g_unknown_free; }
uint64_t dm_calls() { return g_log.size(); }
uint64_t dm_block_id(uint64_t p) { auto it = g_live.find((void*)(uintptr_t)p); return it == g_live.end() ? 0 : it->second.id; }   // (an address may come again, a serial number does not)
void dm_call(uint64_t i, int* op, uint64_t* id, uint64_t* bytes, int* ok) { const Call& c = g_log[i]; *op = c.op; *id = c.id; *bytes = c.bytes; *ok = c.ok; }

Rig* dm_new() { return new Rig(); }
void dm_delete(Rig* r) { delete r->m; delete r; }
uint64_t dm_held(Rig* r) { return r->m->held.size(); }
int dm_dev(Rig* r, int s, uint64_t count) { return s < 8 ? r->m->dev(r->w[s], count) : r->m->dev(r->v[s - 8], count); }
int dm_pinned(Rig* r, int s, uint64_t count) { return s < 8 ? r->m->pinned(r->w[s], count) : r->m->pinned(r->v[s - 8], count); }
void dm_drop(Rig* r, int s) {   // (with the capacity reset the call sites pair a drop with)
  if (s < 8) { r->m->drop(r->w[s]); r->wcap[s] = 0; } else { r->m->drop(r->v[s - 8]); r->vcap[s - 8] = 0; }
}
int dm_grow(Rig* r, int s, uint64_t need, uint64_t ncap, int pinned) {
  return s < 8 ? r->m->grow(r->w[s], r->wcap[s], need, ncap, pinned != 0) : r->m->grow(r->v[s - 8], r->vcap[s - 8], need, ncap, pinned != 0);
}
uint64_t dm_ptr(Rig* r, int s) { return (uint64_t)(uintptr_t)(s < 8 ? (void*)r->w[s] : r->v[s - 8]); }
uint64_t dm_cap(Rig* r, int s) { return s < 8 ? r->wcap[s] : r->vcap[s - 8]; }
void dm_forget(Rig* r, int s) { if (s < 8) r->w[s] = nullptr; else r->v[s - 8] = nullptr; }   // the slot's pointer only: the owner still holds the block
void dm_poke(Rig* r, int s, uint64_t p) { r->v[s - 8] = (void*)(uintptr_t)p; }                   // a pointer the owner never handed out

// The allocate-new-then-swap idiom of ens_reserve / ens_obs_reserve (soilmx.hip) on a device + pinned pair in slots d and h: the new
// pair goes into locals through the same owner; on failure the locals are dropped and the old pair stays, on success the old pair is
// dropped and the slots take the new one.
int dm_swap_pair(Rig* r, int d, int h, uint64_t count) {
  uint32_t* nd = nullptr; uint32_t* nh = nullptr;
  if (r->m->dev(nd, count) != hipSuccess || r->m->pinned(nh, count) != hipSuccess) { r->m->drop(nd); return -1; }
  r->m->drop(r->w[d]); r->m->drop(r->w[h]);
  r->w[d] = nd; r->w[h] = nh; r->wcap[d] = r->wcap[h] = (uint32_t)count;
  return 0;
}

// AnalysisScratch (soil_scratch.h) on the rig's owner. as_ptr: 0 .. 9 the u32 planes, 10 the f64 plane, 11 temp, 12 / 13 the device /
// pinned tables, 14 / 15 the count words, 16 / 17 the result region. as_cap: 0 words, 1 more_words, 2 temp_bytes, 3 tab_cap, 4 res_cap.
static AnalysisScratch::Need as_need(uint64_t words, int planes, int more, int f64, uint64_t temp_bytes, uint32_t members, uint64_t count_words, uint64_t res_bytes) {
  AnalysisScratch::Need n;
  n.words = words; n.planes = planes; n.more = more; n.f64 = f64 != 0; n.temp_bytes = temp_bytes; n.members = members; n.count_words = count_words; n.res_bytes = res_bytes;
  return n;
}
int as_reserve(Rig* r, uint64_t words, int planes, int more, int f64, uint64_t temp_bytes, uint32_t members, uint64_t count_words, uint64_t res_bytes) {
  return r->a.reserve(*r->m, as_need(words, planes, more, f64, temp_bytes, members, count_words, res_bytes));
}
int as_fits(Rig* r, uint64_t words, int planes, int more, int f64, uint64_t temp_bytes, uint32_t members, uint64_t count_words, uint64_t res_bytes) {
  return r->a.fits(as_need(words, planes, more, f64, temp_bytes, members, count_words, res_bytes)) ? 1 : 0;
}
void as_drop(Rig* r) { r->a.drop(*r->m); }
uint64_t as_ptr(Rig* r, int i) {
  const AnalysisScratch& a = r->a;
  const void* p[18] = {a.plane[0], a.plane[1], a.plane[2], a.plane[3], a.plane[4], a.plane[5], a.plane[6], a.plane[7], a.plane[8], a.plane[9], a.h64, a.temp,
                       a.d_tab, a.h_tab, a.d_cnt, a.h_cnt, a.d_res, a.h_res};
  return (uint64_t)(uintptr_t)p[i];
}
uint64_t as_cap(Rig* r, int i) {
  const uint64_t c[5] = {r->a.words, r->a.more_words, r->a.temp_bytes, r->a.tab_cap, r->a.res_cap};
  return c[i];
}
}
