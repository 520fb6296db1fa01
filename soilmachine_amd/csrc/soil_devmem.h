// soil_devmem.h -- the one owner of a context's device and pinned host memory (host code only).
//
// Most device pointers live inside the POD views the kernels take by value (DevState, SpecShared, BatchShared, ForkDst, EnsEntry),
// so they cannot own anything themselves. A DevMem remembers every block it handed out instead: one per smx_ctx, smx_ensemble,
// smx_lbm and strip transport. Its destructor frees what is still held, so a destroy function lists no buffers and a buffer somebody
// adds cannot be forgotten there. Every operation returns the runtime's hipError_t; what to do with it -- and whether to clear the
// runtime's sticky error -- is the call site's business. hipMalloc / hipHostMalloc / hipFree / hipHostFree are called by name and NOT
// declared here: the including file brings hip_runtime.h (soilmx.hip) or stand-ins that count and fail on demand (tests/devmem_host).
#pragma once
#include <stddef.h>
#include <type_traits>
#include <vector>

struct DevMem {
  struct Block { void* p; bool pinned; };
  std::vector<Block> held;                                    // ~100 entries at most: a linear search
  DevMem() = default; DevMem(const DevMem&) = delete; DevMem& operator=(const DevMem&) = delete;
  ~DevMem() { clear(); }
  void clear() { for (const Block& b : held) release(b); held.clear(); }   // (a destroy function calls it before its stream goes)
  // `count` elements of T (bytes for void*) into p, which the owner remembers; p is null on failure
  template <class T> hipError_t dev(T*& p, size_t count) { return get(p, count, false); }
  template <class T> hipError_t pinned(T*& p, size_t count) { return get(p, count, true); }
  // free one block and null its pointer; a null pointer or one this owner does not hold is left alone
  template <class T> void drop(T*& p) {
    for (size_t i = 0; i < held.size(); i++)
      if (p && held[i].p == (void*)p) { release(held[i]); held[i] = held.back(); held.pop_back(); p = nullptr; return; }
  }
  // room for `need` elements: nothing to do while cap suffices; else the old block goes BEFORE `ncap` elements are asked for (peak
  // memory), and a failed request leaves a null pointer with capacity 0, never a dangling one
  template <class T, class C> hipError_t grow(T*& p, C& cap, size_t need, size_t ncap, bool pin = false) {
    if ((size_t)cap >= need) return hipSuccess;
    drop(p); cap = 0;
    const hipError_t e = get(p, ncap, pin);
    if (e == hipSuccess) cap = (C)ncap;
    return e;
  }

 private:
  static void release(const Block& b) { if (b.pinned) hipHostFree(b.p); else hipFree(b.p); }
  template <class T> hipError_t get(T*& p, size_t count, bool pin) {
    void* q = nullptr;
    const size_t bytes = count * sizeof(std::conditional_t<std::is_void<T>::value, char, T>);
    const hipError_t e = pin ? hipHostMalloc(&q, bytes) : hipMalloc(&q, bytes);
    if (e != hipSuccess) q = nullptr;
    if (q) held.push_back({q, pin});
    p = static_cast<T*>(q);
    return e;
  }
};
