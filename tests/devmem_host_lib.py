"""ctypes wrapper of tests/devmem_host (soil_devmem.h compiled for the host over counting stand-ins of the four HIP allocation
calls -- TEST INFRASTRUCTURE ONLY)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "devmem_host")
ROOT = os.path.dirname(os.path.dirname(HERE))
LIB = os.path.join(HERE, "libdevmem_host.so")
SRC = [os.path.join(HERE, "devmem_host.cpp"), os.path.join(ROOT, "soilmachine_amd", "csrc", "soil_devmem.h"), os.path.join(ROOT, "soilmachine_amd", "csrc", "soil_scratch.h")]
MALLOC, HOST_MALLOC, FREE, HOST_FREE = range(4)
OOM = 2                       # the stand-ins' hipErrorOutOfMemory
WORDS, BYTES = range(0, 8), range(8, 16)   # slots of uint32_t* (count = 4-byte elements) and of void* (count = bytes)
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB) or any(os.path.getmtime(p) > os.path.getmtime(LIB) for p in SRC):
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-o", LIB, SRC[0]])
        L = C.CDLL(LIB)
        vp, u64, i = C.c_void_p, C.c_uint64, C.c_int
        L.dm_reset.restype = None
        L.dm_fail_at.argtypes = [u64]; L.dm_fail_at.restype = None
        for f in ("dm_live_blocks", "dm_live_bytes", "dm_wrong_free", "dm_unknown_free", "dm_calls"):
            getattr(L, f).restype = u64
        L.dm_call.argtypes = [u64] + [vp] * 4; L.dm_call.restype = None
        L.dm_block_id.argtypes = [u64]; L.dm_block_id.restype = u64
        L.dm_new.restype = vp
        L.dm_delete.argtypes = [vp]; L.dm_delete.restype = None
        L.dm_held.argtypes = [vp]; L.dm_held.restype = u64
        L.dm_dev.argtypes = [vp, i, u64]; L.dm_pinned.argtypes = [vp, i, u64]
        L.dm_drop.argtypes = [vp, i]; L.dm_drop.restype = None
        L.dm_grow.argtypes = [vp, i, u64, u64, i]
        L.dm_ptr.argtypes = [vp, i]; L.dm_ptr.restype = u64
        L.dm_cap.argtypes = [vp, i]; L.dm_cap.restype = u64
        L.dm_forget.argtypes = [vp, i]; L.dm_forget.restype = None
        L.dm_poke.argtypes = [vp, i, u64]; L.dm_poke.restype = None
        L.dm_swap_pair.argtypes = [vp, i, i, u64]
        need = [u64, i, i, i, u64, C.c_uint32, u64, u64]   # words, planes, more, f64, temp_bytes, members, count_words, res_bytes
        L.as_reserve.argtypes = [vp] + need; L.as_fits.argtypes = [vp] + need
        L.as_drop.argtypes = [vp]; L.as_drop.restype = None
        L.as_ptr.argtypes = [vp, i]; L.as_ptr.restype = u64
        L.as_cap.argtypes = [vp, i]; L.as_cap.restype = u64
        _lib = L
    return _lib


def calls(start: int = 0) -> list:
    """The stand-ins' log from entry `start`: (op, block id, bytes, ok) in call order."""
    L = lib()
    out = []
    for k in range(start, L.dm_calls()):
        op, ok = C.c_int(), C.c_int()
        bid, nbytes = C.c_uint64(), C.c_uint64()
        L.dm_call(k, C.byref(op), C.byref(bid), C.byref(nbytes), C.byref(ok))
        out.append((op.value, bid.value, nbytes.value, ok.value))
    return out


class Rig:
    """One DevMem and 16 pointer / capacity slots around it."""

    def __init__(self):
        self.L = lib()
        self.h = self.L.dm_new()

    def delete(self):
        if self.h:
            self.L.dm_delete(self.h)
            self.h = None

    def dev(self, s, count): return self.L.dm_dev(self.h, s, count)
    def pinned(self, s, count): return self.L.dm_pinned(self.h, s, count)
    def drop(self, s): self.L.dm_drop(self.h, s)
    def grow(self, s, need, ncap, pinned=False): return self.L.dm_grow(self.h, s, need, ncap, int(pinned))
    def ptr(self, s): return self.L.dm_ptr(self.h, s)
    def cap(self, s): return self.L.dm_cap(self.h, s)
    def held(self): return self.L.dm_held(self.h)
    def forget(self, s): self.L.dm_forget(self.h, s)
    def poke(self, s, p): self.L.dm_poke(self.h, s, p)
    def swap_pair(self, d, h, count): return self.L.dm_swap_pair(self.h, d, h, count)

    # the AnalysisScratch on this owner (soil_scratch.h); need: (words, planes, more, f64, temp_bytes, members, count_words, res_bytes)
    def as_reserve(self, need): return self.L.as_reserve(self.h, *need)
    def as_fits(self, need): return bool(self.L.as_fits(self.h, *need))
    def as_drop(self): self.L.as_drop(self.h)
    def as_ptrs(self): return [self.L.as_ptr(self.h, k) for k in range(18)]
    def as_blocks(self): return [self.L.dm_block_id(p) for p in self.as_ptrs()]   # the serial numbers of the blocks the pointers name (0: null)
    def as_caps(self): return [self.L.as_cap(self.h, k) for k in range(5)]
