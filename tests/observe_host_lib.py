"""ctypes wrapper of tests/observe_host (soil_observe.h compiled for the host -- TEST INFRASTRUCTURE ONLY)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from soilmachine_amd.snapshot import Snapshot

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "observe_host")
ROOT = os.path.dirname(os.path.dirname(HERE))
LIB = os.path.join(HERE, "libobserve_host.so")
SRC = [os.path.join(HERE, "observe_host.cpp")] + [os.path.join(ROOT, "soilmachine_amd", "csrc", f) for f in ("soil_core.h", "soil_observe.h")]
NIL = 0xFFFFFFFF
PLANES = {"height": 0, "water": 1, "wfreq": 2, "windfreq": 3}
# oh_figures' variants: (tile, staged buried types per cell)
VARIANTS = {0: (256, 8), 1: (256, 1), 2: (64, 0), 3: (96, 3)}
FIELDS = [("sumh", "f"), ("nsec", "u"), ("typehash", "u"), ("wet_cells", "u"), ("water_volume", "f"), ("hmin", "f"), ("hmax", "f"),
          ("empty_cells", "u"), ("rand_calls", "u"), ("live_sections", "u"), ("corrupt", "u")]
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB) or any(os.path.getmtime(p) > os.path.getmtime(LIB) for p in SRC):
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", LIB, SRC[0]])
        L = C.CDLL(LIB)
        vp = C.c_void_p
        L.oh_create.restype = vp
        L.oh_create.argtypes = [C.c_int, C.c_int, C.c_uint64] + [vp] * 7 + [C.c_uint64]
        L.oh_destroy.argtypes = [vp]; L.oh_destroy.restype = None
        L.oh_longest_column.argtypes = [vp]; L.oh_longest_column.restype = C.c_uint32
        L.oh_set_prev.argtypes = [vp, C.c_uint64, C.c_uint32, C.c_uint32]; L.oh_set_prev.restype = None
        L.oh_top_prev.argtypes = [vp, C.c_uint64]; L.oh_top_prev.restype = C.c_uint32
        L.oh_figures.argtypes = [vp, C.c_uint32, C.c_int, vp]
        L.oh_plane_stats.argtypes = [vp, C.c_uint32, C.c_int] + [vp] * 5
        assert L.oh_figures_bytes() == 8 * len(FIELDS)
        for v, (_, k) in VARIANTS.items():
            assert L.oh_staged_types(v) == k
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class HostMember:
    """One member's state on the host, built from a snapshot's columns."""

    def __init__(self, s: Snapshot, pool: int | None = None):
        self.L = lib()
        self.dimx, self.dimy = int(s.dimx), int(s.dimy)
        self.pool = int(pool if pool is not None else max(1, s.nsec))
        arr = [np.ascontiguousarray(a, dt) for a, dt in ((s.count, np.uint32), (s.type, np.uint32), (s.size, np.float64), (s.floor, np.float64),
                                                         (s.sat, np.float64), (s.wfreq, np.float32), (s.windfreq, np.float32))]
        self.h = self.L.oh_create(self.dimx, self.dimy, self.pool, *[_p(a) for a in arr], int(s.rand_calls))
        if not self.h:
            raise RuntimeError("observe_host: the pool is too small for the snapshot's buried sections")

    def __del__(self):
        if getattr(self, "h", None):
            self.L.oh_destroy(self.h); self.h = None

    def longest_column(self) -> int:
        return int(self.L.oh_longest_column(self.h))

    def figures(self, lanes: int = 256, variant: int = 0):
        """(rc, dict): the body of k_ens_figures with `lanes` lanes; typehash formatted as Snapshot.digest() does."""
        raw = np.zeros(len(FIELDS), np.uint64)
        rc = int(self.L.oh_figures(self.h, lanes, variant, _p(raw)))
        out = {}
        for (name, kind), w in zip(FIELDS, raw):
            out[name] = float(np.array([w], np.uint64).view(np.float64)[0]) if kind == "f" else int(w)
        out["typehash"] = f"{out['typehash']:016x}"
        return rc, out


def plane_stats(members, plane: str, var: bool = True):
    """The body of k_ens_plane_stats over `members` in that order -> dict of flat arrays in the plane's own indexing."""
    L = lib()
    n = len(members)
    cells = members[0].dimx * members[0].dimy
    hs = (C.c_void_p * n)(*[m.h for m in members])
    out = {"mean": np.zeros(cells), "var": np.zeros(cells) if var else None, "vmin": np.zeros(cells), "vmax": np.zeros(cells),
           "nonzero": np.zeros(cells, np.uint32)}
    rc = L.oh_plane_stats(hs, n, PLANES[plane], _p(out["mean"]), _p(out["var"]), _p(out["vmin"]), _p(out["vmax"]), _p(out["nonzero"]))
    assert rc == 0, rc
    return {k: v for k, v in out.items() if v is not None}
