"""ctypes wrappers of the host builds of the terrain analyses (tests/<name>_host: the kernels' headers compiled by g++ -- TEST
INFRASTRUCTURE ONLY), and the runner of their stand-alone check programs.

What the eight have in common stands here once, in Analysis: the rule that builds and loads a library, the map handle, the tile
variants and the two calls of a run (a count, then the fetch, then a slice per map). An analysis is a description -- its directory,
its entry point, the files its one translation unit reads, its scalar arguments, its planes -- and a run_many of a few lines that
shapes the result as its tests expect it. One object per analysis: lakes, drainage, streams, spill, through, hillslopes, flowpaths,
dispersal."""
from __future__ import annotations

import ctypes as C
import os
import struct
import subprocess

import numpy as np

from soilmachine_amd import capi
from soilmachine_amd.snapshot import Snapshot

TESTS = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(TESTS), "soilmachine_amd", "csrc")
SHARED = os.path.join(TESTS, "analysis_host", "analysis_host.h")
u32, vp = C.c_uint32, C.c_void_p


class HostMap:
    """The top records of one snapshot's columns on the host, held by the library of `analysis`."""

    def __init__(self, analysis: "Analysis", s: Snapshot):
        self.L, self.destroy = analysis.lib(), analysis.maps + "_destroy"
        self.dimx, self.dimy = int(s.dimx), int(s.dimy)
        arr = [np.ascontiguousarray(a, dt) for a, dt in ((s.count, np.uint32), (s.type, np.uint32), (s.size, np.float64), (s.floor, np.float64))]
        self.h = getattr(self.L, analysis.maps + "_create")(self.dimx, self.dimy, *[capi.ptr(a) for a in arr])

    def __del__(self):
        if getattr(self, "h", None):
            getattr(self.L, self.destroy)(self.h); self.h = None


class Analysis:
    """One host build. entry(maps, nm, variant, lanes, order, *scalars, cap, out, [struct_size,] counts, *planes, *tail)."""
    includes = ()               # the analyses whose <name>_host.cpp this one's includes
    maps = "dh"                 # the prefix of create and destroy
    shapes = ("dh", 3, 3)       # the prefix of variants and variant, the values a variant has, the values variants() returns
    scalars = ()                # the ctypes of the scalar arguments in front of cap
    struct_size = False         # whether the entry takes the size of a record
    tail = ()                   # the ctypes of the arguments behind the planes

    def __init__(self):
        self.HERE = os.path.join(TESTS, self.name + "_host")
        self.PLANES = tuple(self.planes)
        self._lib = None

    def sources(self) -> list:
        """Every file the translation unit reads, <name>_host.cpp first."""
        chain, todo = [], [type(self)]
        while todo:
            a = todo.pop(0)
            chain.append(os.path.join(TESTS, a.name + "_host", a.name + "_host.cpp"))
            todo += a.includes
        return chain + [SHARED] + [os.path.join(CSRC, h) for h in ("soil_core.h", "soil_lakes.h") + self.headers]

    def lib(self):
        if self._lib is None:
            so, src = os.path.join(self.HERE, f"lib{self.name}_host.so"), self.sources()
            if not os.path.exists(so) or any(os.path.getmtime(p) > os.path.getmtime(so) for p in src):
                subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, src[0]])
            L = C.CDLL(so)
            create, destroy = getattr(L, self.maps + "_create"), getattr(L, self.maps + "_destroy")
            create.restype, create.argtypes = vp, [C.c_int, C.c_int, vp, vp, vp, vp]
            destroy.restype, destroy.argtypes = None, [vp]
            getattr(L, self.shapes[0] + "_variant").argtypes = [C.c_int] + [C.POINTER(C.c_int)] * self.shapes[1]
            getattr(L, self.entry).argtypes = [vp, u32, C.c_int, u32, C.c_int, *self.scalars, u32, vp, *([C.c_uint64] if self.struct_size else []), vp,
                                               *[vp] * len(self.PLANES), *self.tail]
            self._lib = L
        return self._lib

    def variants(self) -> dict:
        """variant -> its tile shape: (tile columns, tile rows[, slots of the pass table], slots of the statistics table)"""
        L = self.lib()
        prefix, has, shown = self.shapes
        out = {}
        for v in range(getattr(L, prefix + "_variants")()):
            vals = [C.c_int() for _ in range(has)]
            assert getattr(L, prefix + "_variant")(v, *[C.byref(a) for a in vals]) == 0
            out[v] = tuple(a.value for a in vals[:shown])
        return out

    def HostMap(self, s: Snapshot) -> HostMap:
        return HostMap(self, s)

    def _call(self, maps, variant, lanes, order, scalars, cap, out, counts, planes=None, tail=None):
        hs = (vp * len(maps))(*[m.h for m in maps])
        planes = planes or {}
        return getattr(self.lib(), self.entry)(hs, len(maps), variant, lanes, order, *scalars, cap, out, *([C.sizeof(self.record)] if self.struct_size else []),
                                               capi.ptr(counts), *[capi.ptr(planes.get(k)) for k in self.PLANES], *(tail or [None] * len(self.tail)))

    def batch(self) -> int:
        """G: the sweeps of one batch (SPILL_BATCH) -- spill and through."""
        f = getattr(self.lib(), self.shapes[0] + "_batch")
        f.restype = u32
        return int(f())

    def _rc(self, maps, variant, lanes, order, scalars) -> int:
        """The return code of a counting call (no records, no planes, nothing behind them)."""
        return self._call(maps, variant, lanes, order, scalars, 0, None, np.zeros(max(1, len(maps)), np.uint32))

    def _run(self, maps, variant, lanes, order, scalars, cap, planes, tail, count_tail=None):
        """The kernels' bodies over `maps` in one go (the ensemble path) -> one (records, planes, count) per map; cap None: two calls,
        a count and the fetch, as the Python binding does. planes: the names asked for; tail: the arguments behind the planes, count_tail: those of the counting call where they differ."""
        n = len(maps)
        counts = np.zeros(max(1, n), np.uint32)
        if cap is None:
            assert self._call(maps, variant, lanes, order, scalars, 0, None, counts, None, tail if count_tail is None else count_tail) == 0
            cap = int(counts[:n].max()) if n else 0
        out = (self.record * max(1, n * cap))()
        words = sum(m.dimx * m.dimy for m in maps)
        pl = {k: np.zeros(words, self.planes[k]) for k in planes}
        assert self._call(maps, variant, lanes, order, scalars, cap, out, counts, pl, tail) == 0
        res, at = [], 0
        for i, m in enumerate(maps):
            k = min(cap, int(counts[i]))
            cells = m.dimx * m.dimy
            res.append(([out[i * cap + r].as_dict() for r in range(k)], {p: v[at:at + cells].reshape(m.dimx, m.dimy).copy() for p, v in pl.items()}, int(counts[i])))
            at += cells
        return res


class Lakes(Analysis):
    name, entry, headers, record = "lakes", "lh_census", (), capi.Lake
    maps, shapes = "lh", ("lh", 3, 3)
    planes = {"labels": np.uint32}

    def run_many(self, maps, variant: int = 0, lanes: int = 256, descending: bool = False, cap: int | None = None):
        """One (records, labels, nlakes) per map."""
        return [(recs, pl["labels"], n) for recs, pl, n in self._run(maps, variant, lanes, int(descending), (), cap, self.PLANES, None)]

    def run(self, s: Snapshot, variant: int = 0, lanes: int = 256, descending: bool = False, cap: int | None = None):
        """(records, labels, nlakes) of one snapshot."""
        return self.run_many([self.HostMap(s)], variant, lanes, descending, cap)[0]


class Drainage(Analysis):
    name, entry, headers, record = "drainage", "dh_drainage", ("soil_drain.h",), capi.Basin
    planes = {"receivers": np.uint32, "labels": np.uint32, "area": np.uint32}

    def run_many(self, maps, variant: int = 0, lanes: int = 256, order: int = 0, cap: int | None = None, planes=None):
        """One (records, planes, nbasins) per map. order: bit 0 the workgroups, bit 1 the lanes, last to first."""
        return self._run(maps, variant, lanes, order, (), cap, self.PLANES if planes is None else planes, None)

    def run(self, s: Snapshot, variant: int = 0, lanes: int = 256, order: int = 0, cap: int | None = None, planes=None):
        """(records, planes, nbasins) of one snapshot."""
        return self.run_many([self.HostMap(s)], variant, lanes, order, cap, planes)[0]


class Streams(Analysis):
    name, entry, headers, record = "streams", "sh_streams", ("soil_drain.h", "soil_streams.h"), capi.Stream
    includes, shapes, scalars = (Drainage,), ("dh", 3, 2), (u32,)
    planes = {"order": np.uint32, "segments": np.uint32, "reach": np.uint32, "heads": np.uint32}

    def run_many(self, maps, threshold: int, variant: int = 0, lanes: int = 256, order: int = 0, cap: int | None = None, planes=None):
        """One (records, planes, nstreams) per map. order: bit 0 the workgroups, bit 1 the lanes, last to first."""
        return self._run(maps, variant, lanes, order, (threshold,), cap, self.PLANES if planes is None else planes, None)

    def run(self, s: Snapshot, threshold: int, variant: int = 0, lanes: int = 256, order: int = 0, cap: int | None = None, planes=None):
        """(records, planes, nstreams) of one snapshot."""
        return self.run_many([self.HostMap(s)], threshold, variant, lanes, order, cap, planes)[0]


class Spill(Analysis):
    name, entry, headers, record = "spill", "sh_spill", ("soil_drain.h", "soil_spill.h"), capi.Spill
    includes, shapes, scalars, struct_size, tail = (Drainage,), ("sh", 4, 4), (u32,), True, (C.POINTER(u32), C.POINTER(u32))
    planes = {"filled": np.float64}
    RELAX_BLOCKS = 0xFFFFFFFF              # a lane per cell: no stride (the library's cap, SPILL_RELAX_BLOCKS, is 2048)

    def run_many(self, maps, variant: int = 0, lanes: int = 256, order: int = 0, cap: int | None = None, filled: bool = True, relax_blocks: int = RELAX_BLOCKS):
        """([(records, filled plane or None, nbasins) per map], (sweeps, batches)). order: bit 0 the workgroups, bit 1 the lanes,
        last to first; relax_blocks: the workgroups of a relax sweep at most."""
        sw, ba = u32(), u32()
        res = self._run(maps, variant, lanes, order, (relax_blocks,), cap, self.PLANES if filled else (), [C.byref(sw), C.byref(ba)])
        return [(recs, pl.get("filled"), n) for recs, pl, n in res], (int(sw.value), int(ba.value))

    def run(self, s: Snapshot, variant: int = 0, lanes: int = 256, order: int = 0, cap: int | None = None, filled: bool = True, relax_blocks: int = RELAX_BLOCKS):
        """((records, filled plane, nbasins), (sweeps, batches)) of one snapshot."""
        res, sweeps = self.run_many([self.HostMap(s)], variant, lanes, order, cap, filled, relax_blocks)
        return res[0], sweeps


class Through(Analysis):
    name, entry, headers, record = "through", "th_through", ("soil_drain.h", "soil_spill.h", "soil_through.h"), capi.Through
    includes, shapes, scalars, struct_size, tail = (Drainage,), ("th", 4, 4), (u32,), True, (vp,)
    planes = {"through_area": np.uint32, "outlets": np.uint32}
    RELAX_BLOCKS = Spill.RELAX_BLOCKS

    def run_many(self, maps, variant: int = 0, lanes: int = 256, order: int = 0, cap: int | None = None, planes: bool = True, relax_blocks: int = RELAX_BLOCKS):
        """([(records, planes dict or None, nbasins) per map], (level sweeps, hop sweeps, batches)). order: bit 0 the workgroups,
        bit 1 the lanes, last to first; relax_blocks: the workgroups of a relax sweep, a hop sweep and the exit at most."""
        sw = np.zeros(3, np.uint32)
        res = self._run(maps, variant, lanes, order, (relax_blocks,), cap, self.PLANES if planes else (), [capi.ptr(sw)])
        return [(recs, pl if planes else None, n) for recs, pl, n in res], tuple(int(v) for v in sw)

    def run(self, s: Snapshot, variant: int = 0, lanes: int = 256, order: int = 0, cap: int | None = None, planes: bool = True, relax_blocks: int = RELAX_BLOCKS):
        """((records, planes, nbasins), (level sweeps, hop sweeps, batches)) of one snapshot."""
        res, sweeps = self.run_many([self.HostMap(s)], variant, lanes, order, cap, planes, relax_blocks)
        return res[0], sweeps


class Hillslopes(Analysis):
    name, entry, headers, record = "hillslopes", "hh_hillslopes", ("soil_drain.h", "soil_streams.h", "soil_hills.h"), capi.Hillslope
    includes, scalars, tail = (Streams,), (u32,), (C.POINTER(u32),)
    planes = {"entry": np.uint32, "hillslope": np.uint32, "straight": np.uint32, "diagonal": np.uint32, "hand": np.float64}

    def run_many(self, maps, threshold: int, variant: int = 0, lanes: int = 256, order: int = 0, cap: int | None = None, planes=None):
        """One (records, planes, nsegments, rounds) per map. order: bit 0 the workgroups, bit 1 the lanes, last to first."""
        rounds = u32()
        res = self._run(maps, variant, lanes, order, (threshold,), cap, self.PLANES if planes is None else planes, [C.byref(rounds)], [None])
        return [r + (int(rounds.value),) for r in res]

    def run(self, s, threshold: int, variant: int = 0, lanes: int = 256, order: int = 0, cap: int | None = None, planes=None):
        """(records, planes, nsegments, rounds) of one snapshot."""
        return self.run_many([self.HostMap(s)], threshold, variant, lanes, order, cap, planes)[0]


class Flowpaths(Analysis):
    name, entry, record = "flowpaths", "fh_flowpaths", capi.Flowpath
    headers = ("soil_drain.h", "soil_streams.h", "soil_hills.h", "soil_paths.h")
    includes, tail = (Drainage,), (vp, u32, vp, C.POINTER(u32))
    planes = {"terminal": np.uint32, "straight": np.uint32, "diagonal": np.uint32, "drop": np.float64, "upstream": np.uint32, "source": np.uint32, "stem": np.uint32}

    def run_many(self, maps, variant: int = 0, lanes: int = 256, order: int = 0, cap: int | None = None, planes=None, profile_cap: int | None = None):
        """One (records, planes, profile, nbasins, nprofile, rounds) per map. order: bit 0 the workgroups, bit 1 the lanes, last to
        first; bits 2 and 3 flip those two for the up-walk alone. profile_cap (one map only): None = no profile."""
        nps = np.zeros(max(1, len(maps)), np.uint32)
        rounds = u32()
        prof = np.full(max(1, profile_cap or 0), 0xFFFFFFFF, np.uint32)
        res = self._run(maps, variant, lanes, order, (), cap, self.PLANES if planes is None else planes,
                        [capi.ptr(prof) if profile_cap else None, profile_cap or 0, capi.ptr(nps), C.byref(rounds)], [None, 0, capi.ptr(nps), None])
        return [(recs, pl, prof[:min(profile_cap, int(nps[i]))].copy() if profile_cap is not None else None, n, int(nps[i]), int(rounds.value))
                for i, (recs, pl, n) in enumerate(res)]

    def run(self, s, variant: int = 0, lanes: int = 256, order: int = 0, cap: int | None = None, planes=None, profile_cap: int | None = -1):
        """(records, planes, profile, nbasins, nprofile, rounds) of one snapshot; profile_cap -1: room for every cell."""
        m = self.HostMap(s)
        return self.run_many([m], variant, lanes, order, cap, planes, m.dimx * m.dimy if profile_cap == -1 else profile_cap)[0]


class Dispersal(Analysis):
    name, entry, headers, record = "dispersal", "dph_dispersal", ("soil_drain.h", "soil_disp.h"), capi.Dispersal
    includes, scalars, tail = (Drainage,), (u32, u32), (C.POINTER(u32),)
    planes = {"area": np.uint64, "donors": np.uint32, "receivers": np.uint32}
    FLOW_BLOCKS = 1024                     # DISP_FLOW_BLOCKS of soil_disp.h

    def rc(self, maps, exponent: int, variant: int = 0, lanes: int = 256, order: int = 0, flow_blocks: int = FLOW_BLOCKS) -> int:
        """The return code of a counting call (no records, no planes)."""
        return self._rc(maps, variant, lanes, order, (flow_blocks, exponent))

    def run_many(self, maps, exponent: int = 1, variant: int = 0, lanes: int = 256, order: int = 0, flow_blocks: int = FLOW_BLOCKS, cap: int | None = None, planes=None):
        """One (records, planes, nbasins, rounds) per map. order: bit 0 the workgroups, bit 1 the lanes, last to first; bits 2 and 3
        flip those two for the flow launches alone."""
        rounds = u32()
        res = self._run(maps, variant, lanes, order, (flow_blocks, exponent), cap, self.PLANES if planes is None else planes, [C.byref(rounds)], [None])
        return [r + (int(rounds.value),) for r in res]

    def run(self, s, exponent: int = 1, variant: int = 0, lanes: int = 256, order: int = 0, flow_blocks: int = FLOW_BLOCKS, cap: int | None = None, planes=None):
        """(records, planes, nbasins, rounds) of one snapshot."""
        return self.run_many([self.HostMap(s)], exponent, variant, lanes, order, flow_blocks, cap, planes)[0]


lakes, drainage, streams, spill, through = Lakes(), Drainage(), Streams(), Spill(), Through()
hillslopes, flowpaths, dispersal = Hillslopes(), Flowpaths(), Dispersal()
ANALYSES = (lakes, drainage, streams, spill, through, hillslopes, flowpaths, dispersal)


# ---- the stand-alone check programs (tests/<name>_host/<name>_check.cpp): programs of their own with the address and
# undefined-behaviour sanitizers linked in, run as child processes -- nothing sanitized is loaded into this interpreter

def build_check(tmp_path, H: Analysis) -> str:
    """H's check program, built by the line in its first comment."""
    exe = str(tmp_path / f"{H.name}_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(H.HERE, f"{H.name}_check.cpp")])
    return exe


def run_check(exe: str, args=()) -> str:
    """The program's output; it has to end well and report no failure."""
    r = subprocess.run([exe, *args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "FAIL" not in r.stdout, r.stdout
    return r.stdout


def write_columns(f, magic: int, s: Snapshot) -> None:
    """The head of a dump: the magic word, the dimensions, the number of sections and the columns as the snapshot holds them."""
    f.write(struct.pack("<Iiii", magic, int(s.dimx), int(s.dimy), int(s.type.size)))
    for a, dt in ((s.count, "<u4"), (s.type, "<u4"), (s.size, "<f8"), (s.floor, "<f8")):
        f.write(np.ascontiguousarray(a, dt).tobytes())
