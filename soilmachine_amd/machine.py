"""Host-side mirror of the reference's interface for the particle-transport hot path.

``Layermap`` mirrors the surface of ``class Layermap`` (source/layermap.h:127-228) that the tick driver
and the particles use, ``SoilMachine`` mirrors the tick loop of SoilMachine.cpp:283-329 with rendering
removed. All compute is in the HIP library behind include/soilmx.h; nothing here falls back to the CPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .snapshot import Snapshot
from .soilfile import SoilConfig, soils_array, layers_array


class SoilmxError(RuntimeError):
    pass


POOLSIZE = 10_000_000      # SoilMachine.cpp:16


def default_pool(dimx: int, dimy: int) -> int:
    """The reference's POOLSIZE (10 M sections, SoilMachine.cpp:16). Deviation, stated: maps of 2048^2 cells and
    more do not fit it (the reference silently drops terrain there), so large maps get
    4 sections per cell instead."""
    return max(POOLSIZE, 4 * int(dimx) * int(dimy))


class Layermap:
    """Device-resident layermap (cells + section pool + frequency planes) behind the C-ABI."""

    def __init__(self, cfg: SoilConfig, dimx: int | None = None, dimy: int | None = None, *, seed: int = 0,
                 pool: int | None = None, device: int = 0, engine: int = capi.ENGINE_SERIAL, initialize: bool = True,
                 x_range: tuple | None = None):
        self.L = capi.load()
        self.cfg = cfg
        self.dimx = int(dimx if dimx is not None else cfg.SIZEX)
        self.dimy = int(dimy if dimy is not None else cfg.SIZEY)
        self.seed = seed
        self.pool = int(pool if pool is not None else default_pool(self.dimx, self.dimy))
        c = capi.Config(self.dimx, self.dimy, cfg.SCALE, device, self.pool, engine, 0)
        self.x_range = x_range                                    # (lo, hi): a STRIP context holding only these columns (smx_create_strip)
        self.h = None
        self.h = self._open(c)
        self._soils = soils_array(cfg)
        self._chk(self.L.smx_set_soils(self.h, capi.ptr(self._soils), len(self._soils)))
        self._chk(self.L.smx_srand(self.h, seed))                 # srand(SEED) SoilMachine.cpp:41
        if initialize:
            self.initialize(seed)

    # -- plumbing --
    def _open(self, c: capi.Config):
        """Create the device context (smx_create / smx_create_strip); raises SoilmxError with the library's text."""
        h = C.c_void_p()
        x_range = self.x_range
        rc = self.L.smx_create(C.byref(c), C.byref(h)) if x_range is None else self.L.smx_create_strip(C.byref(c), int(x_range[0]), int(x_range[1]), C.byref(h))
        if rc != 0:
            msg = self.L.smx_last_error(h).decode() if h else "smx_create failed"
            if h:
                self.L.smx_destroy(h)
            raise SoilmxError(f"smx_create: {msg} (rc={rc})")
        return h

    def _chk(self, rc: int):
        if rc != 0:
            raise SoilmxError(self.L.smx_last_error(self.h).decode() + f" (rc={rc})")

    def close(self):
        if getattr(self, "h", None):
            self.L.smx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- Layermap API --
    def initialize(self, seed: int | None = None):
        """Layermap::initialize (layermap.h:163-216) on the device."""
        lay = layers_array(self.cfg)
        self._chk(self.L.smx_initialize(self.h, self.seed if seed is None else seed, capi.ptr(lay), len(lay)))

    def load(self, s: Snapshot, rand_seed: int | None = None):
        """Import columns / frequency planes; re-seed and fast-forward the rand stream to s.rand_calls."""
        self._chk(self.L.smx_import_columns(self.h, capi.ptr(s.count), capi.ptr(s.type), capi.ptr(s.size),
                                            capi.ptr(s.floor), capi.ptr(s.sat)))
        self._chk(self.L.smx_import_frequency(self.h, capi.ptr(s.wfreq), capi.ptr(s.wtrack), capi.ptr(s.windfreq)))
        if rand_seed is not None:
            self._chk(self.L.smx_srand(self.h, rand_seed))
            self._chk(self.L.smx_rand_advance(self.h, s.rand_calls))

    def snapshot(self) -> Snapshot:
        ns = C.c_uint64()
        self._chk(self.L.smx_num_sections(self.h, C.byref(ns)))
        nc, ns = self.dimx * self.dimy, int(ns.value)
        count = np.zeros(nc, np.uint32); ty = np.zeros(ns, np.uint32)
        size = np.zeros(ns); floor = np.zeros(ns); sat = np.zeros(ns)
        self._chk(self.L.smx_export_columns(self.h, capi.ptr(count), capi.ptr(ty), capi.ptr(size), capi.ptr(floor), capi.ptr(sat)))
        wf, wt, wi = self.frequency()
        c = self.counters()
        return Snapshot(self.dimx, self.dimy, self.cfg.SCALE, len(self.cfg.soils), c["rand_calls"], c["pool_free"],
                        count, ty, size, floor, sat, wf, wt, wi)

    def heights(self) -> np.ndarray:
        out = np.zeros(self.dimx * self.dimy)
        self._chk(self.L.smx_read_heights(self.h, capi.ptr(out)))
        return out

    def frequency(self):
        """The water frequency, water track and wind frequency maps (f32 per cell, index y*dimx+x)."""
        nc = self.dimx * self.dimy
        wf, wt, wi = (np.zeros(nc, np.float32) for _ in range(3))
        self._chk(self.L.smx_read_frequency(self.h, capi.ptr(wf), capi.ptr(wt), capi.ptr(wi)))
        return wf, wt, wi

    def surface(self) -> np.ndarray:
        out = np.zeros(self.dimx * self.dimy, np.uint32)
        self._chk(self.L.smx_read_surface(self.h, capi.ptr(out)))
        return out

    def normals(self) -> np.ndarray:
        out = np.zeros((self.dimx * self.dimy, 3), np.float32)
        self._chk(self.L.smx_normals(self.h, capi.ptr(out)))
        return out

    def vertices(self, colors: np.ndarray, cut=None, mode: str = "update") -> np.ndarray:
        """Layermap::update(Vertexpool&) (layermap.h:475-555) for the whole map in one device pass: (cells, 11) float32 =
        position[3], normal[3], color[4], index (the reference's 44-byte Vertex); `colors` = (nsoils, 4) RGBA."""
        colors = np.ascontiguousarray(colors, np.float32).reshape(-1, 4)
        out = np.zeros((self.dimx * self.dimy, 11), np.float32)
        if cut is None:
            self._chk(self.L.smx_fill_vertices(self.h, capi.ptr(colors), colors.shape[0], capi.ptr(out)))
        else:   # mode "update": the global SLICE of Layermap::update (layermap.h:477-510); "slice": Layermap::slice(s) (:557-613)
            self._chk(self.L.smx_fill_vertices_cut(self.h, capi.ptr(colors), colors.shape[0], 0 if mode == "update" else 1, float(cut), capi.ptr(out)))
        return out

    def vertex(self, x: int, y: int, colors: np.ndarray, cut=None, mode: str = "update") -> np.ndarray:
        """ONE column's vertex under the same rules: Layermap::update(ivec2, Vertexpool&) (layermap.h:475-549) -> (11,) float32."""
        colors = np.ascontiguousarray(colors, np.float32).reshape(-1, 4)
        out = np.zeros(11, np.float32)
        m = -1 if cut is None else (0 if mode == "update" else 1)
        self._chk(self.L.smx_fill_vertex_cut(self.h, capi.ptr(colors), colors.shape[0], m, float(cut or 0.0), int(x), int(y), capi.ptr(out)))
        return out

    def heights_bilinear(self, pos: np.ndarray) -> np.ndarray:
        """Layermap::height(vec2) at the (n, 2) float32 positions: the four cells around each are read, so every position must lie in
        [0, dimx - 1) x [0, dimy - 1) -- a map one cell wide has none; anything else raises SoilmxError and reads nothing."""
        pos = np.ascontiguousarray(pos, np.float32)
        out = np.zeros(pos.shape[0])
        self._chk(self.L.smx_heights_bilinear(self.h, capi.ptr(pos), pos.shape[0], capi.ptr(out)))
        return out

    def add(self, x: int, y: int, size: float, type_: int):
        self._chk(self.L.smx_add(self.h, x, y, size, type_))

    def remove(self, x: int, y: int, h: float) -> float:
        r = C.c_double()
        self._chk(self.L.smx_remove(self.h, x, y, h, C.byref(r)))
        return r.value

    def save(self, path: str):
        """Checkpoint on disk (columns, frequency planes, rand() generator state): smx_save."""
        self._chk(self.L.smx_save(self.h, path.encode()))

    def restore(self, path: str):
        """Resume from a checkpoint written by save() (or a bare snapshot: then the rand stream must be re-seeded)."""
        rc = self.L.smx_load(self.h, path.encode())
        if rc not in (0, 1):
            self._chk(rc)
        return rc == 0

    def copy_from(self, src: "Layermap"):
        """Take over `src`'s whole state on the device (smx_copy_state): columns, frequency planes, rand() generator, SCALE, soil
        table, flag plane and live-section count -- what save() on `src` and restore() here would leave, without the host. Equal
        dims, the same device; this map's pool size, engine and other counters stay."""
        rc = self.L.smx_copy_state(self.h, src.h)
        if rc != 0:
            self._chk(rc)
        self.cfg = src.cfg
        self._soils = src._soils

    def digest(self) -> dict:
        """The Appendix-E state digest (sum of heights, section count, type hash) + rand() draws consumed."""
        sh, ns, th = C.c_double(), C.c_uint64(), C.c_uint64()
        self._chk(self.L.smx_digest(self.h, C.byref(sh), C.byref(ns), C.byref(th)))
        return {"sumh": sh.value, "nsec": int(ns.value), "typehash": f"{th.value:016x}",
                "rand_calls": self.counters()["rand_calls"]}

    def _analysis(self, call, rec, cap, planes, dtype=np.uint32, count=None):
        """What the terrain analyses share: the count call where ``cap`` is None (``count``, or ``call`` with no records and
        no planes), the array sized by it, the fetch, the dicts -- and the (dimx, dimy) planes asked for, ``planes`` listing
        (name, wanted) in the order of the plane arguments of ``call(out, cap, byref(n), *plane_pointers)``. ``dtype``: of every
        plane, or a dict name -> dtype for the planes that are not uint32."""
        n = C.c_uint32()
        if cap is None:
            self._chk(count(C.byref(n)) if count else call(None, 0, C.byref(n), *[None] * len(planes)))
            cap = int(n.value)
        cap = int(cap)
        out = (rec * max(1, cap))()
        each = dtype if isinstance(dtype, dict) else {k: dtype for k, _ in planes}
        got = {k: np.zeros(self.dimx * self.dimy, each.get(k, np.uint32)) for k, want in planes if want}
        self._chk(call(out, cap, C.byref(n), *[capi.ptr(got.get(k)) for k, _ in planes]))
        return [out[k].as_dict() for k in range(min(cap, int(n.value)))], {k: v.reshape(self.dimx, self.dimy) for k, v in got.items()}

    def _basin_count(self, n):
        """``spill`` and ``through`` take their count from the drainage call: record k is basin k of ``drainage()``."""
        return self.L.smx_drainage(self.h, None, C.sizeof(capi.Basin), 0, n, None, None, None)

    def lakes(self, labels: bool = False, cap: int | None = None):
        """The lake census (``smx_lakes``): one dict per lake in rank order -- ``first_cell`` (the lake's smallest cell index
        x*dimy+y, its identity), ``cells``, ``volume_q40`` (the exact integer sum of floor(size * 2^40)) and ``volume`` (that as a
        float), ``level_min`` / ``level_max`` (extremes of the water level floor + size), ``depth_max``, the inclusive box ``x0, y0,
        x1, y1`` and ``flags`` (1: touches the map border, 2: the volume is unreliable). A lake is a maximal set of wet cells -- top
        section Air -- connected through the eight neighbours. ``labels``: also the (dimx, dimy) uint32 plane of ranks, 0xFFFFFFFF
        for a dry cell. ``cap`` None: two calls, a count and the fetch; else at most ``cap`` lakes. Sees every tick queued before
        it and changes nothing."""
        recs, planes = self._analysis(lambda out, cap, n, lab: self.L.smx_lakes(self.h, out, C.sizeof(capi.Lake), cap, n, lab), capi.Lake, cap, [("labels", labels)])
        return (recs, planes["labels"]) if labels else recs

    def drainage(self, receivers: bool = False, labels: bool = False, area: bool = False, cap: int | None = None):
        """Where the water goes (``smx_drainage``): one dict per basin in rank order -- ``first_cell`` (the sink's cell index
        x*dimy+y or the lake's ``first_cell``: join on it with ``lakes()``), ``cells``, ``wet_cells`` (0 for a sink's basin),
        ``flags`` (1: the terminal is a lake, 2: the sink lies on, or the lake touches, the map border), ``height_min`` /
        ``height_max`` and the inclusive box ``x0, y0, x1, y1``. A dry cell drains to the lowest of its eight neighbours that is lower
        than itself (ties: the smaller cell index); a path ends at a sink or at the first wet cell. With a plane asked for the result
        is ``(records, planes)``, ``planes`` a dict of (dimx, dimy) uint32 arrays: ``receivers`` (the receiver's cell index,
        0xFFFFFFFF for a sink and a wet cell), ``labels`` (the basin's rank) and ``area`` (1 + the areas of the cells draining into
        the cell). ``cap`` None: two calls, a count and the fetch; else at most ``cap`` basins. Sees every tick queued before it and
        changes nothing."""
        recs, planes = self._analysis(lambda out, cap, n, *pl: self.L.smx_drainage(self.h, out, C.sizeof(capi.Basin), cap, n, *pl), capi.Basin, cap,
                                      [("receivers", receivers), ("labels", labels), ("area", area)])
        return (recs, planes) if planes else recs

    def streams(self, threshold: int, order: bool = False, segments: bool = False, reach: bool = False, heads: bool = False, cap: int | None = None):
        """The channel network (``smx_streams``): one dict per segment in rank order (ascending ``first_cell``) -- ``first_cell``,
        ``last_cell``, ``cells``, ``order`` (Strahler), ``down`` (``first_cell`` of the segment it joins, 0xFFFFFFFF where it ends
        in a lake or at a sink), ``basin`` (join on it with ``drainage()`` / ``lakes()``), ``flags`` (1: enters a lake, 2: ends at
        a sink, 4: starts at a head, 8: ``last_cell`` on the map border), ``heads`` (Shreve magnitude), ``straight`` / ``diagonal``
        (length = straight + diagonal * sqrt(2)), ``area_first`` / ``area_last``, ``height_first`` / ``height_last``. A channel cell
        is a dry cell with a contributing area of at least ``threshold`` (>= 1); a segment runs from a head or a confluence down to
        the next confluence, a lake or a sink. With a plane asked for the result is ``(records, planes)``, ``planes`` a dict of
        (dimx, dimy) uint32 arrays: ``order``, ``reach`` (cells on the longest channel path down to the cell) and ``heads`` (0 off
        the channels) and ``segments`` (the segment's rank, 0xFFFFFFFF off the channels). ``cap`` None: two calls, a count and the
        fetch; else at most ``cap`` segments. Sees every tick queued before it and changes nothing."""
        threshold = int(threshold)
        recs, planes = self._analysis(lambda out, cap, n, *pl: self.L.smx_streams(self.h, threshold, out, C.sizeof(capi.Stream), cap, n, *pl), capi.Stream, cap,
                                      [("order", order), ("segments", segments), ("reach", reach), ("heads", heads)])
        return (recs, planes) if planes else recs

    def spill(self, filled: bool = False, cap: int | None = None):
        """Where the basins overflow (``smx_spill``): one dict per basin in rank order, record k for basin k of ``drainage()`` --
        ``first_cell``, ``pour_cell`` / ``pour_to`` (the pour point: the basin's lowest pass, a cell of the basin and its neighbour in
        another basin, 0xFFFFFFFF: off the map), ``to_basin`` (``first_cell`` of the basin it pours into, 0xFFFFFFFF off the map),
        ``flags`` (1: the terminal is a lake, 2: pours off the map, 4: nested in a larger depression -- the fill level is above the
        pour height --, 8 / 16: ``storage_q40`` / ``fill_storage_q40`` unreliable), ``cells_below``, ``pour_height``, ``fill_height``
        (how high water must rise before it leaves the map), ``storage_q40`` / ``fill_storage_q40`` (the exact integer sums of
        floor((level - h) * 2^40) over the basin's cells below the pour height / the fill level) and ``storage`` / ``fill_storage``
        (those as floats). ``filled``: the result is ``(records, plane)``, the (dimx, dimy) float64 plane max(h, fill level of the
        cell's basin). ``cap`` None: two calls, a count and the fetch; else at most ``cap`` basins. Sees every tick queued before it
        and changes nothing; the number of relax sweeps depends on the map (``spill_sweeps()``)."""
        recs, planes = self._analysis(lambda out, cap, n, pl: self.L.smx_spill(self.h, out, C.sizeof(capi.Spill), cap, n, pl), capi.Spill, cap, [("filled", filled)],
                                      dtype=np.float64, count=self._basin_count)
        return (recs, planes["filled"]) if filled else recs

    def spill_sweeps(self) -> tuple:
        """(sweeps launched, batches) of the last ``spill()`` (``smx_get_spill_sweeps``)."""
        a, b = C.c_uint32(), C.c_uint32()
        self._chk(self.L.smx_get_spill_sweeps(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def through(self, area: bool = False, outlets: bool = False, cap: int | None = None):
        """Where the water goes once the pits and lakes are full (``smx_through``): one dict per basin in rank order, record k for basin
        k of ``drainage()`` and ``spill()`` -- ``first_cell``, ``exit_cell`` / ``exit_to`` (the exit: the tight pass with the smallest
        (c, n) among those that shorten the way off the map; 0xFFFFFFFF: off the map), ``down`` (``first_cell`` of the basin it exits
        into, 0xFFFFFFFF off the map: the basins form a forest), ``outlet`` / ``outlet_cell`` (``first_cell`` of the root below the
        basin and that root's exit cell), ``hops`` (exits on the way off the map, 1 for a root), ``flags`` (1: the terminal is a lake,
        2: exits off the map, 4: the exit is not ``spill()``'s pour point, 8: ``exit_to`` is a wet cell), ``cells``, ``through_cells``
        (the cells of the basin and of every basin above it), ``upstream_basins``, ``exit_height``, ``fill_height``. ``area`` /
        ``outlets``: the result is ``(records, planes)``, the (dimx, dimy) uint32 planes ``through_area`` (the contributing area
        routed through the overflows) and ``outlets`` (the rank of the root the cell's basin leaves through). ``cap`` None: two calls,
        a count and the fetch; else at most ``cap`` basins. Sees every tick queued before it and changes nothing; the number of
        sweeps depends on the map (``through_sweeps()``)."""
        recs, planes = self._analysis(lambda out, cap, n, *pl: self.L.smx_through(self.h, out, C.sizeof(capi.Through), cap, n, *pl), capi.Through, cap,
                                      [("through_area", area), ("outlets", outlets)], count=self._basin_count)
        return (recs, planes) if planes else recs

    def through_sweeps(self) -> tuple:
        """(level sweeps, hop sweeps, batches) of the last ``through()`` (``smx_get_through_sweeps``)."""
        a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._chk(self.L.smx_get_through_sweeps(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def flowpaths(self, cap: int | None = None, terminal: bool = False, straight: bool = False, diagonal: bool = False, drop: bool = False,
                  upstream: bool = False, source: bool = False, stem: bool = False, profiles: bool = False):
        """The flow paths (``smx_flowpaths``): one dict per basin, record k for basin k of ``drainage()`` -- ``first_cell`` and
        ``cells`` (the basin), ``source_cell`` / ``terminal_cell`` (the two ends of the main stem, the basin's longest flow path, of
        equally long ones the one from the smallest cell), ``steps_max`` / ``diagonal`` (its steps and how many are diagonal) and
        ``length`` (straight + diagonal * sqrt(2)), ``profile_at`` (where the stem starts in the profile), ``flags`` (1: the stem
        ends in a wet cell), ``straight_sum`` / ``diagonal_sum`` (exact sums of the steps to the terminal over the basin's cells),
        ``drop_source`` and ``drop_max``. A dry cell's terminal is the sink or the first wet cell on its way down, a wet cell its
        own; ``drop`` is the cell's height above its terminal. With a plane asked for the result is ``(records, planes)``,
        ``planes`` a dict of (dimx, dimy) arrays: ``terminal`` (a cell index), ``straight`` / ``diagonal`` (steps to the terminal),
        ``upstream`` (the steps of the longest path that arrives at the cell), ``source`` (where that path starts), ``stem`` (the
        position on the basin's main stem counted from its source, 0xFFFFFFFF off the stems), all uint32, and ``drop`` (float64).
        ``profiles``: every record also gets ``profile``, the cells of its stem from source to terminal -- a slice of one list, the
        long profile being the heights along it; the stems of ALL basins are found whatever ``cap`` is. ``cap`` None: two calls, a
        count and the fetch; else at most ``cap`` basins. Sees every tick queued before it and changes nothing."""
        prof = np.zeros(self.dimx * self.dimy if profiles else 1, np.uint32)
        pcap, nprof = (prof.size if profiles else 0), C.c_uint32()
        recs, planes = self._analysis(lambda out, cap, n, *pl: self.L.smx_flowpaths(self.h, out, C.sizeof(capi.Flowpath), cap, n, *pl,
                                                                                     capi.ptr(prof) if out is not None and profiles else None,
                                                                                     pcap if out is not None else 0, C.byref(nprof)),
                                      capi.Flowpath, cap, [("terminal", terminal), ("straight", straight), ("diagonal", diagonal), ("drop", drop), ("upstream", upstream),
                                                           ("source", source), ("stem", stem)], dtype={"drop": np.float64})
        if profiles:
            for r in recs:
                r["profile"] = prof[r["profile_at"]:r["profile_at"] + r["steps_max"] + 1].copy()
        return (recs, planes) if planes else recs

    def catchments(self, cells, gauge: bool = False, straight: bool = False, diagonal: bool = False, drop: bool = False, bins: int = 0,
                   bin_height: float | None = None):
        """Which land drains through the listed cells (``smx_catchments``). ``cells``: a sequence of distinct flat indices x*dimy + y
        or of ``(x, y)`` pairs -- gauges, dam sites, outlets; any cell may be one. One dict per listed cell, in list order --
        ``cell``, ``cells`` (the OWN catchment: the cells whose way down meets this gauge before any other gauge, sink or wet cell,
        the gauge cell included), ``area`` (``cells`` summed over the gauge and every gauge above it: the whole catchment, for a dry
        gauge the ``area`` plane of ``drainage()`` at the cell), ``downstream`` (the list position of the next gauge down the flow,
        0xFFFFFFFF without one), ``basin`` (the rank in ``drainage()``), ``steps_max`` / ``farthest_cell`` (the longest way to the
        gauge inside the own catchment and the cell it starts at), ``straight_sum`` / ``diagonal_sum``, ``drop_max``,
        ``drop_sum_q40`` (the exact integer sum of floor(drop * 2^40)) and ``drop_sum`` (that as a float) and ``flags`` (1:
        ``drop_sum_q40`` unreliable, 2: the gauge cell is wet, 4: it is a sink). ``bins`` (1 to 64) with ``bin_height``: every dict
        also gets ``hist``, the hypsometry of the own catchment -- ``hist[b]`` counts its cells with
        ``b * bin_height <= drop < (b + 1) * bin_height``, the last bin everything above. With a plane asked for the result is
        ``(records, planes)``, ``planes`` a dict of (dimx, dimy) arrays for EVERY cell: ``gauge`` (the list position of the cell's
        entry, 0xFFFFFFFF where its water meets no gauge), ``straight`` / ``diagonal`` (the steps to the entry), uint32, and ``drop``
        (float64, the height above the entry). One call, no count; sees every tick queued before it and changes nothing.

        The catchments of chosen stream segments, delineated at their outlets::

            segs = [s for s in m.streams(256) if s["order"] >= 3]
            recs, planes = m.catchments([s["last_cell"] for s in segs], gauge=True)
            own = planes["gauge"] == 0                  # the own catchment of segs[0]'s outlet

        A gauge's WHOLE catchment is its own plus those of the gauges that have it as ``downstream``, and theirs in turn::

            def whole(i):
                mask = planes["gauge"] == i
                for j, r in enumerate(recs):
                    if r["downstream"] == i:
                        mask |= whole(j)
                return mask                             # mask.sum() == recs[i]["area"]
        """
        cl = np.asarray(cells if isinstance(cells, np.ndarray) else list(cells), np.int64)
        if cl.ndim == 2 and cl.shape[1] == 2:
            cl = cl[:, 0] * self.dimy + cl[:, 1]
        cl = np.ascontiguousarray(cl.reshape(-1), np.uint32)
        n, bins = len(cl), int(bins)
        out = (capi.Catchment * max(1, n))()
        hist = np.zeros((n, bins), np.uint32) if bins else None
        wanted = [("gauge", gauge), ("straight", straight), ("diagonal", diagonal), ("drop", drop)]
        got = {k: np.zeros(self.dimx * self.dimy, np.float64 if k == "drop" else np.uint32) for k, want in wanted if want}
        self._chk(self.L.smx_catchments(self.h, capi.ptr(cl), n, out, C.sizeof(capi.Catchment), capi.ptr(hist), bins, float(bin_height or 0.0),
                                        *[capi.ptr(got.get(k)) for k, _ in wanted]))
        recs = [out[k].as_dict() for k in range(n)]
        for k, r in enumerate(recs if bins else ()):
            r["hist"] = hist[k].copy()
        planes = {k: v.reshape(self.dimx, self.dimy) for k, v in got.items()}
        return (recs, planes) if planes else recs

    def horizons(self, directions=0xFFFF, reach: int = 0, suns=None, slope: bool = False, step: bool = False, sky: bool = False, open: bool = False,
                 lit: bool = False):
        """What every cell sees when it looks up along the lattice directions (``smx_horizons``). ``directions``: a 16-bit mask, or
        an iterable of indices 0..15 or of ``(ux, uy)`` pairs of ``capi.HORIZON_DIRECTIONS`` (counter-clockwise from +x); ``reach``:
        the steps a ray is followed at most, 0 = to the map's edge; ``suns``: what ``capi.horizon_suns`` takes or gives -- (azimuth,
        elevation) pairs in degrees, (d, tangent) pairs, at most 64, each towards a selected direction. One dict per selected
        direction in ascending d -- ``direction``, ``ux``, ``uy``, ``bounded`` (the cells with something above them that way),
        ``step_max`` / ``step_max_cell`` (the farthest horizon and the cell that has it), ``step_sum``, ``slope_max`` and
        ``lit_cells``: the number of cells each sun of THIS direction lights, in the order of ``suns``. With a plane asked for the
        result is ``(records, planes)``: ``slope`` (float64) and ``step`` (uint32) of shape (nd, dimx, dimy), plane j for the j-th
        selected direction -- the horizon slope S, +0.0 on open ground, and the step K that has it, 0 there --; ``sky`` (float64,
        the sky-view factor: the mean of 1 / (1 + S*S), 1.0 on open ground), ``open`` (uint32, bit d where nothing stands above the
        cell in direction d) and ``lit`` (uint32, the number of suns that light the cell) of shape (dimx, dimy). One call; sees
        every tick queued before it and changes nothing.

        The shadow of a low sun in the south-west and the shelter from a wind out of the north (Winstral's Sx within 64 cells)::

            d, tangent = capi.horizon_direction(azimuth=225.0, elevation=10.0)
            recs, pl = m.horizons([d], suns=[(d, tangent)], lit=True)
            shadow = pl["lit"] == 0
            up, _ = capi.horizon_direction(90.0, 0.0)          # the direction the wind comes from
            sx = m.horizons([up], reach=64, slope=True)[1]["slope"][0]
        """
        mask = capi.horizon_mask(directions)
        ds = [d for d in range(16) if mask >> d & 1]
        nd, n = max(1, len(ds)), self.dimx * self.dimy
        sl = capi.horizon_suns(list(suns)) if suns is not None and len(suns) else None
        ns = len(suns) if sl is not None else 0
        counts = np.zeros(max(1, ns), np.uint32)
        out = (capi.Horizon * nd)()
        wanted = [("slope", slope, np.float64, nd * n), ("step", step, np.uint32, nd * n), ("sky", sky, np.float64, n), ("open", open, np.uint32, n), ("lit", lit, np.uint32, n)]
        got = {k: np.zeros(size, dt) for k, want, dt, size in wanted if want}
        self._chk(self.L.smx_horizons(self.h, mask, int(reach), out, C.sizeof(capi.Horizon), sl, ns, capi.ptr(counts) if ns else None,
                                      *[capi.ptr(got.get(k)) for k, _, _, _ in wanted]))
        recs = [out[j].as_dict() for j in range(len(ds))]
        for r in recs:
            r["lit_cells"] = [int(counts[i]) for i in range(ns) if sl[i].direction == r["direction"]]
        planes = {k: v.reshape((len(ds), self.dimx, self.dimy) if k in ("slope", "step") else (self.dimx, self.dimy)) for k, v in got.items()}
        return (recs, planes) if planes else recs

    def proximity(self, cells=None, nearest: bool = False, group: bool = False, dist2: bool = False, bins: int = 0, bin_width: int = 1, cap: int | None = None):
        """How far every cell is from water or from a listed cell as the crow flies (``smx_proximity``): the exact Euclidean distance
        transform. ``cells`` None: the SITES are the wet cells, grouped by the lakes of ``lakes()`` (group k is lake k); else a
        sequence of distinct flat indices x*dimy + y or of ``(x, y)`` pairs, site ``cells[i]`` being group i. Every cell belongs to
        the ZONE of its nearest site's group -- the smaller squared distance, then the smaller site cell index. One dict per group,
        in group order -- ``site`` (the listed cell, or the lake's ``first_cell``), ``sites`` (1, or the lake's cells), ``cells`` (the
        size of the zone), ``dist2_max`` / ``farthest_cell`` (the largest squared distance in the zone and the smallest cell that
        has it), ``flags`` (1: the zone touches the map border), ``dist2_sum`` (exact) and the bounding box ``x0, y0, x1, y1``.
        ``bins`` (1 to 64) with ``bin_width``: every dict also gets ``buffers`` -- ``buffers[b]`` counts the zone's cells with
        ``b * bin_width <= floor(sqrt(dist2)) < (b + 1) * bin_width``, the last bin everything beyond. With a plane asked for the
        result is ``(records, planes)``, ``planes`` a dict of (dimx, dimy) uint32 arrays for EVERY cell: ``nearest`` (the cell index
        of the nearest site), ``group`` and ``dist2`` (the squared distance in cells; take the root for a distance); all three are
        0xFFFFFFFF on a map without a site. A list: one call; water: ``cap`` None makes two, a count and the fetch, else at most
        ``cap`` lakes get a record (the planes are whole either way). Sees every tick queued before it and changes nothing.

        A riparian buffer of five cells around the lakes, and the distance to the nearest channel as a covariate next to HAND::

            recs, pl = m.proximity(dist2=True)
            shore = pl["dist2"] <= 25
            channels = np.flatnonzero(m.streams(256, order=True)[1]["order"])
            away = np.sqrt(m.proximity(channels, dist2=True)[1]["dist2"])
        """
        cl, n = capi.proximity_cells(cells, self.dimy)
        bins, bin_width = int(bins), int(bin_width)
        count = C.c_uint32()
        wanted = [("nearest", nearest), ("group", group), ("dist2", dist2)]
        if cl is not None:
            cap = n
        elif cap is None:
            self._chk(self.L.smx_proximity(self.h, None, 0, None, C.sizeof(capi.Proximity), 0, C.byref(count), None, 0, 1, None, None, None))
            cap = int(count.value)
        cap = int(cap)
        out = (capi.Proximity * max(1, cap))()
        hist = np.zeros((cap, bins), np.uint32) if bins else None
        got = {k: np.zeros(self.dimx * self.dimy, np.uint32) for k, want in wanted if want}
        self._chk(self.L.smx_proximity(self.h, capi.ptr(cl), n, out if cap else None, C.sizeof(capi.Proximity), cap, C.byref(count), capi.ptr(hist), bins, bin_width,
                                       *[capi.ptr(got.get(k)) for k, _ in wanted]))
        recs = [out[k].as_dict() for k in range(min(cap, int(count.value)))]
        for k, r in enumerate(recs if bins else ()):
            r["buffers"] = hist[k].copy()
        planes = {k: v.reshape(self.dimx, self.dimy) for k, v in got.items()}
        return (recs, planes) if planes else recs

    def dispersal(self, exponent: int = 1, area: bool = False, donors: bool = False, receivers: bool = False, cap: int | None = None):
        """Dispersed flow (``smx_dispersal``): the multiple-flow-direction contributing area next to the D8 one of ``drainage()``. A
        dry cell splits its water over ALL lower neighbours in proportion to slope ** ``exponent`` (0 to 16; a diagonal step counts
        0.7071...), in fixed point with one cell = 2^24, so that every figure is an exact integer; what the truncated shares leave
        goes to the D8 receiver and nothing is lost. One dict per basin, record k for basin k of ``drainage()`` -- ``first_cell``,
        ``cells`` and ``flags`` (the basin), ``inflow_q24`` (what arrives at the sink or in the lake), ``leak_in_q24`` /
        ``leak_out_q24`` (what crosses the basin's divides: inflow = cells * 2^24 + leak_in - leak_out), ``peak_q24`` / ``peak_cell``
        (the largest area on the basin's dry land and the smallest cell that holds it; 0 and 0xFFFFFFFF for a lake without dry
        land), ``givers`` (dry cells with a lower neighbour) and ``split_cells`` (those with two or more), and the floats
        ``inflow``, ``leak_in``, ``leak_out`` and ``peak`` in cells. With a plane asked for the result is ``(records, planes)``,
        ``planes`` a dict of (dimx, dimy) arrays: ``area`` (uint64: divide by 2^24 for cells), ``donors`` (the higher dry
        neighbours) and ``receivers`` (the lower neighbours of a dry cell), uint32. ``cap`` None: two calls, the basin count and the
        fetch; else at most ``cap`` basins. Sees every tick queued before it and changes nothing; the number of rounds depends on the
        map (``dispersal_rounds()``)."""
        exponent = int(exponent)
        recs, planes = self._analysis(lambda out, cap, n, *pl: self.L.smx_dispersal(self.h, exponent, out, C.sizeof(capi.Dispersal), cap, n, *pl), capi.Dispersal, cap,
                                      [("area", area), ("donors", donors), ("receivers", receivers)], dtype={"area": np.uint64}, count=self._basin_count)
        return (recs, planes) if planes else recs

    def dispersal_rounds(self) -> tuple:
        """(rounds that found ready cells, batches) of the last ``dispersal()`` (``smx_get_dispersal_rounds``)."""
        a, b = C.c_uint32(), C.c_uint32()
        self._chk(self.L.smx_get_dispersal_rounds(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def budget(self, base: "Layermap", ntypes: int | None = None, dground: bool = False, dheight: bool = False, dsolid: bool = False, dwater: bool = False,
               cap: int | None = None):
        """The sediment budget (``smx_budget``): what changed from ``base`` -- another map of the same dimensions on the same device,
        typically the ``copy_from`` taken before the run -- to this map. Returns ``(basins, soils)``. ``basins``: one dict per
        drainage basin of the BASE in rank order -- ``first_cell`` and ``cells`` (join on them with ``base.drainage()``),
        ``lowered_cells`` / ``raised_cells`` (the ground went down / up; the ground is the top of the solid column, the floor of a
        water section), ``resurfaced_cells`` (another top type), ``eroded_q40`` / ``deposited_q40`` (the exact integer sums of the
        cells' losses / gains of floor(size * 2^40) over every section that is not Air), ``water_gained_q40`` / ``water_lost_q40``
        (the same for Air), ``cut_max`` / ``cut_cell`` and ``fill_max`` / ``fill_cell`` (the deepest cut and the highest fill and the
        smallest cell that has it; 0.0 and 0xFFFFFFFF without one), ``flags`` (1: a term was unreliable, 2: a sum wrapped, 4: a NaN
        ground) and the floats ``eroded``, ``deposited`` and ``net`` in height units x cells: the basin's sediment yield is
        ``-net``. ``soils``: one dict per type 0..ntypes-1 for the whole map -- ``gained_q40`` / ``lost_q40`` (the cells' gains /
        losses of the type's volume), ``held_gained_q40`` / ``held_lost_q40`` (the same on size * sat), ``cells_gained`` /
        ``cells_lost``, ``surfaced`` / ``covered`` (cells where the type came to the top / left it), ``flags`` and the floats
        ``gained``, ``lost`` and ``net``. ``ntypes`` None: the soil table's length, capped at 64. With a plane asked for the result
        is ``(basins, soils, planes)``, ``planes`` a dict of (dimx, dimy) arrays: ``dground`` and ``dheight`` (float64), ``dsolid``
        and ``dwater`` (int64, in units of 2^-40). ``cap`` None: two calls, the basin count and the fetch; else at most ``cap``
        basins. Sees every tick queued before it on either map and changes nothing."""
        nt = min(len(self._soils), capi.TOTALS_MAX_TYPES) if ntypes is None else int(ntypes)
        soils = (capi.BudgetSoil * max(1, nt))()

        def call(out, cap, n, *pl):
            fetch = out is not None or cap != 0 or any(p is not None for p in pl)        # (the counting call takes no soil table)
            return self.L.smx_budget(self.h, base.h, out, C.sizeof(capi.BudgetBasin), cap, n, soils if fetch else None, C.sizeof(capi.BudgetSoil), nt, *pl)

        recs, planes = self._analysis(call, capi.BudgetBasin, cap, [("dground", dground), ("dheight", dheight), ("dsolid", dsolid), ("dwater", dwater)],
                                      dtype={"dground": np.float64, "dheight": np.float64, "dsolid": np.int64, "dwater": np.int64})
        table = [soils[t].as_dict() for t in range(nt)]
        return (recs, table, planes) if planes else (recs, table)

    def hillslopes(self, threshold: int, entry: bool = False, hillslope: bool = False, straight: bool = False, diagonal: bool = False, hand: bool = False,
                   cap: int | None = None):
        """The land beside the channels (``smx_hillslopes``): one dict per segment, record k for segment k of ``streams(threshold)``
        -- ``first_cell`` (join on it with ``streams()``), ``cells`` (the dry cells off the channels whose entry lies on the
        segment), ``steps_max`` / ``farthest_cell`` (the longest way to the segment and the cell it starts at, 0xFFFFFFFF without a
        cell), ``straight_sum`` / ``diagonal_sum`` (flow length = straight + diagonal * sqrt(2)), ``hand_max``, ``hand_sum_q40`` (the
        exact integer sum of floor(hand * 2^40)) and ``hand_sum`` (that as a float), ``bank_cells`` (one step from the segment),
        ``head_cells`` (entering at the segment's first cell) and ``flags`` (1: ``hand_sum_q40`` unreliable). A dry cell's entry is
        the first channel cell, sink or wet cell on its way down, the cell itself included; ``hand`` is the cell's height above its
        entry. With a plane asked for the result is ``(records, planes)``, ``planes`` a dict of (dimx, dimy) arrays: ``entry`` (the
        entry's cell index), ``hillslope`` (the rank of the entry's segment, 0xFFFFFFFF for unchannelled land), ``straight`` /
        ``diagonal`` (steps to the entry), all uint32 and 0xFFFFFFFF / 0 for a wet cell, and ``hand`` (float64: the cells with
        ``hand < stage`` are under water at that stage). ``cap`` None: two calls, a count and the fetch; else at most ``cap``
        segments. Sees every tick queued before it and changes nothing."""
        threshold = int(threshold)
        recs, planes = self._analysis(lambda out, cap, n, *pl: self.L.smx_hillslopes(self.h, threshold, out, C.sizeof(capi.Hillslope), cap, n, *pl), capi.Hillslope,
                                      cap, [("entry", entry), ("hillslope", hillslope), ("straight", straight), ("diagonal", diagonal), ("hand", hand)],
                                      dtype={"hand": np.float64})
        return (recs, planes) if planes else recs

    # -- the strata read on the device --
    def soil_totals(self, ntypes: int | None = None, other: bool = False):
        """How much of each soil the map holds (``smx_soil_totals``): one dict per type 0..ntypes-1 -- ``sections`` (top sections
        included), ``cells`` (columns holding the type), ``top_cells`` (columns whose top section it is), ``volume_q40`` / ``held_q40``
        (the exact integer sums of floor(size * 2^40) and floor(size * sat * 2^40)), ``volume`` / ``held`` (those times 2^-40) and
        ``flags`` (1: volume unreliable, 2: held unreliable). ``ntypes`` None: the context's soil count, capped at 64. ``other``:
        also the number of sections of a type >= ntypes. Sees every tick queued before it and changes nothing."""
        nt = min(len(self._soils), capi.TOTALS_MAX_TYPES) if ntypes is None else int(ntypes)
        out = (capi.SoilTotal * max(1, nt))()
        rest = C.c_uint64()
        self._chk(self.L.smx_soil_totals(self.h, out, C.sizeof(capi.SoilTotal), nt, C.byref(rest)))
        recs = [out[t].as_dict() for t in range(nt)]
        return (recs, int(rest.value)) if other else recs

    def soil_thickness(self, types, cover: bool = False, sections: bool = False):
        """Per-cell planes for up to eight soil types from one walk of every column (``smx_soil_thickness``): ``thickness`` of shape
        (len(types), dimx, dimy), the summed sizes of the type's sections; with ``cover`` also the summed sizes of everything above the
        type's highest section (-1.0 where the column has none); with ``sections`` also the section counts (uint32). f64 sums in walk
        order, top to bottom. Returns the plane, or a tuple in the order thickness, cover, sections."""
        ty = np.ascontiguousarray(list(types), np.uint32)
        shape = (max(1, len(ty)), self.dimx * self.dimy)
        th = np.zeros(shape)
        cv = np.zeros(shape) if cover else None
        ns = np.zeros(shape, np.uint32) if sections else None
        self._chk(self.L.smx_soil_thickness(self.h, capi.ptr(ty), len(ty), capi.ptr(th), capi.ptr(cv), capi.ptr(ns)))
        out = [a.reshape(len(ty), self.dimx, self.dimy) for a in (th, cv, ns) if a is not None]
        return out[0] if len(out) == 1 else tuple(out)

    def cores(self, cells):
        """The columns under the listed cells (``smx_cores``; indices x*dimy + y, repeats allowed): ``count, type, size, floor, sat``
        in the snapshot layout -- columns in list order, sections bottom to top, ``count[i]`` of them for ``cells[i]``. Two calls, a
        count and the fetch; only the listed columns cross the host."""
        cl = np.ascontiguousarray(list(cells) if not isinstance(cells, np.ndarray) else cells, np.uint32)
        n = len(cl)
        count = np.zeros(n, np.uint32)
        total = C.c_uint64()
        rc = self.L.smx_cores(self.h, capi.ptr(cl), n, capi.ptr(count), 0, C.byref(total), None, None, None, None)
        if rc not in (0, 1):
            self._chk(rc)
        cap = int(total.value)
        ty, size, floor, sat = np.zeros(cap, np.uint32), np.zeros(cap), np.zeros(cap), np.zeros(cap)
        if rc == 1:
            self._chk(self.L.smx_cores(self.h, capi.ptr(cl), n, capi.ptr(count), cap, C.byref(total), capi.ptr(ty), capi.ptr(size), capi.ptr(floor), capi.ptr(sat)))
        return count, ty, size, floor, sat

    @staticmethod
    def transect_cells(p0, p1) -> list:
        """The cells (x, y) on the line from p0 to p1, both included. With dx = x1 - x0, dy = y1 - y0 and N = max(|dx|, |dy|), point i
        of 0..N is x0 + sgn(dx) * ((2*i*|dx| + N) // (2*N)) and likewise for y: the longer axis advances one cell per point, the
        shorter one rounds half away from p0. N = 0 is the single cell."""
        (x0, y0), (x1, y1) = (int(p0[0]), int(p0[1])), (int(p1[0]), int(p1[1]))
        dx, dy = x1 - x0, y1 - y0
        n = max(abs(dx), abs(dy))
        if n == 0:
            return [(x0, y0)]
        sx, sy = (dx > 0) - (dx < 0), (dy > 0) - (dy < 0)
        return [(x0 + sx * ((2 * i * abs(dx) + n) // (2 * n)), y0 + sy * ((2 * i * abs(dy) + n) // (2 * n))) for i in range(n + 1)]

    def transect(self, p0, p1):
        """The cores of the cells on the line from (x0, y0) to (x1, y1), in order (the rule: ``transect_cells``): ``cells`` (the
        indices x*dimy + y) and ``count, type, size, floor, sat`` as ``cores`` gives them. Both ends must lie on the map."""
        pts = self.transect_cells(p0, p1)
        for x, y in (pts[0], pts[-1]):
            if not (0 <= x < self.dimx and 0 <= y < self.dimy):
                raise ValueError(f"transect: ({x}, {y}) is outside the {self.dimx} x {self.dimy} map")
        cells = np.array([x * self.dimy + y for x, y in pts], np.uint32)
        return (cells,) + self.cores(cells)

    def counters(self) -> dict:
        c = capi.Counters()
        self._chk(self.L.smx_get_counters_sized(self.h, C.byref(c), C.sizeof(c)))
        return c.as_dict()

    def set_batch_dilate(self, tiles: int):
        self._chk(self.L.smx_set_batch_dilate(self.h, int(tiles)))

    def set_relax_wind(self, min_running: int = 0xFFFFFFFF, steps_per_epoch: int = 4):
        """relaxed schedule: wind steps relaxed (up to `steps_per_epoch` steps per epoch) while more than `min_running` particles run"""
        self._chk(self.L.smx_set_relax_wind(self.h, int(min_running), int(steps_per_epoch)))

    def set_relax_launch(self, persistent: int = -1, tail_at: int = -1):
        """relaxed water epochs: launch shape only, never the result (smx_set_relax_launch): persistent 1 = one cooperative launch per chunk,
        0 = five launches per epoch; tail_at = running particles from which one workgroup runs whole epochs (0..256); -1 = default"""
        self._chk(self.L.smx_set_relax_launch(self.h, int(persistent), int(tail_at)))

    def set_relax_settle(self, mode: int = -1, max_waves: int = 0, lanes: int = 0):
        """relaxed epochs, what follows apply: launch shape only, never the result (smx_set_relax_settle): mode 1 = one dataflow launch
        (k_relax_settle) where all its wavefronts are resident, 0 = filter + colour lists as two launches, 2 = as 1 with the water epochs' floods
        inside the same launch (k_relax_settle_floods) where settle and flood wavefronts are resident together, -1 = default; max_waves caps the
        resident wavefronts the fused launch may count on (0 = the device's), lanes = flagged cells per wavefront (0 = the rule's)"""
        self._chk(self.L.smx_set_relax_settle(self.h, int(mode), int(max_waves), int(lanes)))

    def set_analysis_launch(self, flow_blocks: int = 0, relax_blocks: int = 0, strata_blocks: int = 0):
        """the analyses' strided launches: launch shape only, never the result (smx_set_analysis_launch): the most workgroups of
        ``dispersal()``'s flow rounds (default 1024), of the relax, hop and exit sweeps of ``spill()`` and ``through()`` (2048) and of
        ``soil_totals()``, ``soil_thickness()`` and ``cores()`` (8192); 0 = the default. Holds for the calls on this map, not for an
        ensemble's"""
        self._chk(self.L.smx_set_analysis_launch(self.h, int(flow_blocks), int(relax_blocks), int(strata_blocks)))

    def analysis_launch(self) -> dict:
        """the values of ``set_analysis_launch`` in force (a default as its number) and, under ``flow_grid`` / ``relax_grid`` /
        ``strata_grid``, the workgroups the last call on this map gave each family's launches (0: none yet)"""
        b, g = (C.c_int32 * 3)(), (C.c_uint32 * 3)()
        self._chk(self.L.smx_get_analysis_launch(self.h, b, g))
        return {"flow_blocks": int(b[0]), "relax_blocks": int(b[1]), "strata_blocks": int(b[2]),
                "flow_grid": int(g[0]), "relax_grid": int(g[1]), "strata_grid": int(g[2])}

    def relax_settle_stats(self) -> dict:
        """cells that went through the waiting (crowded) path of k_relax_settle; dense epochs that took the fused / the two-launch path"""
        c, f, s = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._chk(self.L.smx_get_relax_settle(self.h, C.byref(c), C.byref(f), C.byref(s)))
        return {"crowded_cells": int(c.value), "epochs_fused": int(f.value), "epochs_split": int(s.value)}

    def relax_flood_flow_stats(self) -> dict:
        """water epochs that took k_relax_settle_floods (set_relax_settle mode 2), floods that acted in them, and those of them that found a
        flagged cell next to their tiles (a function of the input, not of timing)"""
        j, a, g = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._chk(self.L.smx_get_relax_flood_flow(self.h, C.byref(j), C.byref(a), C.byref(g)))
        return {"epochs_joined": int(j.value), "floods_acted": int(a.value), "floods_gated": int(g.value)}

    def set_water_generations(self, k: int):
        """throughput engines: the water phase's particles as k consecutive generations of n/k (smx_set_water_generations)"""
        self._chk(self.L.smx_set_water_generations(self.h, int(k)))

    def set_water_stagger(self, gap_epochs: int):
        """relaxed engine: the k generations of a water phase born `gap_epochs` apart inside ONE phase (smx_set_water_stagger; 0 = one after the other)"""
        self._chk(self.L.smx_set_water_stagger(self.h, int(gap_epochs)))

    def water_stagger(self) -> int:
        g = C.c_int32()
        self._chk(self.L.smx_get_water_stagger(self.h, C.byref(g)))
        return int(g.value)

    def water_generations(self) -> int:
        k = C.c_int32()
        self._chk(self.L.smx_get_water_generations(self.h, C.byref(k)))
        return int(k.value)

    def set_batch_strips(self, nstrips: int, inset: int = 16, seam_halfwidth: int = 48):
        self._chk(self.L.smx_set_batch_strips(self.h, int(nstrips), int(inset), int(seam_halfwidth)))

    def batch_stats(self) -> dict:
        e, g, l = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._chk(self.L.smx_get_batch_stats(self.h, C.byref(e), C.byref(g), C.byref(l)))
        return {"epochs": int(e.value), "generations": int(g.value), "children_lost": int(l.value)}

    def timing(self) -> dict:
        t = capi.Timing()
        self._chk(self.L.smx_get_timing_sized(self.h, C.byref(t), C.sizeof(t)))
        return t.as_dict()

    def timing_reset(self):
        self._chk(self.L.smx_timing_reset(self.h))

    def sync(self):
        self._chk(self.L.smx_sync(self.h))


class SoilMachine:
    """The tick driver of SoilMachine.cpp:283-329 (rendering removed) on top of a device ``Layermap``."""

    def __init__(self, cfg: SoilConfig, size: int | None = None, *, dimx: int | None = None, dimy: int | None = None,
                 seed: int = 0, nwater: int | None = None, nwind: int | None = None, dowater: bool = True,
                 dowind: bool = True, **kw):
        self.cfg = cfg
        self.map = Layermap(cfg, dimx if dimx is not None else size, dimy if dimy is not None else size, seed=seed, **kw)
        self.nwater = cfg.NWATER if nwater is None else nwater
        self.nwind = cfg.NWIND if nwind is None else nwind
        self.dowater, self.dowind = dowater, dowind

    def tick(self, n: int = 1, sync: bool = False):
        m = self.map
        for _ in range(n):
            m._chk(m.L.smx_tick(m.h, self.nwater, self.nwind, int(self.dowater), int(self.dowind)))
        if sync:
            m.sync()
            self._check_pool()

    def _check_pool(self):
        """The reference prints "Memory Pool Out-Of-Elements" and drops the section (layermap.h:92-95); here the
        counter is surfaced as a warning whenever it has grown since the last synchronised tick."""
        ov = self.map.counters()["pool_overflow"]
        if ov > getattr(self, "_pool_overflow_seen", 0):
            import warnings
            warnings.warn(f"soilmx: section pool exhausted ({ov} pool.get() failures so far, capacity {self.map.pool}): "
                          f"sections are being dropped exactly as the reference's POOLSIZE overflow does", RuntimeWarning)
            self._pool_overflow_seen = ov

    # phase-by-phase access, as the reference's host loop spells it out
    def water(self, n=None): self.map._chk(self.map.L.smx_tick_water(self.map.h, self.nwater if n is None else n))
    def grid_pass(self): self.map._chk(self.map.L.smx_grid_pass(self.map.h))
    def wind(self, n=None): self.map._chk(self.map.L.smx_tick_wind(self.map.h, self.nwind if n is None else n))
    def map_frequency(self): self.map._chk(self.map.L.smx_map_frequency(self.map.h))
    def reset_frequency(self): self.map._chk(self.map.L.smx_reset_frequency(self.map.h))
