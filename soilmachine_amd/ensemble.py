"""Ensembles: many independent maps on the exact SERIAL engine, ticked together (smx_ensemble_* in include/soilmx.h).

Every member is an ordinary device context with the full ``Layermap`` interface, owned by its ``Ensemble``. One
``Ensemble.tick`` runs the tick loop of SoilMachine.cpp:283-329 on every member with a fixed number of kernel launches
for the whole ensemble; member i ends it in exactly the state a standalone SERIAL ``Layermap`` reaches from the same
inputs (hence the reference's state).
"""
from __future__ import annotations

import ctypes as C
from collections.abc import Sequence

import numpy as np

from . import capi
from .machine import Layermap, SoilmxError
from .soilfile import SoilConfig


class EnsembleMember(Layermap):
    """A member of an ``Ensemble``: a ``Layermap`` whose context the ensemble created and frees."""

    def __init__(self, ens: "Ensemble", cfg: SoilConfig, dimx: int | None = None, dimy: int | None = None, *, seed: int = 0,
                 pool: int | None = None, initialize: bool = True):
        self._ens = ens
        super().__init__(cfg, dimx, dimy, seed=seed, pool=pool, device=ens.device, engine=capi.ENGINE_SERIAL, initialize=initialize)

    def _open(self, c: capi.Config):
        h = C.c_void_p()
        rc = self.L.smx_ensemble_add(self._ens.h, C.byref(c), C.byref(h))
        if rc != 0:
            raise SoilmxError(f"smx_ensemble_add: {self._ens.last_error()} (rc={rc})")
        self._ens.members.append(self)              # the ensemble holds it from here on, whatever the set-up below does
        return h

    @classmethod
    def _wrap(cls, ens: "Ensemble", h, src: Layermap, pool: int) -> "EnsembleMember":
        """A member around a handle the library has already made and filled (smx_ensemble_fork): none of Layermap.__init__'s set-up."""
        m = cls.__new__(cls)
        m._ens = ens
        m.L = ens.L
        m.cfg, m.dimx, m.dimy, m.seed = src.cfg, src.dimx, src.dimy, src.seed
        m.pool = int(pool)
        m.x_range = None
        m._soils = src._soils
        m.h = C.c_void_p(h)
        return m

    def close(self):
        """Forget the handle; the context itself belongs to the ensemble (Ensemble.close frees it)."""
        self.h = None


class Ensemble:
    """A set of exact maps ticked together on one device (``smx_ensemble_*``)."""

    def __init__(self, device: int = 0):
        self.L = capi.load()
        self.device = int(device)
        self.members: list[EnsembleMember] = []
        h = C.c_void_p()
        rc = self.L.smx_ensemble_create(self.device, C.byref(h))
        if rc != 0:
            msg = self.L.smx_ensemble_last_error(h).decode() if h else "smx_ensemble_create failed"
            if h:
                self.L.smx_ensemble_destroy(h)
            raise SoilmxError(f"smx_ensemble_create: {msg} (rc={rc})")
        self.h = h

    # -- plumbing --
    def last_error(self) -> str:
        return self.L.smx_ensemble_last_error(self.h).decode()

    def _chk(self, rc: int):
        if rc != 0:
            raise SoilmxError(self.last_error() + f" (rc={rc})")

    def close(self):
        if getattr(self, "h", None):
            for m in self.members:
                m.h = None
            self.L.smx_ensemble_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self) -> int:
        return len(self.members)

    # -- members --
    def add(self, cfg: SoilConfig, dimx: int | None = None, dimy: int | None = None, *, seed: int = 0,
            pool: int | None = None, initialize: bool = True) -> EnsembleMember:
        """A new member: as ``Layermap(cfg, dimx, dimy, seed=seed, pool=pool)`` -- soils set, srand(seed), initialize(seed).
        ``pool`` defaults to the reference's POOLSIZE like ``Layermap``; pass a smaller one for many members. ``initialize`` off:
        an empty map, for a caller that loads a state (``Layermap.load`` / ``restore``)."""
        n = len(self.members)
        try:
            return EnsembleMember(self, cfg, dimx, dimy, seed=seed, pool=pool, initialize=initialize)
        except Exception:
            # set_soils / srand / initialize failed after smx_ensemble_add (e.g. smx_initialize's -4, a pool smaller than cells x
            # layers): take the half-made member out again, so that the ensemble holds exactly the members this object lists
            while len(self.members) > n:
                m = self.members.pop()
                if m.h:
                    self.L.smx_ensemble_remove(self.h, m.h)
                    m.h = None
            raise

    def fork(self, src: Layermap, n: int = 1, *, seeds=None, pool: int | None = None) -> list:
        """``n`` new members branched from ``src`` on the device (``smx_ensemble_fork``): each holds src's columns, frequency planes,
        soil table and SCALE with every counter but the live sections at zero. ``src`` is a ``Layermap`` of any engine or an
        ``EnsembleMember`` (of this ensemble or another) on this device and is only read. ``seeds`` None: every member continues
        src's rand() stream exactly; a sequence of n seeds: member i is as after ``srand(seeds[i])``. ``pool``: sections per
        member (None: src's own pool). If the call fails nothing is added."""
        n = int(n)
        sd = None
        if seeds is not None:
            sd = np.ascontiguousarray(list(seeds), np.uint32)
            if sd.shape != (n,):
                raise ValueError(f"seeds: {sd.size} seeds for {n} members")
        out = (C.c_void_p * max(n, 1))()
        self._chk(self.L.smx_ensemble_fork(self.h, src.h, n, int(pool or 0), capi.ptr(sd), out))
        made = [EnsembleMember._wrap(self, out[i], src, int(pool or src.pool)) for i in range(n)]
        self.members.extend(made)
        return made

    def remove(self, member: EnsembleMember):
        """Take `member` out of the ensemble and free it (smx_ensemble_remove); the members after it move up one place."""
        i = next((k for k, m in enumerate(self.members) if m is member), None)
        if i is None:
            raise ValueError("not a member of this ensemble")
        self._chk(self.L.smx_ensemble_remove(self.h, member.h))
        del self.members[i]
        member.h = None

    def size(self) -> int:
        n = C.c_int32()
        self._chk(self.L.smx_ensemble_size(self.h, C.byref(n)))
        return int(n.value)

    # -- ticks --
    def _counts(self, v, name: str) -> list:
        n = len(self.members)
        if v is None or isinstance(v, (int, np.integer)):
            return [v] * n
        if not isinstance(v, (Sequence, np.ndarray)):
            raise TypeError(f"{name}: an int, None or one entry per member")
        v = list(v)
        if len(v) != n:
            raise ValueError(f"{name}: {len(v)} counts for {n} members")
        return v

    def tick(self, nwater, nwind, dowater: bool = True, dowind: bool = True, n: int = 1):
        """``n`` ticks of SoilMachine.cpp:283-329 on every member. ``nwater`` / ``nwind``: an int for all members or one entry per
        member; a member whose ``nwater`` entry is None sits the tick out, and so does one whose ``nwind`` entry is None while
        ``dowind`` is set (without wind ``nwind`` is not read)."""
        if self.size() != len(self.members):
            raise SoilmxError(f"ensemble: the library holds {self.size()} members, this object lists {len(self.members)}")
        w = self._counts(nwater, "nwater")
        d = self._counts(nwind, "nwind") if dowind else [0] * len(self.members)
        on = [a is not None and b is not None for a, b in zip(w, d)]
        aw = np.array([int(a) if o else -1 for a, o in zip(w, on)], np.int32)
        ad = np.array([int(b) if o else 0 for b, o in zip(d, on)], np.int32)
        for _ in range(n):
            self._chk(self.L.smx_ensemble_tick(self.h, capi.ptr(aw), capi.ptr(ad), int(bool(dowater)), int(bool(dowind))))

    def sync(self):
        self._chk(self.L.smx_ensemble_sync(self.h))

    # -- the ensemble observed as one thing --
    def _check_members(self):
        if self.size() != len(self.members):
            raise SoilmxError(f"ensemble: the library holds {self.size()} members, this object lists {len(self.members)}")

    def figures(self) -> list:
        """One dict per member, in member order (``smx_ensemble_figures``: one launch for all members): the digest ``sumh`` /
        ``nsec`` / ``typehash`` (formatted as ``Snapshot.digest()``), ``wet_cells``, ``water_volume``, ``hmin``, ``hmax``,
        ``empty_cells``, ``rand_calls``, ``live_sections`` -- each bit-identical to the per-member readers on the same state. Sees
        every tick queued before it; no sync needed."""
        self._check_members()
        n = len(self.members)
        out = (capi.MemberFigures * n)()
        self._chk(self.L.smx_ensemble_figures(self.h, out, C.sizeof(capi.MemberFigures)))
        return [f.as_dict() for f in out]

    def plane_stats(self, plane: str = "height", members=None, *, var: bool = True, minmax: bool = True, nonzero: bool = True) -> dict:
        """Per-cell statistics of one plane ACROSS members (``smx_ensemble_plane_stats``): ``plane`` is "height", "water" (the top
        section's size where it is water, else 0), "wfreq" or "windfreq"; ``members`` a list of members or indices, folded in that
        order (None: all). Returns ``mean`` and, as asked, ``var`` (population variance), ``vmin`` / ``vmax``, ``nonzero`` (members
        with a value != 0) as flat arrays of dimx*dimy values in the plane's own indexing: x*dimy + y for the cell planes, like
        ``Layermap.heights()``, and y*dimx + x for the frequency planes, like ``Layermap.frequency()``. The selected members must
        have equal dims."""
        self._check_members()
        if plane not in capi.PLANES:
            raise ValueError(f"plane: one of {sorted(capi.PLANES)}")
        if members is None:
            idx = list(range(len(self.members)))
        else:
            idx = []
            for m in members:
                if isinstance(m, (int, np.integer)):
                    idx.append(int(m))
                else:
                    k = next((k for k, x in enumerate(self.members) if x is m), None)
                    if k is None:
                        raise ValueError("plane_stats: not a member of this ensemble")
                    idx.append(k)
        which = np.array(idx or [0], np.int32)
        # (the library checks the selection and names the offender; the shape comes from the first member it accepts)
        first = self.members[idx[0]] if idx and 0 <= idx[0] < len(self.members) else None
        cells = first.dimx * first.dimy if first else 1
        out = {"mean": np.zeros(cells)}
        if var:
            out["var"] = np.zeros(cells)
        if minmax:
            out["vmin"] = np.zeros(cells); out["vmax"] = np.zeros(cells)
        if nonzero:
            out["nonzero"] = np.zeros(cells, np.uint32)
        self._chk(self.L.smx_ensemble_plane_stats(self.h, capi.PLANES[plane], None if members is None else capi.ptr(which), len(idx), capi.ptr(out["mean"]), capi.ptr(out.get("var")),
                                                  capi.ptr(out.get("vmin")), capi.ptr(out.get("vmax")), capi.ptr(out.get("nonzero"))))
        return out

    def _analysis(self, call, rec, cap, count=None):
        """What the five terrain analyses share: the count call where ``cap`` is None (``count``, or ``call`` with no records), the
        array sized by the largest count, the fetch ``call(out, cap, counts)`` and one list of dicts per member."""
        self._check_members()
        n = len(self.members)
        if n == 0:
            return []
        counts = np.zeros(n, np.uint32)
        if cap is None:
            self._chk(count(capi.ptr(counts)) if count else call(None, 0, capi.ptr(counts)))
            cap = int(counts.max())
        cap = int(cap)
        out = (rec * max(1, n * cap))()
        self._chk(call(out, cap, capi.ptr(counts)))
        return [[out[i * cap + k].as_dict() for k in range(min(cap, int(counts[i])))] for i in range(n)]

    def _basin_counts(self, counts):
        """``spill`` and ``through`` take their counts from the drainage call: record k is basin k of ``drainage()``."""
        return self.L.smx_ensemble_drainage(self.h, None, C.sizeof(capi.Basin), 0, counts)

    def lakes(self, cap: int | None = None) -> list:
        """The lake census of every member (``smx_ensemble_lakes``: the same launches whatever the member count): one list of lake
        dicts per member, in member order, each as ``Layermap.lakes()`` gives it. ``cap`` None: two calls, a count with no records
        and the fetch sized by the largest count; else at most ``cap`` lakes per member. Members may differ in size."""
        return self._analysis(lambda out, cap, counts: self.L.smx_ensemble_lakes(self.h, out, C.sizeof(capi.Lake), cap, counts), capi.Lake, cap)

    def lake_counts(self) -> list:
        """The number of lakes of every member (``smx_ensemble_lakes`` with no records)."""
        self._check_members()
        counts = np.zeros(len(self.members), np.uint32)
        self._chk(self.L.smx_ensemble_lakes(self.h, None, C.sizeof(capi.Lake), 0, capi.ptr(counts)))
        return [int(c) for c in counts]

    def drainage(self, cap: int | None = None) -> list:
        """The basins of every member (``smx_ensemble_drainage``: the same launches whatever the member count): one list of basin
        dicts per member, in member order, each as ``Layermap.drainage()`` gives it. ``cap`` None: two calls, a count with no records
        and the fetch sized by the largest count; else at most ``cap`` basins per member. Members may differ in size."""
        return self._analysis(lambda out, cap, counts: self.L.smx_ensemble_drainage(self.h, out, C.sizeof(capi.Basin), cap, counts), capi.Basin, cap)

    def basin_counts(self) -> list:
        """The number of basins of every member (``smx_ensemble_drainage`` with no records)."""
        self._check_members()
        counts = np.zeros(len(self.members), np.uint32)
        self._chk(self.L.smx_ensemble_drainage(self.h, None, C.sizeof(capi.Basin), 0, capi.ptr(counts)))
        return [int(c) for c in counts]

    def streams(self, threshold: int, cap: int | None = None) -> list:
        """The channel segments of every member (``smx_ensemble_streams``: the same launches whatever the member count): one list of
        segment dicts per member, in member order, each as ``Layermap.streams(threshold)`` gives it. ``cap`` None: two calls, a count
        with no records and the fetch sized by the largest count; else at most ``cap`` segments per member. Members may differ in size."""
        threshold = int(threshold)
        return self._analysis(lambda out, cap, counts: self.L.smx_ensemble_streams(self.h, threshold, out, C.sizeof(capi.Stream), cap, counts), capi.Stream, cap)

    def hillslopes(self, threshold: int, cap: int | None = None) -> list:
        """The hillslope records of every member (``smx_ensemble_hillslopes``: the same launches whatever the member count): one list
        of dicts per member, in member order, each as ``Layermap.hillslopes(threshold)`` gives it, record k for segment k of
        ``streams(threshold)``. ``cap`` None: two calls, a count with no records and the fetch sized by the largest count; else at
        most ``cap`` segments per member. Members may differ in size."""
        threshold = int(threshold)
        return self._analysis(lambda out, cap, counts: self.L.smx_ensemble_hillslopes(self.h, threshold, out, C.sizeof(capi.Hillslope), cap, counts),
                              capi.Hillslope, cap)

    def flowpaths(self, cap: int | None = None) -> list:
        """The flow path records of every member (``smx_ensemble_flowpaths``: the same launches whatever the member count): one list
        of dicts per member, in member order, each as ``Layermap.flowpaths()`` gives it, record k for basin k of ``drainage()``;
        ``profile_at`` counts within the member. ``cap`` None: two calls, a count with no records and the fetch sized by the largest
        count; else at most ``cap`` basins per member. Members may differ in size."""
        return self._analysis(lambda out, cap, counts: self.L.smx_ensemble_flowpaths(self.h, out, C.sizeof(capi.Flowpath), cap, counts), capi.Flowpath, cap)

    def catchments(self, cells, bins: int = 0, bin_height: float | None = None) -> list:
        """The catchment records of every member (``smx_ensemble_catchments``: the same launches whatever the member count): one list
        of dicts per member, in member order, each as ``Layermap.catchments(cells, bins=bins, bin_height=bin_height)`` gives it.
        ONE list serves every member, as flat indices into each member's own plane: give ``(x, y)`` pairs only where all members
        have the same ``dimy`` (the first member's is used). Every listed cell has to lie inside every member."""
        self._check_members()
        nm = len(self.members)
        cl = np.asarray(cells if isinstance(cells, np.ndarray) else list(cells), np.int64)
        if cl.ndim == 2 and cl.shape[1] == 2:
            cl = cl[:, 0] * (self.members[0].dimy if nm else 1) + cl[:, 1]
        cl = np.ascontiguousarray(cl.reshape(-1), np.uint32)
        n, bins = len(cl), int(bins)
        out = (capi.Catchment * max(1, nm * n))()
        hist = np.zeros((max(1, nm), n, bins), np.uint32) if bins else None
        self._chk(self.L.smx_ensemble_catchments(self.h, capi.ptr(cl), n, out, C.sizeof(capi.Catchment), capi.ptr(hist), bins, float(bin_height or 0.0)))
        res = [[out[i * n + k].as_dict() for k in range(n)] for i in range(nm)]
        for i, recs in enumerate(res if bins else ()):
            for k, r in enumerate(recs):
                r["hist"] = hist[i, k].copy()
        return res

    def horizons(self, directions=0xFFFF, reach: int = 0, suns=None) -> list:
        """The horizon records of every member (``smx_ensemble_horizons``: the same launches whatever the member count): one list of
        dicts per member, in member order, each as ``Layermap.horizons(directions, reach, suns)`` gives it. ONE mask, reach and sun
        list serve every member; members may differ in size."""
        self._check_members()
        nm = len(self.members)
        mask = capi.horizon_mask(directions)
        ds = [d for d in range(16) if mask >> d & 1]
        nd = len(ds)
        sl = capi.horizon_suns(list(suns)) if suns is not None and len(suns) else None
        ns = len(suns) if sl is not None else 0
        counts = np.zeros(max(1, nm * ns), np.uint32)
        out = (capi.Horizon * max(1, nm * nd))()
        self._chk(self.L.smx_ensemble_horizons(self.h, mask, int(reach), out, C.sizeof(capi.Horizon), sl, ns, capi.ptr(counts) if ns else None))
        res = [[out[i * nd + j].as_dict() for j in range(nd)] for i in range(nm)]
        for i, recs in enumerate(res):
            for r in recs:
                r["lit_cells"] = [int(counts[i * ns + k]) for k in range(ns) if sl[k].direction == r["direction"]]
        return res

    def proximity(self, cells=None, bins: int = 0, bin_width: int = 1) -> list:
        """The proximity records of every member (``smx_ensemble_proximity``: the same launches whatever the member count): one list of
        dicts per member, in member order, each as ``Layermap.proximity(cells, bins=bins, bin_width=bin_width)`` gives it. ``cells``
        None: the wet cells of every member, grouped by its lakes (two calls, a count and the fetch sized by the largest count); else
        ONE list serves every member, as flat indices into each member's own plane: give ``(x, y)`` pairs only where all members have
        the same ``dimy`` (the first member's is used). Every listed cell has to lie inside every member."""
        self._check_members()
        nm = len(self.members)
        cl, n = capi.proximity_cells(cells, self.members[0].dimy if nm else 1)
        bins, bin_width = int(bins), int(bin_width)
        counts = np.zeros(max(1, nm), np.uint32)
        cap = n
        if cl is None:
            self._chk(self.L.smx_ensemble_proximity(self.h, None, 0, None, C.sizeof(capi.Proximity), 0, capi.ptr(counts), None, 0, 1))
            cap = int(counts[:nm].max()) if nm else 0
        out = (capi.Proximity * max(1, nm * cap))()
        hist = np.zeros((max(1, nm), cap, bins), np.uint32) if bins else None
        self._chk(self.L.smx_ensemble_proximity(self.h, capi.ptr(cl), n, out if cap else None, C.sizeof(capi.Proximity), cap, capi.ptr(counts), capi.ptr(hist), bins, bin_width))
        res = [[out[i * cap + k].as_dict() for k in range(min(cap, int(counts[i])))] for i in range(nm)]
        for i, recs in enumerate(res if bins else ()):
            for k, r in enumerate(recs):
                r["buffers"] = hist[i, k].copy()
        return res

    def dispersal(self, exponent: int = 1, cap: int | None = None) -> list:
        """The dispersed-flow records of every member (``smx_ensemble_dispersal``: the same launches whatever the member count): one
        list of dicts per member, in member order, each as ``Layermap.dispersal(exponent)`` gives it, record k for basin k of
        ``drainage()``. ``cap`` None: two calls, the basin counts and the fetch sized by the largest; else at most ``cap`` basins per
        member. Members may differ in size."""
        exponent = int(exponent)
        return self._analysis(lambda out, cap, counts: self.L.smx_ensemble_dispersal(self.h, exponent, out, C.sizeof(capi.Dispersal), cap, counts), capi.Dispersal, cap,
                              count=self._basin_counts)

    def dispersal_rounds(self) -> tuple:
        """(rounds that found ready cells, batches) of the last ``dispersal()`` (``smx_ensemble_get_dispersal_rounds``)."""
        a, b = C.c_uint32(), C.c_uint32()
        self._chk(self.L.smx_ensemble_get_dispersal_rounds(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def spill(self, cap: int | None = None) -> list:
        """The spill records of every member (``smx_ensemble_spill``: the same launches whatever the member count): one list of
        dicts per member, in member order, each as ``Layermap.spill()`` gives it. ``cap`` None: two calls, the basin counts and the
        fetch sized by the largest; else at most ``cap`` basins per member. Members may differ in size."""
        return self._analysis(lambda out, cap, counts: self.L.smx_ensemble_spill(self.h, out, C.sizeof(capi.Spill), cap, counts), capi.Spill, cap, count=self._basin_counts)

    def spill_sweeps(self) -> tuple:
        """(sweeps launched, batches) of the last ``spill()`` (``smx_ensemble_get_spill_sweeps``)."""
        a, b = C.c_uint32(), C.c_uint32()
        self._chk(self.L.smx_ensemble_get_spill_sweeps(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def through(self, cap: int | None = None) -> list:
        """The through-drainage records of every member (``smx_ensemble_through``: the same launches whatever the member count): one
        list of dicts per member, in member order, each as ``Layermap.through()`` gives it. ``cap`` None: two calls, the basin counts
        and the fetch sized by the largest; else at most ``cap`` basins per member. Members may differ in size."""
        return self._analysis(lambda out, cap, counts: self.L.smx_ensemble_through(self.h, out, C.sizeof(capi.Through), cap, counts), capi.Through, cap, count=self._basin_counts)

    def through_sweeps(self) -> tuple:
        """(level sweeps, hop sweeps, batches) of the last ``through()`` (``smx_ensemble_get_through_sweeps``)."""
        a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._chk(self.L.smx_ensemble_get_through_sweeps(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def set_analysis_launch(self, flow_blocks: int = 0, relax_blocks: int = 0, strata_blocks: int = 0):
        """The launch shape of this ensemble's ``dispersal()``, ``spill()`` / ``through()`` and ``soil_totals()``, never a result
        (``smx_ensemble_set_analysis_launch``; see ``Layermap.set_analysis_launch``). ``soil_totals()`` gives every member
        ``strata_blocks // len(ensemble)`` workgroups, at least one. Holds for the calls on the ensemble, not for a member's own."""
        self._chk(self.L.smx_ensemble_set_analysis_launch(self.h, int(flow_blocks), int(relax_blocks), int(strata_blocks)))

    def analysis_launch(self) -> dict:
        """The values in force and the workgroups of the last call's launches, as ``Layermap.analysis_launch`` gives them."""
        b, g = (C.c_int32 * 3)(), (C.c_uint32 * 3)()
        self._chk(self.L.smx_ensemble_get_analysis_launch(self.h, b, g))
        return {"flow_blocks": int(b[0]), "relax_blocks": int(b[1]), "strata_blocks": int(b[2]),
                "flow_grid": int(g[0]), "relax_grid": int(g[1]), "strata_grid": int(g[2])}

    def soil_totals(self, ntypes: int, other: bool = False) -> list:
        """The soil totals of every member (``smx_ensemble_soil_totals``: one table upload and one launch whatever the member count):
        one list of ``ntypes`` dicts per member, in member order, each as ``Layermap.soil_totals(ntypes)`` gives it. ``other``: a pair,
        the lists and each member's number of sections of a type >= ntypes. Members may differ in size and soil table."""
        self._check_members()
        n, nt = len(self.members), int(ntypes)
        out = (capi.SoilTotal * max(1, n * max(nt, 0)))()
        rest = np.zeros(max(1, n), np.uint64)
        self._chk(self.L.smx_ensemble_soil_totals(self.h, out, C.sizeof(capi.SoilTotal), nt, capi.ptr(rest)))
        recs = [[out[i * nt + t].as_dict() for t in range(nt)] for i in range(n)]
        return (recs, [int(v) for v in rest[:n]]) if other else recs

    def budget(self, base: Layermap, ntypes: int, cap: int | None = None) -> list:
        """How far every member moved from ``base`` (``smx_ensemble_budget``: the drainage chain once, on the base, and the same
        launches whatever the member count): one ``(basins, soils)`` per member, in member order, each as
        ``Layermap.budget(base, ntypes)`` gives it -- the basins are the BASE's, so every member has the same ones. ``base`` is a
        ``Layermap`` or an ``EnsembleMember`` of another ensemble with the members' dimensions on this device, typically the source
        of the fork. ``cap`` None: two calls, the basin count and the fetch; else at most ``cap`` basins per member."""
        self._check_members()
        n, nt = len(self.members), int(ntypes)
        if n == 0:
            return []
        count = C.c_uint32()
        if cap is None:
            self._chk(self.L.smx_ensemble_budget(self.h, base.h, None, C.sizeof(capi.BudgetBasin), 0, C.byref(count), None, 0, 0))
            cap = int(count.value)
        cap = int(cap)
        out = (capi.BudgetBasin * max(1, n * cap))()
        soils = (capi.BudgetSoil * max(1, n * max(nt, 0)))()
        self._chk(self.L.smx_ensemble_budget(self.h, base.h, out, C.sizeof(capi.BudgetBasin), cap, C.byref(count), soils, C.sizeof(capi.BudgetSoil), nt))
        k = min(cap, int(count.value))
        return [([out[i * cap + r].as_dict() for r in range(k)], [soils[i * nt + t].as_dict() for t in range(nt)]) for i in range(n)]

    def timing(self) -> dict:
        t = capi.Timing()
        self._chk(self.L.smx_ensemble_get_timing(self.h, C.byref(t), C.sizeof(t)))
        return t.as_dict()

    def timing_reset(self):
        self._chk(self.L.smx_ensemble_timing_reset(self.h))


__all__ = ["Ensemble", "EnsembleMember"]
