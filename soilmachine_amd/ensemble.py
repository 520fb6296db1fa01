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
                 pool: int | None = None):
        self._ens = ens
        super().__init__(cfg, dimx, dimy, seed=seed, pool=pool, device=ens.device, engine=capi.ENGINE_SERIAL)

    def _open(self, c: capi.Config):
        h = C.c_void_p()
        rc = self.L.smx_ensemble_add(self._ens.h, C.byref(c), C.byref(h))
        if rc != 0:
            raise SoilmxError(f"smx_ensemble_add: {self._ens.last_error()} (rc={rc})")
        self._ens.members.append(self)              # the ensemble holds it from here on, whatever the set-up below does
        return h

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
            pool: int | None = None) -> EnsembleMember:
        """A new member: as ``Layermap(cfg, dimx, dimy, seed=seed, pool=pool)`` -- soils set, srand(seed), initialize(seed).
        ``pool`` defaults to the reference's POOLSIZE like ``Layermap``; pass a smaller one for many members."""
        n = len(self.members)
        try:
            return EnsembleMember(self, cfg, dimx, dimy, seed=seed, pool=pool)
        except Exception:
            # set_soils / srand / initialize failed after smx_ensemble_add (e.g. smx_initialize's -4, a pool smaller than cells x
            # layers): take the half-made member out again, so that the ensemble holds exactly the members this object lists
            while len(self.members) > n:
                m = self.members.pop()
                if m.h:
                    self.L.smx_ensemble_remove(self.h, m.h)
                    m.h = None
            raise

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

    def timing(self) -> dict:
        t = capi.Timing()
        self._chk(self.L.smx_ensemble_get_timing(self.h, C.byref(t), C.sizeof(t)))
        return t.as_dict()

    def timing_reset(self):
        self._chk(self.L.smx_ensemble_timing_reset(self.h))


__all__ = ["Ensemble", "EnsembleMember"]
