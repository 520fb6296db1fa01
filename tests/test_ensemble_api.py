"""Ensembles (smx_ensemble_*) on a CPU-only box: the library exports the entry points, and creating an ensemble without a
GPU fails loudly (no CPU fallback) while destroying the handle it returned stays safe."""
import ctypes as C

import pytest

from soilmachine_amd import capi

ENSEMBLE_SYMBOLS = ["smx_ensemble_create", "smx_ensemble_destroy", "smx_ensemble_last_error", "smx_ensemble_add",
                    "smx_ensemble_remove", "smx_ensemble_size", "smx_ensemble_tick", "smx_ensemble_sync", "smx_ensemble_get_timing",
                    "smx_ensemble_timing_reset"]


def test_library_exports_the_ensemble_entry_points():
    L = capi.load()
    for n in ENSEMBLE_SYMBOLS:
        assert hasattr(L, n), f"libsoilmx.so does not export {n}"
        assert n in capi.SYMBOLS


def test_ensemble_create_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    L = capi.load()
    h = C.c_void_p()
    rc = L.smx_ensemble_create(0, C.byref(h))
    assert rc != 0
    msg = L.smx_ensemble_last_error(h)
    assert b"no HIP device" in msg or b"hip" in msg.lower()
    # a member cannot be added to the failed ensemble, and it says why
    cfg = capi.Config(16, 16, 80, 0, 4096, capi.ENGINE_SERIAL, 0)
    m = C.c_void_p()
    assert L.smx_ensemble_add(h, C.byref(cfg), C.byref(m)) != 0
    assert not m
    L.smx_ensemble_destroy(h)
    L.smx_ensemble_destroy(None)


def test_python_ensemble_raises_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from soilmachine_amd.ensemble import Ensemble
    from soilmachine_amd.machine import SoilmxError
    with pytest.raises(SoilmxError, match="smx_ensemble_create"):
        Ensemble(0)
