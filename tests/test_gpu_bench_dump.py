"""bench.py --dump-outputs end to end on the device: two runs with the same arguments write the same six arrays byte for byte, and
they are the state of the map after the warm-up and the timed ticks, read back from the same workload driven directly."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from common import ROOT, load_cfg

NAMES = {"cell_index": np.float64, "height": np.float64, "surface_type": np.float64,
         "water_frequency": np.float32, "water_track": np.float32, "wind_frequency": np.float32}
SIZE, STEPS, WARMUP = 64, 2, 1


def _bench(out_dir, detail_dir):
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [
        os.path.join(ROOT, "bench.py"), "--gpus", "1", "--size", str(SIZE), "--steps", str(STEPS), "--warmup", str(WARMUP),
        "--no-lines", "--no-cpu-baseline", "--dump-outputs", str(out_dir)]
    p = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, SMX_BENCH_DETAIL_DIR=str(detail_dir)), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_bench_dump_outputs_are_reproducible_and_are_the_timed_state(tmp_path):
    lines = [_bench(tmp_path / f"dump{k}", tmp_path / f"detail{k}") for k in range(2)]
    for ln in lines:
        assert ln["steps"] == STEPS and ln["warmup"] == WARMUP and ln["ms_per_step"] > 0
    got = []
    for k in range(2):
        d = tmp_path / f"dump{k}"
        assert sorted(p.name for p in d.iterdir()) == sorted(f"{n}.npy" for n in NAMES)
        arrs = {n: np.load(d / f"{n}.npy") for n in NAMES}
        for n, dt in NAMES.items():
            assert arrs[n].dtype == dt and arrs[n].shape == (SIZE * SIZE,), n
        got.append(arrs)
    for n in NAMES:
        assert got[0][n].tobytes() == got[1][n].tobytes(), n
    assert np.array_equal(got[0]["cell_index"], np.arange(SIZE * SIZE, dtype=np.float64))
    # the same workload driven directly (bench.py's counts for the relaxed engine at this size): warm-up + timed ticks, then the readers
    from soilmachine_amd import capi
    from soilmachine_amd.machine import SoilMachine
    cfg = load_cfg("rockgravelpebblessand.soil")
    area = (SIZE / 256.0) ** 2
    nwater, nwind = int(250 * area), int(250 * area * cfg.NWIND / max(cfg.NWATER, 1))
    sm = SoilMachine(cfg, SIZE, seed=0, nwater=nwater, nwind=nwind, dowind=nwind > 0, pool=max(10_000_000, 3 * SIZE * SIZE),
                     engine=capi.ENGINE_RELAXED)
    m = sm.map
    sm.tick(WARMUP, sync=True)                  # as bench.measure drives it
    for _ in range(STEPS):
        sm.tick(1)
        m.sync()
    wf, wt, wi = m.frequency()
    want = {"height": m.heights(), "surface_type": m.surface().astype(np.float64), "water_frequency": wf, "water_track": wt, "wind_frequency": wi}
    m.close()
    for n, a in want.items():
        assert got[0][n].tobytes() == a.tobytes(), n
