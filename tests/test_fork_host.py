"""Forking a map (smx_copy_state / smx_ensemble_fork) without a GPU: the bodies of k_fork_count / k_fork_scatter / k_fork_planes
(soilmachine_amd/csrc/soil_fork.h) compiled for the host by tests/fork_host and run with the lanes looped, against a numpy
restatement of the pool layout smx_import_columns produces, on the committed golden snapshots and on a synthetic map."""
import ctypes as C
import ctypes.util

import numpy as np
import pytest

from common import golden_snapshot
from fork_host_lib import (EMPTY, F_AIR, F_SAT, NIL, PATTERN, RAND_WORDS, SEC, SOIL_WORDS, Dest, fork, import_layout, lib, rand_seed,
                           scrambled_source)
from soilmachine_amd import capi
from soilmachine_amd.snapshot import Snapshot

GOLDEN = [("default64", 20), ("rgps64", 10), ("rocksand48x80", 5), ("painted64", 5)]


def synthetic() -> Snapshot:
    """37 x 29 cells (no multiple of any group width): empty columns, single-section columns, columns of 2..40 sections, water on
    top of some, saturations in some buried sections."""
    rng = np.random.default_rng(11)
    dimx, dimy = 37, 29
    n = dimx * dimy
    count = rng.choice([0, 1, 1, 2, 3, 5, 40], n).astype(np.uint32)
    count[:3] = (0, 1, 0); count[-2:] = (1, 0)
    ns = int(count.sum())
    ty = rng.integers(1, 5, ns).astype(np.uint32)
    end = np.cumsum(count.astype(np.int64))
    tops = end[count > 0] - 1
    ty[tops[::7]] = 0                                         # water on top of every 7th non-empty column
    sat = np.where(rng.random(ns) < 0.05, rng.random(ns), 0.0)
    f = lambda: rng.random(n).astype(np.float32)
    return Snapshot(dimx, dimy, 80, 5, 12345, 0, count, ty, rng.random(ns), rng.random(ns), sat, f(), f(), f())


def source_of(s: Snapshot, seed: int, slack: int = 100):
    """(cells, pool, flags, sticky): `s` in a scrambled pool with `slack` free records; the flag plane carries sticky F_SAT bits on
    columns that hold no saturation now, and F_AIR bits that are stale (the fork must derive that bit, not copy it)."""
    rng = np.random.default_rng(seed)
    lay = import_layout(s, s.nsec)
    cells, pool = scrambled_source(lay, lay["used"] + slack, rng)
    sticky = np.where(rng.random(s.ncells) < 0.1, F_SAT, 0).astype(np.uint8)
    assert ((sticky != 0) & ((lay["flags"] & F_SAT) == 0)).any()
    flags = (lay["flags"] & F_SAT) | sticky | np.where(rng.random(s.ncells) < 0.5, F_AIR, 0).astype(np.uint8)
    return cells, pool, flags, sticky


def assert_layout(d: Dest, want: dict, cap: int, what: str):
    used = want["used"]
    assert d.cells.tobytes() == want["cells"].tobytes(), f"{what}: cell records"
    assert d.pool[:used].tobytes() == want["pool"].tobytes(), f"{what}: pool[0..used)"
    assert int(d.free_count[0]) == want["free_count"] == cap - used, f"{what}: free_count"
    assert np.array_equal(d.freelist[:cap - used], want["freelist"]), f"{what}: free list"
    assert np.array_equal(d.flags, want["flags"]), f"{what}: flag plane"
    assert int(d.ctr[lib().fh_live_counter()]) == want["live"], f"{what}: live sections"
    assert d.pool[used:].tobytes() == bytes([PATTERN]) * ((cap - used) * SEC.itemsize), f"{what}: pool records past `used` were written"
    assert (d.freelist[cap - used:] == 0xA5A5A5A5).all(), f"{what}: free-list entries past free_count were written"


def snapshots():
    return [(f"{c}.t{t}", golden_snapshot(c, t)) for c, t in GOLDEN] + [("synthetic", synthetic())]


SNAPS = snapshots()


# ---------------------------------------------------------------- 1. the entry points exist and refuse nonsense without a device
def test_symbols_and_null_arguments():
    L = capi.load()
    for n in ("smx_copy_state", "smx_ensemble_fork"):
        assert hasattr(L, n), f"libsoilmx.so does not export {n}"
        assert n in capi.SYMBOLS
    out = (C.c_void_p * 1)()
    assert L.smx_copy_state(None, None) == -2
    assert L.smx_ensemble_fork(None, None, 1, 0, None, out) == -2
    assert lib().fh_max_lanes() == 256


# ---------------------------------------------------------------- 2. the import layout, byte for byte
@pytest.mark.parametrize("name,s", SNAPS, ids=[n for n, _ in SNAPS])
def test_layout_equals_the_import_layout(name, s):
    if name == "default64.t20":
        wet = int((s.type[np.cumsum(s.count.astype(np.int64))[s.count > 0] - 1] == 0).sum())
        assert wet == 399 and (s.sat != 0).any()
    if name == "rgps64.t10":
        assert s.nsec == 124893 and int(s.count.max()) == 893
    cells, pool, flags, sticky = source_of(s, 5)
    rng = np.random.default_rng(9)
    planes = rng.random(3 * s.ncells).astype(np.float32)
    soils = rng.integers(0, 2**32, 5 * SOIL_WORDS, dtype=np.uint64).astype(np.uint32)
    rnd = rng.integers(0, 2**32, RAND_WORDS, dtype=np.uint64).astype(np.uint32)
    for cap in (s.nsec, s.nsec + 1000):                        # cap == sum of the counts succeeds
        rc, d, info = fork(cells, pool, flags, cap, planes=planes, soils=soils, rnd=rnd)
        assert rc == 0 and info["bad"] == 2**64 - 1, (name, rc, info)
        want = import_layout(s, cap, sticky)
        assert info["used"] == want["used"] and info["used"] + info["nonempty"] == s.nsec
        assert_layout(d, want, cap, f"{name}, cap {cap}")
        assert np.array_equal(d.planes.view(np.uint32), planes.view(np.uint32)), "frequency planes"
        assert np.array_equal(d.soils[:soils.size], soils) and (d.soils[soils.size:] == 0xA5A5A5A5).all(), "soil table"
        assert np.array_equal(d.rnd, rnd), "the generator, continued"
        others = np.delete(d.ctr, lib().fh_live_counter())
        assert (others == 0xA5A5A5A5A5A5A5A5).all(), "other counters were written"
    keep = (sticky != 0) & ((import_layout(s, s.nsec)["flags"] & F_SAT) == 0)
    assert keep.any() and (d.flags[keep] & F_SAT).all(), "sticky F_SAT bits on columns without a saturation"
    empty = s.count == 0
    if empty.any():
        e = d.cells[empty]
        assert (e["type"] == EMPTY).all() and (e["prev"] == NIL).all() and not e["size"].any() and not e["floor"].any() and not e["sat"].any()


def test_layout_does_not_depend_on_the_source_pool():
    s = golden_snapshot("rgps64", 10)
    images = set()
    for seed, slack in ((1, 0), (2, 17), (3, 5000)):
        cells, pool, flags, _ = source_of(s, seed, slack)
        flags = import_layout(s, s.nsec)["flags"]             # (the same flag plane: only the pool differs)
        rc, d, _ = fork(cells, pool, flags, s.nsec + 64)
        assert rc == 0
        images.add(d.image())
    assert len(images) == 1


# ---------------------------------------------------------------- 3. lane independence
@pytest.mark.parametrize("name,s", [SNAPS[1], SNAPS[2], SNAPS[4]], ids=[SNAPS[i][0] for i in (1, 2, 4)])
def test_result_does_not_depend_on_the_group_width(name, s):
    cells, pool, flags, _ = source_of(s, 21)
    planes = np.random.default_rng(2).random(3 * s.ncells).astype(np.float32)
    images = {}
    for lanes in (1, 64, 96, 256):
        rc, d, info = fork(cells, pool, flags, s.nsec + 3, lanes=lanes, planes=planes, rnd=rand_seed(4))
        assert rc == 0
        images[lanes] = (d.image(), tuple(info.values()))
    assert len(set(images.values())) == 1, f"{name}: the result depends on the lanes per group"
    assert fork(cells, pool, flags, s.nsec, lanes=0)[0] == -2 and fork(cells, pool, flags, s.nsec, lanes=257)[0] == -2


# ---------------------------------------------------------------- 4. capacity
@pytest.mark.parametrize("name,s", [SNAPS[0], SNAPS[4]], ids=[SNAPS[0][0], SNAPS[4][0]])
def test_capacity_rule(name, s):
    cells, pool, flags, _ = source_of(s, 8)
    rc, d, _ = fork(cells, pool, flags, s.nsec)
    assert rc == 0 and int(d.free_count[0]) == s.nsec - import_layout(s, s.nsec)["used"]
    rc, d, info = fork(cells, pool, flags, s.nsec - 1)
    assert rc == -4 and info["used"] + info["nonempty"] == s.nsec
    assert d.image() == Dest(s.ncells, s.nsec - 1, lib().fh_counters()).image(), "-4 must leave the destination untouched"


# ---------------------------------------------------------------- 5. corrupt chains
def deep_cell(s: Snapshot, at_least: int = 3) -> int:
    return int(np.nonzero(s.count >= at_least)[0][7])


@pytest.mark.parametrize("lanes", [64, 256])
def test_corrupt_chains_are_refused_with_the_cell(lanes):
    s = golden_snapshot("rocksand48x80", 5)
    cells, pool, flags, _ = source_of(s, 13)
    cap_src = pool.shape[0]
    c = deep_cell(s)
    untouched = Dest(s.ncells, s.nsec, lib().fh_counters()).image()
    # a link that leaves the pool
    bad = pool.copy()
    bad["prev"][cells["prev"][c]] = cap_src
    rc, d, info = fork(cells, bad, flags, s.nsec, lanes=lanes)
    assert rc == -5 and info["bad"] == c and d.image() == untouched
    bad_cells = cells.copy()
    bad_cells["prev"][c] = cap_src + 5                           # ... straight from the cell record
    rc, d, info = fork(bad_cells, pool, flags, s.nsec, lanes=lanes)
    assert rc == -5 and info["bad"] == c and d.image() == untouched
    # a cycle: the second buried section points back at the first
    cyc = pool.copy()
    first = cells["prev"][c]
    cyc["prev"][pool["prev"][first]] = first
    rc, d, info = fork(cells, cyc, flags, s.nsec, lanes=lanes)
    assert rc == -5 and info["bad"] == c and d.image() == untouched
    # two bad cells: the first one in cell order is named
    c2 = int(np.nonzero(s.count >= 3)[0][2])
    assert c2 < c
    two = bad.copy()
    two["prev"][cells["prev"][c2]] = 0xFFFFFFF0
    rc, d, info = fork(cells, two, flags, s.nsec, lanes=lanes)
    assert rc == -5 and info["bad"] == c2 and d.image() == untouched
    # a chain as long as the pool is sound: links == cap is allowed
    n1 = np.zeros(1, SEC); n1["type"] = 2; n1["prev"] = 3
    chain = np.zeros(4, SEC); chain["type"] = 1; chain["prev"] = [NIL, 0, 1, 2]
    rc, d, info = fork(n1, chain, np.zeros(1, np.uint8), 5, lanes=lanes)
    assert rc == 0 and info["used"] == 4 and list(d.pool["prev"][:4]) == [NIL, 0, 1, 2] and int(d.cells["prev"][0]) == 3


# ---------------------------------------------------------------- 6. the seeded generator is libc's
@pytest.mark.parametrize("seed", [0, 1, 14, 2**31 + 5])
def test_seeded_members_get_libc_srand(seed):
    s = synthetic()
    cells, pool, flags, _ = source_of(s, 3)
    rc, d, _ = fork(cells, pool, flags, s.nsec, rnd=rand_seed(99), seed=seed)
    assert rc == 0 and np.array_equal(d.rnd, rand_seed(seed))
    ring, idx, calls = [int(v) for v in d.rnd[:31]], int(d.rnd[31]), int(d.rnd[32]) | int(d.rnd[33]) << 32
    assert calls == 0
    libc = C.CDLL(ctypes.util.find_library("c"))
    libc.srand(C.c_uint(seed))
    for _ in range(40):
        v = (ring[idx % 31] + ring[(idx - 3) % 31]) & 0xFFFFFFFF
        ring[idx % 31] = v
        idx += 1
        assert v >> 1 == libc.rand()
