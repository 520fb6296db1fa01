"""The owner of a context's device and pinned memory (soilmachine_amd/csrc/soil_devmem.h) without a GPU: the header compiled by
tests/devmem_host over stand-ins of hipMalloc / hipHostMalloc / hipFree / hipHostFree that count, log and fail on demand. The
out-of-memory paths cannot be provoked on a device, so this is where they are exercised."""
import numpy as np
import pytest

from devmem_host_lib import BYTES, FREE, HOST_FREE, HOST_MALLOC, MALLOC, OOM, WORDS, Rig, calls, lib


@pytest.fixture
def rig():
    L = lib()
    assert L.dm_live_blocks() == 0, "an earlier test left blocks behind"
    L.dm_reset()
    r = Rig()
    yield r
    r.delete()
    assert L.dm_live_blocks() == 0 and L.dm_live_bytes() == 0, "destroying the owner must free everything it still holds"
    assert L.dm_wrong_free() == 0, "a block went through the other kind's free call"
    assert L.dm_unknown_free() == 0, "a pointer the stand-ins never handed out was freed"


def test_any_sequence_then_destroy_leaves_nothing(rig):
    """Allocate, grow and drop at random over all 16 slots, one allocation in seven failing; the stand-ins' live blocks and bytes
    follow a model all the way, and destroying the owner (the fixture) leaves 0 live blocks."""
    L = lib()
    rng = np.random.default_rng(5)
    slot = {}                     # slot -> (bytes, pinned) of the block its pointer names
    orphans = 0                   # bytes of blocks whose slot was overwritten: only the owner still knows them
    norphans = 0
    for step in range(400):
        s = int(rng.integers(0, 16))
        el = 4 if s in WORDS else 1
        op = int(rng.integers(0, 4))
        fail = rng.random() < 1 / 7
        n = int(rng.integers(1, 5000))
        if op == 3:
            rig.drop(s)
            slot.pop(s, None)
        elif op == 2:
            pinned = slot[s][1] if s in slot else bool(rng.integers(0, 2))
            cap = rig.cap(s)
            L.dm_fail_at(1 if fail else 0)
            rc = rig.grow(s, n, 2 * n, pinned)
            if n <= cap:
                assert rc == 0 and s in slot
            elif fail:
                assert rc == OOM and rig.ptr(s) == 0 and rig.cap(s) == 0
                slot.pop(s, None)
            else:
                assert rc == 0 and rig.cap(s) == 2 * n
                slot[s] = (2 * n * el, pinned)
        else:
            if rig.cap(s):
                continue          # (a slot under grow keeps to grow: its capacity names its block)
            L.dm_fail_at(1 if fail else 0)
            rc = rig.pinned(s, n) if op else rig.dev(s, n)
            if s in slot:
                orphans += slot.pop(s)[0]; norphans += 1
            if fail:
                assert rc == OOM and rig.ptr(s) == 0
            else:
                assert rc == 0 and rig.ptr(s) != 0
                slot[s] = (n * el, bool(op))
        L.dm_fail_at(0)
        assert L.dm_live_blocks() == len(slot) + norphans == rig.held(), f"step {step}"
        assert L.dm_live_bytes() == sum(b for b, _ in slot.values()) + orphans, f"step {step}"
    assert L.dm_live_blocks() > 0 and norphans > 0


def test_count_is_elements_of_the_pointer_type(rig):
    assert rig.dev(0, 1000) == 0 and rig.pinned(1, 3) == 0          # uint32_t*
    assert rig.dev(8, 1000) == 0 and rig.pinned(9, 3) == 0          # void*: bytes
    assert [(op, b) for op, _, b, _ in calls()] == [(MALLOC, 4000), (HOST_MALLOC, 12), (MALLOC, 1000), (HOST_MALLOC, 3)]


def test_grow_with_room_makes_no_call(rig):
    assert rig.grow(0, 100, 150) == 0 and rig.cap(0) == 150
    p, n = rig.ptr(0), lib().dm_calls()
    for need in (0, 1, 100, 149, 150):
        assert rig.grow(0, need, 4 * need + 1) == 0
    assert lib().dm_calls() == n and rig.ptr(0) == p and rig.cap(0) == 150


@pytest.mark.parametrize("pinned", [False, True])
def test_grow_frees_the_old_block_before_it_asks_for_the_new_one(rig, pinned):
    assert rig.grow(0, 100, 100, pinned) == 0
    n = lib().dm_calls()
    (_, old, _, _), = calls()
    assert rig.grow(0, 101, 150, pinned) == 0 and rig.cap(0) == 150
    a, f = (HOST_MALLOC, HOST_FREE) if pinned else (MALLOC, FREE)
    log = calls(n)
    assert [c[0] for c in log] == [f, a], "old block released first, then ONE request: peak memory stays that of the larger block"
    assert log[0][1] == old and log[0][2] == 400 and log[1][2] == 600
    assert lib().dm_live_blocks() == 1 and lib().dm_live_bytes() == 600


def test_failed_grow_leaves_null_and_zero_and_a_later_grow_works(rig):
    L = lib()
    assert rig.grow(0, 10, 10) == 0
    L.dm_fail_at(1)
    assert rig.grow(0, 20, 30) == OOM, "the runtime's error comes back to the call site"
    assert rig.ptr(0) == 0 and rig.cap(0) == 0, "no dangling pointer, no stale capacity"
    assert L.dm_live_blocks() == 0 and rig.held() == 0, "the old block was freed (before the request that failed)"
    assert [(c[0], c[3]) for c in calls()] == [(MALLOC, 1), (FREE, 1), (MALLOC, 0)]
    assert rig.grow(0, 20, 30) == 0 and rig.ptr(0) != 0 and rig.cap(0) == 30
    assert L.dm_live_blocks() == 1 and L.dm_live_bytes() == 120


def test_failed_allocation_leaves_null(rig):
    lib().dm_fail_at(1)
    assert rig.dev(0, 10) == OOM and rig.ptr(0) == 0 and rig.held() == 0
    lib().dm_fail_at(1)
    assert rig.pinned(8, 10) == OOM and rig.ptr(8) == 0 and rig.held() == 0


def test_drop_of_null_unknown_or_dropped_pointer_changes_nothing(rig):
    L = lib()
    assert rig.dev(0, 10) == 0 and rig.pinned(8, 10) == 0
    n = L.dm_calls()
    rig.drop(1); rig.drop(9)                                        # null
    rig.poke(10, 0x1234560)                                         # never handed out by this owner
    rig.drop(10)
    assert rig.ptr(10) == 0x1234560, "an unknown pointer is not the owner's to null"
    assert L.dm_calls() == n and L.dm_live_blocks() == 2 and rig.held() == 2
    rig.drop(0)
    assert rig.ptr(0) == 0 and L.dm_calls() == n + 1 and L.dm_live_blocks() == 1
    rig.drop(0); rig.drop(0)                                        # twice more: the pointer is null by now
    assert L.dm_calls() == n + 1 and L.dm_live_blocks() == 1 and rig.held() == 1
    rig.poke(10, 0)


def test_each_kind_goes_through_its_own_free_call():
    L = lib()
    assert L.dm_live_blocks() == 0
    L.dm_reset()
    r = Rig()
    assert r.dev(0, 1) == 0 and r.pinned(1, 2) == 0 and r.dev(2, 3) == 0 and r.pinned(3, 4) == 0
    r.grow(8, 5, 5, pinned=True); r.grow(9, 6, 6)
    kind = {bid: op for op, bid, _, _ in calls()}                   # block id -> MALLOC / HOST_MALLOC
    r.drop(0); r.drop(1)                                            # two by hand ...
    r.forget(2)                                                     # ... one whose pointer is lost ...
    r.delete()                                                      # ... and the rest by the destructor
    frees = [(op, bid) for op, bid, _, _ in calls() if op in (FREE, HOST_FREE)]
    assert len(frees) == 6 and L.dm_live_blocks() == 0
    for op, bid in frees:
        assert op == (HOST_FREE if kind[bid] == HOST_MALLOC else FREE), f"block {bid}"
    assert L.dm_wrong_free() == 0 and L.dm_unknown_free() == 0


@pytest.mark.parametrize("fail_at", [1, 2])
def test_allocate_new_then_swap_keeps_the_old_pair_when_either_allocation_fails(rig, fail_at):
    """ens_reserve / ens_obs_reserve: a device + pinned pair is replaced only once BOTH new blocks exist."""
    L = lib()
    assert rig.swap_pair(0, 1, 64) == 0
    d, h = rig.ptr(0), rig.ptr(1)
    assert d and h and L.dm_live_blocks() == 2 and L.dm_live_bytes() == 2 * 256
    n = L.dm_calls()
    L.dm_fail_at(fail_at)
    assert rig.swap_pair(0, 1, 128) == -1
    assert (rig.ptr(0), rig.ptr(1), rig.cap(0), rig.cap(1)) == (d, h, 64, 64), "the old pair stays"
    assert L.dm_live_blocks() == 2 and L.dm_live_bytes() == 2 * 256 and rig.held() == 2, "the new block that did come was dropped again"
    want = [(MALLOC, 0)] if fail_at == 1 else [(MALLOC, 1), (HOST_MALLOC, 0), (FREE, 1)]
    assert [(c[0], c[3]) for c in calls(n)] == want
    assert rig.swap_pair(0, 1, 128) == 0                            # and with memory to be had, the swap goes through
    assert rig.ptr(0) not in (0, d) and rig.ptr(1) not in (0, h) and rig.cap(0) == 128
    assert L.dm_live_blocks() == 2 and L.dm_live_bytes() == 2 * 512
