"""The scratch of the five terrain analyses (soilmachine_amd/csrc/soil_scratch.h) without a GPU: AnalysisScratch compiled by
tests/devmem_host over the stand-in allocator, which counts, logs and fails on demand. Scratch growth under memory pressure can fail
in production without ever failing on a device in a test, so this is where every one of its out-of-memory paths runs."""
from collections import namedtuple

import pytest

from devmem_host_lib import FREE, HOST_FREE, HOST_MALLOC, MALLOC, OOM, Rig, calls, lib

Need = namedtuple("Need", "words planes more f64 temp_bytes members count_words res_bytes")
MEMBER = 32                                   # sizeof(LakeMember)
H64, TEMP, D_TAB, H_TAB, D_CNT, H_CNT, D_RES, H_RES = range(10, 18)   # Rig.as_ptrs(): 0 .. 9 are the u32 planes
RESULT = [D_RES, H_RES]


def count_words(nm):                          # spill and through: the counts, then 16 change counts
    return ((nm + 15) & ~15) + 16


def head(nm):                                 # the others: the counts in front of the records
    return (nm * 4 + 63) & ~63


# a need shaped like each analysis: 3 maps of 9 x 7, 33 x 47 and 1 x 70 cells, records of 64 (48: basins) bytes
W, NM = 9 * 7 + 33 * 47 + 70, 3
NEEDS = {
    "lakes": Need(W, 2, 0, 0, 1543, NM, 0, head(NM) + 40 * 64),
    "drainage": Need(W, 3, 0, 0, 1543, NM, 0, head(NM) + 200 * 48),
    "drainage_area": Need(W, 3, 2, 0, 1543, NM, 0, head(NM) + 200 * 48),
    "streams": Need(W, 10, 0, 0, 1543, NM, 0, head(NM) + 90 * 64),
    "spill_chain": Need(W, 4, 0, 1, 1543, NM, count_words(NM), 0),          # before the basins are counted: no result region yet
    "spill": Need(W, 4, 0, 1, 1543, NM, count_words(NM), 200 * 64),
    "through": Need(W, 5, 0, 1, 1543, NM, count_words(NM), 200 * 128),
}


def blocks(n: Need) -> list:
    """(op, bytes) of a fresh reserve's allocation calls, in order."""
    out = [(MALLOC, 4 * n.words)] * (n.planes) + [(MALLOC, 8 * n.words)] * n.f64 + [(MALLOC, 4 * n.words)] * n.more
    out += [(MALLOC, n.temp_bytes), (MALLOC, 2 * n.members * MEMBER), (HOST_MALLOC, 2 * n.members * MEMBER)]
    if n.count_words:
        out += [(MALLOC, 4 * n.count_words), (HOST_MALLOC, 4 * n.count_words)]
    if n.res_bytes:
        out += [(MALLOC, n.res_bytes), (HOST_MALLOC, n.res_bytes)]
    return out


def held(n: Need) -> list:
    """The pointers a scratch reserved for n holds."""
    p = list(range(n.planes + n.more)) + [H64] * n.f64 + [TEMP, D_TAB, H_TAB]
    return sorted(p + ([D_CNT, H_CNT] if n.count_words else []) + (RESULT if n.res_bytes else []))


def caps(n: Need) -> list:
    return [n.words, n.words if n.more else 0, n.temp_bytes, n.members, n.res_bytes]


def assert_holds(rig, n: Need):
    ptrs = rig.as_ptrs()
    assert sorted(k for k, p in enumerate(ptrs) if p) == held(n)
    assert len({p for p in ptrs if p}) == len(held(n)), "every pointer names a block of its own"
    assert rig.as_caps() == caps(n) and rig.as_fits(n)


def assert_empty(rig):
    assert rig.as_ptrs() == [0] * 18, "no dangling pointer"
    assert rig.as_caps() == [0] * 5, "no stale capacity"
    assert lib().dm_live_blocks() == 0 and rig.held() == 0


@pytest.fixture
def rig():
    L = lib()
    assert L.dm_live_blocks() == 0, "an earlier test left blocks behind"
    L.dm_reset()
    r = Rig()
    yield r
    r.as_drop()
    assert L.dm_live_blocks() == 0 and r.held() == 0, "drop leaves nothing with the owner"
    r.delete()
    assert L.dm_wrong_free() == 0, "a block went through the other kind's free call"
    assert L.dm_unknown_free() == 0, "a pointer the stand-ins never handed out was freed"


@pytest.mark.parametrize("name", list(NEEDS))
def test_fresh_reserve_accounts_for_every_block_and_drop_frees_them(rig, name):
    L, n = lib(), NEEDS[name]
    assert not rig.as_fits(n)
    assert rig.as_reserve(n) == 0
    assert [(op, b) for op, _, b, ok in calls() if ok] == blocks(n)
    assert L.dm_live_blocks() == len(blocks(n)) == rig.held() and L.dm_live_bytes() == sum(b for _, b in blocks(n))
    assert_holds(rig, n)
    rig.as_drop()
    assert_empty(rig)
    assert sorted(op for op, _, _, _ in calls()[len(blocks(n)):]) == sorted(FREE if op == MALLOC else HOST_FREE for op, _ in blocks(n))


@pytest.mark.parametrize("name", list(NEEDS))
def test_any_failed_allocation_drops_everything_and_the_same_reserve_then_works(rig, name):
    L, n = lib(), NEEDS[name]
    for k in range(1, len(blocks(n)) + 1):
        L.dm_fail_at(k)
        assert rig.as_reserve(n) == OOM, f"allocation {k} failed: reserve says so"
        L.dm_fail_at(0)
        assert_empty(rig)
        assert rig.as_reserve(n) == 0
        assert L.dm_live_blocks() == len(blocks(n))
        assert_holds(rig, n)
        rig.as_drop()
    assert_empty(rig)


def test_a_failed_growth_drops_the_groups_that_were_not_growing_too(rig):
    """Nothing half-sized stays behind: the old planes went before their replacement was asked for, and when that request fails the
    tables, the temporary storage and the result region go as well."""
    L, n = lib(), NEEDS["through"]
    big = n._replace(words=2 * n.words)
    for k in range(1, big.planes + 2):
        assert rig.as_reserve(n) == 0
        L.dm_fail_at(k)
        assert rig.as_reserve(big) == OOM
        L.dm_fail_at(0)
        assert_empty(rig)
    assert rig.as_reserve(big) == 0
    assert_holds(rig, big)


def grown(rig, before: Need, after: Need, moved: list):
    """Reserve `before`, then `after`: only the pointers in `moved` name another block than before (by serial number: an address may
    come again); returns the second reserve's log."""
    assert rig.as_reserve(before) == 0
    was, start = rig.as_blocks(), lib().dm_calls()
    assert not rig.as_fits(after)
    assert rig.as_reserve(after) == 0
    now = rig.as_blocks()
    assert [k for k in range(18) if now[k] != was[k]] == sorted(moved)
    assert_holds(rig, after)
    return calls(start)


@pytest.mark.parametrize("name", ["lakes", "drainage_area", "streams", "spill", "through"])
def test_more_cells_replace_the_planes_and_nothing_else(rig, name):
    n = NEEDS[name]
    big = n._replace(words=n.words + 1)
    mine = list(range(n.planes + n.more)) + [H64] * n.f64
    log = grown(rig, n, big, mine)
    ops = [c[0] for c in log]
    # the planes, then the optional planes: each group's old blocks go before its first new one is asked for (peak memory)
    want = [FREE] * (n.planes + n.f64) + [MALLOC] * (n.planes + n.f64) + [FREE] * n.more + [MALLOC] * n.more
    assert ops == want
    assert [c[2] for c in log if c[0] == MALLOC] == [4 * big.words] * n.planes + [8 * big.words] * n.f64 + [4 * big.words] * n.more
    assert lib().dm_live_bytes() == sum(b for _, b in blocks(big))


@pytest.mark.parametrize("name", ["lakes", "spill"])
def test_more_members_replace_only_the_tables_and_the_counts(rig, name):
    n = NEEDS[name]
    big = n._replace(members=40, count_words=count_words(40) if n.count_words else 0)
    log = grown(rig, n, big, [D_TAB, H_TAB] + ([D_CNT, H_CNT] if n.count_words else []))
    pair = [MALLOC, HOST_MALLOC]
    assert [c[0] for c in log] == ([FREE, HOST_FREE, FREE, HOST_FREE] + pair + pair if n.count_words else [FREE, HOST_FREE] + pair)
    assert lib().dm_live_bytes() == sum(b for _, b in blocks(big))


@pytest.mark.parametrize("name", ["drainage", "through"])
def test_a_larger_result_replaces_only_the_result_region(rig, name):
    n = NEEDS[name]
    big = n._replace(res_bytes=n.res_bytes + 64)
    log = grown(rig, n, big, RESULT)
    assert [(c[0], c[2]) for c in log] == [(FREE, n.res_bytes), (HOST_FREE, n.res_bytes), (MALLOC, big.res_bytes), (HOST_MALLOC, big.res_bytes)]


def test_more_temporary_storage_replaces_only_that(rig):
    n = NEEDS["streams"]
    log = grown(rig, n, n._replace(temp_bytes=4096), [TEMP])
    assert [(c[0], c[2]) for c in log] == [(FREE, n.temp_bytes), (MALLOC, 4096)]


def test_the_basins_table_comes_with_the_second_reserve_of_a_spill_call(rig):
    """spill and through size their result region once the chain has counted the basins: the second reserve adds it and touches nothing."""
    log = grown(rig, NEEDS["spill_chain"], NEEDS["spill"], RESULT)
    assert [c[0] for c in log] == [MALLOC, HOST_MALLOC]


@pytest.mark.parametrize("name", list(NEEDS))
def test_a_need_that_fits_makes_no_allocator_call(rig, name):
    n = NEEDS[name]
    assert rig.as_reserve(n) == 0
    was, start = rig.as_blocks(), lib().dm_calls()
    smaller = n._replace(words=n.words - 5, temp_bytes=8, members=1, count_words=count_words(1) if n.count_words else 0, res_bytes=n.res_bytes // 2)
    for need in (n, smaller, n._replace(res_bytes=0)):
        assert rig.as_fits(need)
        assert rig.as_reserve(need) == 0
    assert lib().dm_calls() == start and rig.as_blocks() == was and rig.as_caps() == caps(n)


def test_the_optional_planes_are_absent_until_asked_for_and_then_added_without_touching_the_others(rig):
    """Drainage's P and AR: allocated only once an area is asked for."""
    n, area = NEEDS["drainage"], NEEDS["drainage_area"]
    assert rig.as_reserve(n) == 0
    assert rig.as_ptrs()[3] == 0 and rig.as_ptrs()[4] == 0 and rig.as_caps()[1] == 0
    assert not rig.as_fits(area)
    was, start = rig.as_blocks(), lib().dm_calls()
    assert rig.as_reserve(area) == 0
    now = rig.as_blocks()
    assert [k for k in range(18) if now[k] != was[k]] == [3, 4] and now[3] and now[4]
    assert [(c[0], c[2]) for c in calls(start)] == [(MALLOC, 4 * n.words)] * 2
    start = lib().dm_calls()
    assert rig.as_reserve(n) == 0 and rig.as_reserve(area) == 0, "a later call without the area keeps them, one with it finds them"
    assert lib().dm_calls() == start and rig.as_blocks() == now
