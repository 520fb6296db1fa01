"""The scratch of the five terrain analyses GROWS between calls on the same owner: an ensemble that gains members between rounds of
all five ensemble calls (cells, member table and records grow), and one map on which the calls follow each other in an order that
adds a group to a scratch that already holds the others (records after a count, the area planes after a call without them, the
basins' table after the chain). Every result is compared with the Python restatement of the loaded snapshot, the ensemble's also
with each member's own single-context call. The public API only."""
import ctypes as C

import pytest

import drainage_ref
import lakes_ref
import spill_ref
import streams_ref
import through_ref
from common import SNAP_CASES, load_cfg
from soilmachine_amd import capi
from soilmachine_amd.ensemble import Ensemble
from soilmachine_amd.machine import Layermap

pytestmark = pytest.mark.gpu

POOL = 1 << 15
THRESHOLD = 2
# the smallest shapes that still differ in every dimension of the need: one tile and one workgroup; several tiles, no tile size divides
# it; one column
MEMBERS = [("random_bernoulli20", (9, 7)), ("random_bernoulli20", (33, 47)), ("random_bernoulli20", (1, 70))]   # lakes, basins, segments in each
DRAIN_ALL = dict(receivers=True, labels=True, area=True)
STREAM_ALL = dict(order=True, segments=True, reach=True, heads=True)


def cfg64():
    return load_cfg(SNAP_CASES["default64"][0])


def restated(name, dims):
    """The snapshot of a drainage_ref input and what the five restatements make of it (computed once per input by the modules' case())."""
    s, base, sp, th = through_ref.case(name, dims)
    return s, {"lakes": lakes_ref.census(s), "drainage": base, "streams": streams_ref.case(name, dims, THRESHOLD)[2], "spill": sp, "through": th}


SAME = {"lakes": lakes_ref.assert_same_census, "drainage": drainage_ref.assert_same_drainage, "streams": streams_ref.assert_same_streams,
        "spill": spill_ref.assert_same_spill, "through": through_ref.assert_same_through}


def own_calls(m):
    """A map's five single-context calls, every plane asked for."""
    return {"lakes": m.lakes(labels=True), "drainage": m.drainage(**DRAIN_ALL), "streams": m.streams(THRESHOLD, **STREAM_ALL), "spill": m.spill(filled=True),
            "through": m.through(area=True, outlets=True)}


def test_an_ensemble_that_gains_members_between_rounds():
    want = []
    with Ensemble(0) as ens:
        for rnd, (name, dims) in enumerate(MEMBERS):
            s, w = restated(name, dims)
            want.append(w)
            ens.add(cfg64(), dims[0], dims[1], seed=0, pool=POOL, initialize=False).load(s)
            got = {"lakes": ens.lakes(), "drainage": ens.drainage(), "streams": ens.streams(THRESHOLD), "spill": ens.spill(), "through": ens.through()}
            for i, m in enumerate(ens.members):
                own = own_calls(m)
                for what, same in SAME.items():
                    tag = f"round {rnd}, member {i} {MEMBERS[i]}, {what}"
                    assert len(got[what]) == rnd + 1
                    same(own[what], want[i][what], f"{tag}: the member's own call against the restatement")
                    same((got[what][i], None), (own[what][0], None), f"{tag}: the ensemble call against the member's own")
                    same((got[what][i], None), (want[i][what][0], None), f"{tag}: the ensemble call against the restatement")
        counts = [[len(w[what][0]) for w in want] for what in SAME]
        print("records per member (lakes, basins, segments, spill, through):", counts)
        assert all(max(c) > c[0] > 0 for c in counts), "every analysis has records in the first round and more of them for a later member"


def test_one_map_whose_calls_add_to_a_scratch_that_holds_the_rest():
    name, dims = MEMBERS[1]
    s, want = restated(name, dims)
    m = Layermap(cfg64(), dims[0], dims[1], seed=0, pool=POOL, initialize=False)
    m.load(s)
    n = C.c_uint32()
    m._chk(m.L.smx_drainage(m.h, None, C.sizeof(capi.Basin), 0, C.byref(n), None, None, None))        # a count: no record yet
    assert n.value == len(want["drainage"][0])
    drainage_ref.assert_same_drainage((m.drainage(), None), want["drainage"], "records after the count")
    third = m.drainage(area=True)                                                                     # the area planes join
    assert set(third[1]) == {"area"}
    drainage_ref.assert_same_drainage(third, want["drainage"], "the area after a call without it")
    spill_ref.assert_same_spill((m.spill(), None), want["spill"], "spill")
    through_ref.assert_same_through(m.through(area=True, outlets=True), want["through"], "through with both planes")
    streams_ref.assert_same_streams(m.streams(THRESHOLD, segments=True), want["streams"], "streams with the segment plane")
    lakes_ref.assert_same_census(m.lakes(labels=True), want["lakes"], "lakes with the labels")
    last = m.drainage(**DRAIN_ALL)
    drainage_ref.assert_same_drainage(last, want["drainage"], "drainage again, every plane")
    drainage_ref.assert_same_drainage((last[0], {"area": last[1]["area"]}), third, "the last drainage call against the third")
    m.close()
