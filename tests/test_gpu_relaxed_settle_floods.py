"""Settle and floods of a dense relaxed water epoch as ONE dataflow launch (k_relax_settle_floods, smx_set_relax_settle mode 2): against the same
headers run by host threads -- full state after every tick and the counters. The per-phase launches run down to the last particle
(set_relax_launch(0, 0)), so every epoch of every generation goes through the launch under test. Scenes, host-thread states and the way a run is
driven are those of tests/test_gpu_relaxed_settle.py (one host run per scene in the session, shared): standing water (floods queue on lake shores next
to freshly flagged cells, nested generations in between), four soils with wind in the same tick (wind epochs have no floods: k_relax_settle), and a
non-square map (the clamps of the gate's widened rectangle at the map's edges). No test drives a wait to its spin budget."""
import pytest

from soilmachine_amd.snapshot import compare
from test_gpu_relaxed import KEYS
from test_gpu_relaxed_settle import SCENES, device, host_states

pytestmark = pytest.mark.gpu

_thin = {}   # scene -> the flood-flow figures of an uncapped run (one flood per wavefront on these maps)


def run_against_host(scene, max_waves=0):
    """mode 2 on `scene` -> (the settle getter's figures, the flood-flow getter's figures), after the last tick"""
    snaps, ch = host_states(scene)
    sm, ticks = device(scene, 2, max_waves)
    for t in range(ticks):
        sm.tick(1, sync=True)
        bad = compare(sm.map.snapshot(), snaps[t])
        assert not bad, f"{scene} mode 2 (max_waves {max_waves}) tick {t}: {bad}"
    settle, flow = sm.map.relax_settle_stats(), sm.map.relax_flood_flow_stats()
    cd = sm.map.counters()
    assert {k: cd[k] for k in KEYS} == {k: ch[k] for k in KEYS}
    assert sm.map.batch_stats()["children_lost"] == 0
    sm.map.close()
    print("[settle+floods]", scene, max_waves, settle, flow)
    if max_waves == 0:
        _thin.setdefault(scene, flow)
    return settle, flow


@pytest.mark.parametrize("scene", list(SCENES))
def test_the_joined_launch_equals_host_threads(scene):
    settle, flow = run_against_host(scene)
    assert settle["epochs_split"] == 0, (settle, flow)                                 # nothing fell back silently
    assert flow["epochs_joined"] > 0 and settle["epochs_fused"] >= flow["epochs_joined"], (settle, flow)   # (joined epochs are fused epochs, and more)
    if scene == "standing-water":                                                      # the scene reaches the gate: floods act next to cells flagged in their epoch
        assert flow["floods_acted"] > 0 and flow["floods_gated"] > 0, flow
    assert flow["floods_gated"] <= flow["floods_acted"], flow
    _, again = run_against_host(scene)
    assert again == flow                                                               # acted and gated are functions of the input, not of timing


def test_thick_wavefronts_equal_host_threads():
    """the setter's cap leaves ceil(nslots / 64) flood wavefronts beside as many settle wavefronts in the top-level generation: several floods per wavefront
    (gated one after the other) with a ragged last one, settle at 64 cells per wavefront"""
    nwater = SCENES["standing-water"][3]
    settle, flow = run_against_host("standing-water", max_waves=2 * ((nwater + 63) // 64))
    assert flow["epochs_joined"] > 0 and flow["floods_acted"] > 0 and flow["floods_gated"] > 0, (settle, flow)
    assert settle["epochs_split"] == 0, settle
    thin = _thin.get("standing-water") or run_against_host("standing-water")[1]
    assert flow == thin, (flow, thin)                                                  # which wavefront holds a flood has no influence on what is counted


def test_a_grid_that_is_not_resident_takes_the_separate_launches():
    """mode 2 on a context that may count on ONE resident wavefront: no room for a settle and a flood wavefront together, so no epoch is joined; mode 1's
    plan then fails too wherever the worst case exceeds 64 flagged cells, and those epochs take filter + colour lists -- the fall-back chain, on a small map"""
    settle, flow = run_against_host("standing-water", max_waves=1)
    assert flow["epochs_joined"] == 0 and flow["floods_acted"] == 0 and flow["floods_gated"] == 0, flow
    assert settle["epochs_split"] > 0, settle
