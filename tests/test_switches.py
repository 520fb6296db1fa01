"""The library's run-time switches (the SMX_* environment variables of csrc/soilmx.hip) as ONE table behind smx_switches: the
table, the call sites in the source and README.md say the same, and a process reports what it read. No GPU needed (the GPU
matrix over the table is tests/test_gpu_switches.py)."""
import json
import os
import re
import subprocess
import sys

from common import ROOT
from soilmachine_amd import capi

CSRC = os.path.join(ROOT, "soilmachine_amd", "csrc")
CLASSES = {"neutral", "changes_results", "diagnostic"}


def test_table_is_well_formed():
    t = capi.switches()
    assert len(t) >= 30
    for name, e in t.items():
        assert re.fullmatch(r"SMX_[A-Z0-9_]+", name), name
        assert e["class"] in CLASSES, (name, e)
    assert {k for k, e in t.items() if e["default"] == "-"} == {"SMX_BATCH_SCHED", "SMX_BATCH_SCHED_WIND", "SMX_BATCH_SCHED_TAIL",
                                                               "SMX_BATCH_SCHED_TAIL_WIND", "SMX_RELAX_WIND_MIN"}
    # what the restated schedules (oracle/, tests/hostsim) are written for is part of a schedule, not a launch shape
    assert t["SMX_BATCH_CHUNK"]["class"] == "changes_results" and t["SMX_BATCH_CHUNK"]["default"] == "32"
    assert t["SMX_RELAX_CHUNK_KIDS"]["class"] == "neutral"
    assert t["SMX_SPIN_BUDGET"]["class"] == t["SMX_GRID_POLL_NAPS"]["class"] == "diagnostic"


def test_every_switch_the_source_reads_is_in_the_table_and_the_reverse():
    read, text = set(), ""
    for f in sorted(os.listdir(CSRC)):
        text = open(os.path.join(CSRC, f)).read()
        read |= set(re.findall(r"\benv_(?:int|flag|str)\(\s*\"(SMX_[A-Z0-9_]+)\"", text))
        # nothing but the table's own loop asks the environment directly
        assert len(re.findall(r"\bgetenv\s*\(", text)) == (1 if f == "soilmx.hip" else 0), f
    assert read == set(capi.switches()), (sorted(read - set(capi.switches())), sorted(set(capi.switches()) - read))


def readme_blocks():
    text = open(os.path.join(ROOT, "README.md")).read()
    a = text.index("Run-time switches (")
    para = text[a:text.index("\n\n", a)] if "\n\n" in text[a:] else text[a:]
    marks = [("neutral", "**Results bit-identical**"), ("diagnostic", "**Diagnostics**"), ("changes_results", "**These CHANGE results**"),
             (None, "Outside the library's table:")]
    pos = [para.index(m) for _, m in marks]
    assert pos == sorted(pos)
    return {cls: para[p:q] for (cls, _), p, q in zip(marks, pos, pos[1:] + [len(para)])}


def test_readme_lists_every_switch_under_its_class():
    blocks, table = readme_blocks(), capi.switches()
    assert "bit-identical" in blocks["neutral"].split(":")[0] and "bit-identical" in blocks["diagnostic"].split(":")[0]
    assert "CHANGE results" in blocks["changes_results"].split(":")[0]
    names = {cls: set(re.findall(r"`(SMX_[A-Z0-9_]+)(?:=[^`]*)?`", b)) for cls, b in blocks.items()}
    for cls in CLASSES:
        want = {k for k, e in table.items() if e["class"] == cls}
        assert names[cls] == want, (cls, sorted(want - names[cls]), sorted(names[cls] - want))
    assert not names[None] & set(table)


def test_a_process_reports_what_it_read():
    code = "import json; from soilmachine_amd import capi; print(json.dumps(capi.switches()))"
    env = {k: v for k, v in os.environ.items() if not k.startswith("SMX_")}
    env.update(SMX_BATCH_WAVES="3", SMX_BATCH_SCHED_WIND="2,1,8", SMX_BATCH_WAVE="7", PYTHONPATH=ROOT)   # (the third is nobody's name)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-800:]
    got, here = json.loads(r.stdout), capi.switches()
    assert set(got) == set(here) and "SMX_BATCH_WAVE" not in got
    assert got["SMX_BATCH_WAVES"] == {"value": "3", "default": "256", "class": "neutral"}
    assert got["SMX_BATCH_SCHED_WIND"] == {"value": "2,1,8", "default": "-", "class": "changes_results"}
    for k, e in got.items():
        assert (e["default"], e["class"]) == (here[k]["default"], here[k]["class"])
        if k not in ("SMX_BATCH_WAVES", "SMX_BATCH_SCHED_WIND"):
            assert e["value"] == e["default"], (k, e)
