"""What the DeepLab head launches and computes on every ASPP route, against the commit before the route became one plan
(multishiftseg_amd/aspp_plan.py): tests/golden/aspp_head_traces_parent.json holds, per configuration of tools/gen_aspp_head_traces.py
(stage-2 and stage-1 steps at 2 x 3 x 592 x 600, eval forwards at 1 x 3 x 592 x 600, under the ASPP switches and on the split-bf16
route), that commit's full launch trace (kind, tag, FLOPs) and a SHA-256 of score, logit, loss, every gradient and every running
statistic. Each case runs one step here: the trace is equal row for row, every recorded hash is equal. (The parent's two runs of
every configuration agreed on every tensor: its `unstable` lists are empty, which the first test holds.)"""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_aspp_head_traces as gen  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "aspp_head_traces_parent.json")))


def test_the_case_table_is_the_generators():
    assert list(GOLDEN) == [c[0] for c in gen.CASES]
    for name, _mode, env, route in gen.CASES:
        assert GOLDEN[name]["env"] == env and GOLDEN[name]["route"] == route
        # score, logit, loss, the running statistics and every gradient were stable across the parent's two runs
        assert GOLDEN[name]["unstable"] == [], name
    assert sum(1 for k in GOLDEN["stage2"]["hashes"] if k.startswith("grad:")) == 18
    assert sum(1 for k in GOLDEN["stage1"]["hashes"] if k.startswith("grad:")) == 1


@pytest.fixture(scope="module")
def inputs():
    return gen.load_inputs()


@pytest.mark.parametrize("case", gen.CASES, ids=[c[0] for c in gen.CASES])
def test_head_launches_and_computes_what_the_parent_did(case, inputs):
    want = GOLDEN[case[0]]
    trace, res = gen.run_case(case, inputs)
    # (JSON round trip: the tags' tuples are lists there)
    trace = json.loads(json.dumps(trace))
    for i, (g, w) in enumerate(zip(trace, want["trace"])):
        assert g == w, f"launch {i}: {g} != parent's {w}"
    assert len(trace) == len(want["trace"])
    assert set(res) == set(want["hashes"]) | set(want["unstable"])
    bad = [k for k, v in want["hashes"].items() if res[k] != v]
    assert not bad, bad
