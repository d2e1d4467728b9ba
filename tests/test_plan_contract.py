"""The convolution planner's contract (csrc/net.hip), host arithmetic only: every plan code fpc_conv2d_plan and
fpc_conv2d_workspace_bytes_for accept, the workspace they ask for, and the plans, workspace and FLOP counts of whole networks
before and after the fpc_net_force_* switches equal the record in tests/golden/plan_contract.json
(tests/golden/make_plan_contract.py), value for value."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def contract():
    from fastposecnn_amd import build, _native
    build.build()
    spec = importlib.util.spec_from_file_location("make_plan_contract", os.path.join(GOLDEN, "make_plan_contract.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(os.path.join(GOLDEN, "plan_contract.json")) as f:
        want = json.load(f)
    return gen, json.loads(json.dumps(gen.collect(_native.lib()))), want      # (through JSON: tuples -> lists, as in the file)


def test_the_record_covers_the_cases(contract):
    gen, _, want = contract
    assert [tuple(s["shape"]) for s in want["conv2d"]] == gen.SHAPES
    for s in want["conv2d"]:
        assert [tuple(r[:3]) for r in s["rows"]] == [(bm, bn, rq) for (bm, bn) in gen.TILES for rq in gen.REQUESTS]
    assert [tuple(n["net"][:2]) + (tuple(n["net"][2]),) + tuple(n["net"][3:]) for n in want["nets"]] == gen.NETS
    for n in want["nets"]:
        assert [f["form"] for f in n["force_winograd"]] == list(range(1, 10))
        assert len(n["plans"]) == n["conv_count"] > 0


def test_conv2d_requests(contract):
    _, got, want = contract
    for g, w in zip(got["conv2d"], want["conv2d"]):
        assert g["workspace_bytes"] == w["workspace_bytes"], w["shape"]
        for gr, wr in zip(g["rows"], w["rows"]):
            assert gr == wr, (w["shape"], "bm, bn, request, rc, out4, bytes_for", gr, wr)
    assert got["conv2d"] == want["conv2d"]


def test_network_plans_and_switches(contract):
    _, got, want = contract
    for g, w in zip(got["nets"], want["nets"]):
        for key in ("net", "workspace_bytes", "conv_count", "plans", "flops"):
            assert g[key] == w[key], (w["net"], key)
        for gf, wf in zip(g["force_winograd"], w["force_winograd"]):
            assert gf == wf, (w["net"], "force_winograd", wf["form"])
        for gs, ws in zip(g["steps"], w["steps"]):
            for a, b in zip(gs, ws):
                assert a == b, (w["net"], b["call"])
    assert got["nets"] == want["nets"]
