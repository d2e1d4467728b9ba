"""The backbone engine's contract per encoder block kind (csrc/net.hip), host arithmetic only: for BasicBlock, Bottleneck, ResNeXt
and SE-ResNet nets through every creation entry, the parameter table in its order, the workspace, every site's plan, the FLOP
counts, what the fpc_net_force_* switches return and change, and what every creation entry refuses equal the record in
tests/golden/encoder_contract.json (tests/golden/make_encoder_contract.py), value for value."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def contract():
    from fastposecnn_amd import build, _native
    build.build()
    spec = importlib.util.spec_from_file_location("make_encoder_contract", os.path.join(GOLDEN, "make_encoder_contract.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(os.path.join(GOLDEN, "encoder_contract.json")) as f:
        want = json.load(f)
    return gen, json.loads(json.dumps(gen.collect(_native.lib()))), want      # (through JSON: tuples -> lists, as in the file)


def test_the_record_covers_the_cases(contract):
    gen, _, want = contract
    cases = json.loads(json.dumps([[list(enc), classes, list(shape)] for enc, classes, shape in gen.NETS]))
    assert [n["net"] for n in want["nets"]] == cases
    assert len(cases) == 7 * 2 * 2
    for n in want["nets"]:
        assert [tuple(s["call"]) for s in n["switches"]] == gen.SWITCHES
        assert len(n["plans"]) == n["conv_count"] > 0 and n["param_count"] > 0
    assert [r["case"] for r in want["refusals"]] == [c[0] for c in gen.refusal_cases()]
    # the accepted call of every entry returns 0, every refusal does not
    for r in want["refusals"]:
        assert (r["rc"] == 0) == (r["case"] == "accepted"), r


def test_parameter_tables_workspace_and_plans(contract):
    _, got, want = contract
    for g, w in zip(got["nets"], want["nets"]):
        for key in ("net", "param_count", "param_sha256", "workspace_bytes", "conv_count", "plans", "flops"):
            assert g[key] == w[key], (w["net"], key)


def test_switches(contract):
    _, got, want = contract
    for g, w in zip(got["nets"], want["nets"]):
        for gs, ws in zip(g["switches"], w["switches"]):
            assert gs == ws, (w["net"], ws["call"])
    assert got["nets"] == want["nets"]


def test_refusals(contract):
    _, got, want = contract
    for g, w in zip(got["refusals"], want["refusals"]):
        assert g == w, w
    assert got["refusals"] == want["refusals"]
