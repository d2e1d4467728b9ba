"""The backbone engine's contract for the MobileNetV2 encoder, host arithmetic only: for fpc_net_create("mobilenet_v2") at every
recorded shape and class count, the parameter table in its order, the workspace, every site's plan, the FLOP counts, what the
fpc_net_force_* switches return and change, and what the creation entry refuses equal the record in
tests/golden/mobilenet_contract.json (tests/golden/make_mobilenet_contract.py), value for value."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def contract():
    from fastposecnn_amd import build, _native
    build.build()
    spec = importlib.util.spec_from_file_location("make_mobilenet_contract", os.path.join(GOLDEN, "make_mobilenet_contract.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(os.path.join(GOLDEN, "mobilenet_contract.json")) as f:
        want = json.load(f)
    return gen, json.loads(json.dumps(gen.collect(_native.lib()))), want      # (through JSON: tuples -> lists, as in the file)


def test_the_record_covers_the_cases(contract):
    gen, _, want = contract
    cases = json.loads(json.dumps([[list(enc), classes, list(shape)] for enc, classes, shape in gen.NETS]))
    assert [n["net"] for n in want["nets"]] == cases
    assert len(cases) == 2 * 2 and all(c[0] == ["name", "mobilenet_v2"] for c in cases)
    for n in want["nets"]:
        assert [tuple(s["call"]) for s in n["switches"]] == gen.SWITCHES
        # the sites are the decoders' alone, 4 x (4 laterals + 7 segmentation convolutions): the encoder's 52 ops are not sites
        assert len(n["plans"]) == n["conv_count"] == 44 and n["param_count"] > 260
    assert [(r["case"], r["name"], r["classes"], tuple(r["shape"])) for r in want["refusals"]] == gen.refusal_cases()
    for r in want["refusals"]:
        assert r["rc"] == (0 if r["case"] == "accepted" else -1), r


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
