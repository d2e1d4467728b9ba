"""The training front end's contract (fastposecnn_amd/lib/train_conv.py) on the MI355X: for every front end one accepted case and
one case per term of its gate, and for the three weight-gradient families the GradSink cases — whether the result is None, its
grad_fn type, shape and memory format, the counters each pass moves, what became of the sink — equal the record in
tests/golden/train_gate_contract.json (tests/golden/make_train_gate_contract.py), value for value.  One run of the case list, a
few seconds, shared by the tests."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FAMILIES = ("dense", "grouped", "stem", "up_add", "pool", "upsample", "groupnorm", "batchnorm", "se")


@pytest.fixture(scope="module")
def contract():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import fastposecnn_amd.lib  # noqa: F401
    spec = importlib.util.spec_from_file_location("make_train_gate_contract", os.path.join(GOLDEN, "make_train_gate_contract.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(os.path.join(GOLDEN, "train_gate_contract.json")) as f:
        want = json.load(f)
    return gen, json.loads(json.dumps(gen.collect())), want      # (through JSON, as in the file)


def test_the_record_covers_the_cases(contract):
    gen, _, want = contract
    cases = gen.cases()
    assert [r["case"] for r in want] == [name for name, _, _ in cases]
    assert len({name for name, _, _ in cases}) == len(cases)
    assert {family for _, family, _ in cases} == set(FAMILIES) == set(gen.FAMILIES)
    by_name = {r["case"]: r for r in want}
    # the first case of every family is accepted: it ran native (a counter moved, or a grad_fn of the project's own)
    for family in FAMILIES:
        first = by_name[next(name for name, f, _ in cases if f == family)]
        assert not first["none"] and first["grad_fn"].endswith("FnBackward"), first
    # every weight-gradient family has every sink case, and the recorded sink protocol is the documented one
    for family in ("dense", "grouped", "stem"):
        for kind in gen.SINKS:
            sink = by_name["%s sink %s" % (family, kind)]["sink"]
            taken = kind == "good" or (family == "dense" and kind == "offset")      # the dense site has no alignment check
            assert sink["written"] == (taken or kind == "written") and sink["weight_grad_is_none"] == taken, (family, kind, sink)
            assert sink["callback_ran"] == int(taken) and sink["entry_kept"] == (kind != "dead"), (family, kind, sink)
    assert not by_name["dense sink on the padded 7-channel head"]["sink"]["written"]


def test_every_case_equals_the_record(contract):
    _, got, want = contract
    for g, w in zip(got, want):
        assert g == w, w["case"]
    assert got == want
