"""The module tree of all eleven encoders (fastposecnn_amd/lib/backbone.py), CPU only: named_modules() and state_dict() in their
order, and what the three descriptor accessors answer, equal the record in tests/golden/encoder_structure.json
(tests/golden/make_encoder_structure.py), value for value."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("make_encoder_structure", os.path.join(GOLDEN, "make_encoder_structure.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def want():
    with open(os.path.join(GOLDEN, "encoder_structure.json")) as f:
        return json.load(f)


def test_the_record_covers_the_encoders(gen, want):
    assert [r["name"] for r in want] == gen.NAMES and len(gen.NAMES) == 11
    # the manifest of se_resnet50's keys, written from the published definition, is the same list
    keys = open(os.path.join(GOLDEN, "state_dict_keys_se_resnet50.txt")).read().split()
    se50 = next(r for r in want if r["name"] == "se_resnet50")
    assert se50["keys_sha256"] == gen.sha(keys) and se50["state"] == len(keys)


def test_every_encoder_equals_the_record(gen, want):
    got = json.loads(json.dumps(gen.collect()))
    for g, w in zip(got, want):
        for key in w:
            assert g[key] == w[key], (w["name"], key)
    assert got == want


def test_unknown_names_raise_key_error():
    from fastposecnn_amd.lib import backbone as bb
    for fn in (bb.encoder_layout, bb.encoder_groups, bb.encoder_reduction, bb.get_encoder, bb.ResNetEncoder, bb.SENetEncoder):
        with pytest.raises(KeyError):
            fn("se_resnext50_32x4d")
    with pytest.raises(KeyError):
        bb.ResNetEncoder("se_resnet50")
    with pytest.raises(KeyError):
        bb.SENetEncoder("resnet50")
