#!/usr/bin/env python3
"""Record what the backbone engine builds for the MobileNetV2 encoder into tests/golden/mobilenet_contract.json.

Host arithmetic only, no device.  tests/golden/encoder_contract.json (make_encoder_contract.py) holds the encoders that are block
kinds; MobileNetV2 is the one that is not, and this record holds it the same way, with that script's own functions: per net the
parameter table (count and the sha256 of its ordered `name:numel` lines), the workspace, every site's plan, the FLOP counts, what
the fpc_net_force_* switches return and change, and what fpc_net_create("mobilenet_v2") refuses (the cases of
tests/test_mobilenet_v2_encoder.py::test_engine_refusals).  tests/test_mobilenet_contract.py calls collect() on the library under
test and compares it with the file, value for value.

The file was recorded from the library of commit e05a00d ("Sweep the MobileNetV2 1x1, depthwise and stem kernels' loop shapes"),
the last one whose engine built the MobileNetV2 encoder beside the block kinds' builder instead of as an encoder family of its own.
It is a record of behaviour: it is regenerated only by a change that MEANS to change a parameter name, a site, a plan or the
workspace, never by a refactoring of the engine.
    python tests/golden/make_mobilenet_contract.py
"""
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "mobilenet_contract.json")

_spec = importlib.util.spec_from_file_location("make_encoder_contract", os.path.join(HERE, "make_encoder_contract.py"))
_gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_gen)
net_contract, create, plans, flops = _gen.net_contract, _gen.create, _gen.plans, _gen.flops
SHAPES, CLASSES, SWITCHES = _gen.SHAPES, _gen.CLASSES, _gen.SWITCHES

ENCODER = ("name", "mobilenet_v2")
NETS = [(ENCODER, classes, shape) for shape in SHAPES for classes in CLASSES]


# what fpc_net_create refuses of this encoder, as (case, name, classes, (B, H, W)); the last entry is accepted
def refusal_cases():
    return [("H 481", "mobilenet_v2", 7, (2, 481, 640)), ("W 650", "mobilenet_v2", 7, (2, 480, 650)),
            ("classes 1", "mobilenet_v2", 1, (2, 480, 640)), ("classes 33", "mobilenet_v2", 33, (2, 480, 640)),
            ("B 0", "mobilenet_v2", 7, (0, 480, 640)),
            ("unknown name", "mobilenet_v3", 7, (1, 480, 640)), ("unknown name", "mobilenet_v2_", 7, (1, 480, 640)),
            ("unknown name", "mobilenet", 7, (1, 480, 640)),
            ("accepted", "mobilenet_v2", 32, (1, 32, 32))]


def refusals(L):
    out = []
    for case, name, classes, (B, H, W) in refusal_cases():
        rc, h = create(L, ("name", name), classes, B, H, W)
        if rc == 0:
            L.fpc_net_destroy(h)
        out.append({"case": case, "name": name, "classes": classes, "shape": [B, H, W], "rc": rc})
    return out


def collect(L):
    return {"nets": [net_contract(L, cfg) for cfg in NETS], "refusals": refusals(L)}


if __name__ == "__main__":
    sys.path.insert(0, REPO)
    from fastposecnn_amd import _native
    with open(OUT, "w") as f:
        json.dump(collect(_native.lib()), f, separators=(",", ":"))
        f.write("\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
