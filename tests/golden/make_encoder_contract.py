#!/usr/bin/env python3
"""Record what the backbone engine builds for every encoder block kind (csrc/net.hip) into tests/golden/encoder_contract.json.

Host arithmetic only, no device.  tests/golden/plan_contract.json holds BasicBlock and plain Bottleneck nets; this record adds the
ResNeXt and SE-ResNet kinds and every creation entry point, and per net the ORDER the engine creates things in: the parameter
table (count and the sha256 of its ordered `name:numel` lines), the workspace, every site's plan, the FLOP counts, what the
fpc_net_force_* switches return and change, and the refusals of every creation entry.  tests/test_encoder_contract.py calls
collect() on the library under test and compares it with the file, value for value.

The file was recorded from the library of commit 7fa7500 ("Run models of 9 to 32 classes on the native backbone engine"), the last
one whose net.hip wrote each block kind out beside the others.  It is a record of behaviour: it is regenerated only by a change
that MEANS to change a parameter name, a site, a plan or the workspace, never by a refactoring of the engine.
    python tests/golden/make_encoder_contract.py
"""
import ctypes
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "encoder_contract.json")

# (3,2,1,1): the smallest layout with a first block that has a downsample, blocks without one, and the Y[0], Y[1], Y[0] alternation
# of a stage whose blocks share their buffers
SMALL = (3, 2, 1, 1)
# how a net is created: ("name", encoder) | ("encoder", block, layers) | ("ex", block, layers, groups, width) | ("se", layers, reduction)
ENCODERS = [("name", "resnet18"), ("name", "resnet34"), ("name", "resnext50_32x4d"), ("name", "se_resnet50"),
            ("encoder", 4, SMALL), ("ex", 4, SMALL, 32, 8), ("se", SMALL, 8)]
SHAPES = [(2, 64, 96), (32, 480, 640)]
CLASSES = [8, 22]
NETS = [(enc, classes, shape) for enc in ENCODERS for shape in SHAPES for classes in CLASSES]
SWITCHES = [("fpc_net_force_winograd", 9), ("fpc_net_force_pointwise", 1), ("fpc_net_force_fold", 1), ("fpc_net_force_stem_pool", 1)]


def _layers(v):
    return None if v is None else (ctypes.c_int * 4)(*v)


def create(L, enc, classes, B, H, W, out="own"):
    """-> (rc, handle); out = None passes a null `out`"""
    h = ctypes.c_void_p()
    o = None if out is None else ctypes.byref(h)
    kind = enc[0]
    if kind == "name":
        rc = L.fpc_net_create(None if enc[1] is None else enc[1].encode(), classes, B, H, W, o)
    elif kind == "encoder":
        rc = L.fpc_net_create_encoder(enc[1], _layers(enc[2]), classes, B, H, W, o)
    elif kind == "ex":
        rc = L.fpc_net_create_encoder_ex(enc[1], _layers(enc[2]), enc[3], enc[4], classes, B, H, W, o)
    else:
        rc = L.fpc_net_create_encoder_se(_layers(enc[1]), enc[2], classes, B, H, W, o)
    return rc, h


def plans(L, h):
    out = []
    for i in range(L.fpc_net_conv_count(h)):
        o5 = (ctypes.c_int * 5)()
        assert L.fpc_net_conv_plan(h, i, o5) == 0
        out.append(list(o5))
    return out


def flops(L, h):
    o3 = (ctypes.c_double * 3)()
    assert L.fpc_net_flops(h, o3) == 0
    return [repr(float(v)) for v in o3]      # repr: the doubles round-trip exactly


def net_contract(L, cfg):
    enc, classes, (B, H, W) = cfg
    rc, h = create(L, enc, classes, B, H, W)
    assert rc == 0, (cfg, rc)
    count = L.fpc_net_param_count(h)
    table = "".join("%s:%d\n" % (L.fpc_net_param_name(h, i).decode(), L.fpc_net_param_numel(h, i)) for i in range(count))
    base = plans(L, h)
    rec = {"net": [list(enc), classes, [B, H, W]], "param_count": count, "param_sha256": hashlib.sha256(table.encode()).hexdigest(),
           "workspace_bytes": L.fpc_net_workspace_bytes(h), "conv_count": L.fpc_net_conv_count(h), "plans": base,
           "flops": flops(L, h), "switches": []}
    L.fpc_net_destroy(h)
    for fn, arg in SWITCHES:      # each on a fresh plan: the return value (a refusal code included) and the sites it changed
        rc, h = create(L, enc, classes, B, H, W)
        assert rc == 0
        r = getattr(L, fn)(h, arg)
        now = plans(L, h)
        rec["switches"].append({"call": [fn, arg], "rc": r, "changed": {str(i): p for i, (b, p) in enumerate(zip(base, now)) if p != b}})
        L.fpc_net_destroy(h)
    return rec


# what every creation entry refuses, as (case, encoder, classes, (B, H, W), out); the first entry of each group is accepted
def refusal_cases():
    ok = (8, (2, 64, 96), "own")
    cases = []
    for entry, null_arg in ((("name", "resnet18"), ("name", None)),
                            (("encoder", 1, SMALL), ("encoder", 1, None)),
                            (("ex", 4, SMALL, 32, 8), ("ex", 4, None, 32, 8)),
                            (("se", SMALL, 8), ("se", None, 8))):
        cases.append(("accepted", entry) + ok)
        cases.append(("null encoder or layers", null_arg) + ok)
        cases.append(("null out", entry, 8, (2, 64, 96), None))
        cases.append(("classes 1", entry, 1, (2, 64, 96), "own"))
        cases.append(("classes 33", entry, 33, (2, 64, 96), "own"))
        cases.append(("H 48", entry, 8, (2, 48, 96), "own"))
        if entry[0] != "name":
            li = 1 if entry[0] == "se" else 2
            for bad in (0, 65):
                e = list(entry)
                e[li] = (3, bad, 1, 1)
                cases.append(("layer count %d" % bad, tuple(e)) + ok)
    cases.append(("unknown name", ("name", "se_resnext50_32x4d")) + ok)
    cases.append(("block 2", ("encoder", 2, SMALL)) + ok)
    cases.append(("groups on BasicBlock", ("ex", 1, SMALL, 32, 4)) + ok)
    cases.append(("width 32 without groups", ("ex", 4, SMALL, 1, 32)) + ok)
    cases.append(("reduction 3", ("se", SMALL, 3)) + ok)
    return cases


def refusals(L):
    out = []
    for case, enc, classes, (B, H, W), o in refusal_cases():
        rc, h = create(L, enc, classes, B, H, W, o)
        if rc == 0 and o is not None:
            L.fpc_net_destroy(h)
        out.append({"case": case, "entry": [None if v is None else (list(v) if isinstance(v, tuple) else v) for v in enc],
                    "classes": classes, "shape": [B, H, W], "null_out": o is None, "rc": rc})
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
