#!/usr/bin/env python3
"""Record what the convolution planner reports and accepts (csrc/net.hip) into tests/golden/plan_contract.json.

Host arithmetic only, no device: the integer plan codes fpc_conv2d_plan / fpc_conv2d_workspace_bytes_for decode, the workspace a
request needs, and the plans, workspace and FLOP counts of whole networks before and after the fpc_net_force_* switches.
tests/test_plan_contract.py calls collect() on the library under test and compares it with the file, value for value.  The file is
a record of behaviour: it is regenerated only by a change that MEANS to change a plan code, an image layout or a heuristic plan,
never by a refactoring of the planner.      python tests/golden/make_plan_contract.py
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "plan_contract.json")

REQUESTS = [0, 1, 2, 4, 102, 104, 1001, 1004, 1102, 2001, 2004, 3000, 3100, 4000, 4001, 6001, 6004, 6102, 7001, 7002] + \
           list(range(-1, -11, -1))
TILES = [(0, 0), (128, 64), (64, 128)]
# (B, Ho, Wo, Cin, Cout, k): packs / one frame, Cout % 128 != 0 / Cin % 16 != 0 / pointwise, lateral / stem
SHAPES = [(2, 30, 40, 128, 128, 3), (1, 15, 20, 64, 64, 3), (2, 12, 14, 24, 64, 3), (3, 60, 80, 64, 256, 1), (2, 48, 64, 4, 64, 7)]
# (name, block, layers, B, H, W), 8 classes
NETS = [("resnet18", 1, (2, 2, 2, 2), 2, 96, 128), ("resnet18", 1, (2, 2, 2, 2), 32, 480, 640),
        ("resnet34", 1, (3, 4, 6, 3), 2, 96, 128), ("resnet34", 1, (3, 4, 6, 3), 32, 480, 640),
        ("bottleneck3463", 4, (3, 4, 6, 3), 2, 96, 128)]
CLASSES = 8


def conv2d_contract(L):
    out = []
    for (B, Ho, Wo, Cin, Cout, k) in SHAPES:
        rows = []
        for (bm, bn) in TILES:
            for rq in REQUESTS:
                o4 = (ctypes.c_int * 4)(-12345, -12345, -12345, -12345)
                rc = L.fpc_conv2d_plan(B, Ho, Wo, Cin, Cout, k, k, bm, bn, rq, o4)
                rows.append([bm, bn, rq, rc, list(o4), L.fpc_conv2d_workspace_bytes_for(B, Ho, Wo, Cin, Cout, k, k, bm, bn, rq)])
        out.append({"shape": [B, Ho, Wo, Cin, Cout, k], "workspace_bytes": L.fpc_conv2d_workspace_bytes(B, Ho, Wo, Cin, Cout, k, k),
                    "rows": rows})
    return out


class Net:
    def __init__(self, L, name, block, layers, B, H, W):
        self.L, self.h = L, ctypes.c_void_p()
        if block == 1:
            rc = L.fpc_net_create(name.encode(), CLASSES, B, H, W, ctypes.byref(self.h))
        else:
            rc = L.fpc_net_create_encoder(block, (ctypes.c_int * 4)(*layers), CLASSES, B, H, W, ctypes.byref(self.h))
        assert rc == 0, (name, rc)

    def close(self):
        self.L.fpc_net_destroy(self.h)

    def plans(self):
        out = []
        for i in range(self.L.fpc_net_conv_count(self.h)):
            o5 = (ctypes.c_int * 5)()
            assert self.L.fpc_net_conv_plan(self.h, i, o5) == 0
            out.append(list(o5))
        return out

    def flops(self):
        o3 = (ctypes.c_double * 3)()
        assert self.L.fpc_net_flops(self.h, o3) == 0
        return [repr(float(v)) for v in o3]      # repr: the doubles round-trip exactly


def changed(base, now):
    """the sites whose out5 differs from `base`, as {site: out5} (every other site must report what `base` does)"""
    assert len(base) == len(now)
    return {str(i): p for i, (b, p) in enumerate(zip(base, now)) if p != b}


def net_contract(L, cfg):
    def fresh():
        return Net(L, *cfg)

    n = fresh()
    base = n.plans()
    rec = {"net": [cfg[0], cfg[1], list(cfg[2]), cfg[3], cfg[4], cfg[5]], "workspace_bytes": L.fpc_net_workspace_bytes(n.h),
           "conv_count": L.fpc_net_conv_count(n.h), "plans": base, "flops": n.flops(), "force_winograd": [], "steps": []}
    n.close()
    for form in range(1, 10):
        n = fresh()
        rc = L.fpc_net_force_winograd(n.h, form)
        rec["force_winograd"].append({"form": form, "rc": rc, "changed": changed(base, n.plans()), "flops": n.flops()})
        n.close()
    # sequences of switches on one plan each: (function, argument) -> return value and the plans after it
    for seq in ([("fpc_net_force_pointwise", 1), ("fpc_net_force_pointwise", 0)],
                [("fpc_net_force_fold", 1), ("fpc_net_force_fold", 0)],
                [("fpc_net_force_fold", 1), ("fpc_net_force_winograd", 9), ("fpc_net_force_winograd", 8)],
                [("fpc_net_force_winograd", 0), ("fpc_net_force_winograd", 10), ("fpc_net_force_direct_h3", 1), ("fpc_net_force_stem_pool", 1)]):
        n = fresh()
        steps = []
        for fn, arg in seq:
            rc = getattr(L, fn)(n.h, arg)
            steps.append({"call": [fn, arg], "rc": rc, "changed": changed(base, n.plans())})
        rec["steps"].append(steps)
        n.close()
    return rec


def collect(L):
    return {"conv2d": conv2d_contract(L), "nets": [net_contract(L, cfg) for cfg in NETS]}


if __name__ == "__main__":
    sys.path.insert(0, REPO)
    from fastposecnn_amd import _native
    with open(OUT, "w") as f:
        json.dump(collect(_native.lib()), f, separators=(",", ":"))
        f.write("\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
