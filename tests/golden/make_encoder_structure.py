#!/usr/bin/env python3
"""Record the module tree of every encoder (fastposecnn_amd/lib/backbone.py) into tests/golden/encoder_structure.json.

Per encoder name: the ordered `name:class` lines of named_modules() and the ordered `key:shape` lines of state_dict(), each as a
count and a sha256 (the keys alone too: tests/golden/state_dict_keys_se_resnet50.txt is the same list for se_resnet50), and what
encoder_layout / encoder_groups / encoder_reduction answer.  CPU only, no library.  tests/test_encoder_structure.py calls collect()
and compares it with the file, value for value.

The file was recorded from commit 953ef84 ("State each encoder block kind once; split the planner out of net.hip"), the last one
with two separate encoder classes and three descriptor tables.  It is regenerated only by a change that MEANS to change a module
or parameter name, never by a refactoring.
    python tests/golden/make_encoder_structure.py
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "encoder_structure.json")

NAMES = ["resnet18", "resnet34", "resnet50", "resnet101", "resnet152", "resnext50_32x4d", "resnext101_32x4d", "resnext101_32x8d",
         "se_resnet50", "se_resnet101", "se_resnet152"]


def sha(lines):
    return hashlib.sha256("".join(line + "\n" for line in lines).encode()).hexdigest()


def structure(bb, name):
    import torch
    with torch.device("meta"):      # the tree and the shapes only: no parameter is allocated or initialised
        enc = bb.get_encoder(name)
    modules = ["%s:%s" % (n, type(m).__name__) for n, m in enc.named_modules()]
    state = ["%s:%s" % (k, "x".join(map(str, v.shape))) for k, v in enc.state_dict().items()]
    return {"name": name, "class": type(enc).__name__, "out_channels": list(enc.out_channels), "modules": len(modules),
            "modules_sha256": sha(modules), "state": len(state), "state_sha256": sha(state), "keys_sha256": sha(list(enc.state_dict())),
            "layout": list(bb.encoder_layout(name)), "groups": list(bb.encoder_groups(name)), "reduction": bb.encoder_reduction(name)}


def collect():
    from fastposecnn_amd.lib import backbone as bb
    return [structure(bb, name) for name in NAMES]


if __name__ == "__main__":
    sys.path.insert(0, REPO)
    with open(OUT, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(rec, separators=(",", ":")) for rec in collect()) + "\n]\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
