"""One-stream time of a ResNet34 B = 32, 480 x 640 forward with every 3x3 site on form 9 and the fold forced (no tuning), per setting
of fpc_net_set_fold_idle_row in alternating blocks of 30 forwards; from a tree whose library has no such switch, the one time under
the name 'parent'.  Run from the root of the tree to be measured; prints one JSON line of ms per forward.
    python tools_dev/fold_idle_row_time.py [rounds = 5]      (profiles/fold_idle_row_ledger.md)"""
import sys, os, json
sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import torch
from fastposecnn_amd import config, synth
import fastposecnn_amd.lib as L
from fastposecnn_amd.engine import NetEngine

dev = torch.device("cuda:0")
hp = config.INFERENCE(); hp.RUNTIME_TIMING = False; hp.ENCODER = "resnet34"; hp.PERFORM_AGGREGATION = False
torch.manual_seed(0)
m = L.pose_regressor.MODELS['PoseRegressor'].load_from_ckpt(None, hp).eval().to(dev)
eng = NetEngine(m, 32, 480, 640, dev, autotune=False, split_precision=3)
eng.force_winograd(9)
eng.force_fold(1)
assert any(p[2] == 5000 for p in eng.conv_plans())
x = torch.stack([synth.make_image(i) for i in range(32)]).to(dev)
has = hasattr(eng, "set_fold_idle_row")
settings = (1, 0) if has else (None,)
res = {s: [] for s in settings}


def block(n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.no_grad():
        a.record()
        for _ in range(n):
            eng.forward(x, want_logits=False)
        b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


block(10)
for rnd in range(int(sys.argv[1]) if len(sys.argv) > 1 else 5):
    for s in settings:
        if s is not None:
            eng.set_fold_idle_row(s)
        block(3)
        res[s].append(round(block(30), 4))
print(json.dumps({("idle_row_%d" % s if s is not None else "parent"): v for s, v in res.items()}))
