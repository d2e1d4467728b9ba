"""ResNet34 B=32 640x480 engine autotuned as the streaming runtime's (tune mode 1, split level 3); prints each direct site's plan,
then runs frames on one stream (profiled from outside)."""
import sys, torch
from fastposecnn_amd import config, synth
import fastposecnn_amd.lib as L
from fastposecnn_amd.engine import NetEngine
hp = config.INFERENCE(); hp.RUNTIME_TIMING = False; hp.ENCODER = "resnet34"; hp.PERFORM_AGGREGATION = False
torch.manual_seed(0)
m = L.pose_regressor.MODELS['PoseRegressor'].load_from_ckpt(None, hp).eval().to("cuda:0")
dev = torch.device("cuda:0")
eng = NetEngine(m, 32, 480, 640, dev, autotune=True, tune_mode=1, graph=False, split_precision=3)
plans = eng.conv_plans()
for i, p in enumerate(plans):
    print("site", i, p)
x = torch.stack([synth.make_image(i) for i in range(32)]).to(dev)
with torch.no_grad():
    for _ in range(6):
        eng.forward(x)
torch.cuda.synchronize()
print("done")
