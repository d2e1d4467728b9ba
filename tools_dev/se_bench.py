"""se_resnet50 at 640 x 480, B = 32, one step in flight: python tools_dev/se_bench.py [out.json] [--batch 32] [--steps 10]

  * the native engine (PoseRegressor.forward's inference path: pure_model_forward + class compression in one C call);
  * the torch-module path on the same weights (HPARAM.USE_NATIVE_ENGINE = False): the only way the parent could run this encoder;
  * resnet50 on the engine beside them;
  * the three SE kernels (k_se_pool + k_se_excite through fpc_se_gate, k_se_scale_add_relu in place) at the four stage shapes,
    times the blocks per stage, against their bytes — the pool reads a block's output once, the scale pass reads it and the
    residual and writes it: 4 x B H W C x 4 bytes per block — at the measured copy rate of DESIGN 4.4 (6.29 TB/s).

Every time is the median of `steps` device-event intervals around one step each, the stream synchronised between steps, after
3 warm-up steps (the engine's autotuning pass and graph capture happen there).  Writes profiles/se_resnet.json."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import fastposecnn_amd.lib as L
from fastposecnn_amd import _native as nat
from fastposecnn_amd import config, synth

COPY_TBPS = 6.29
STAGES = [(120, 160, 256, 3), (60, 80, 512, 4), (30, 40, 1024, 6), (15, 20, 2048, 3)]      # (H, W, C, blocks) of one 640 x 480 frame
REDUCTION = 16


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def event_ms(fn, steps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out), min(out), max(out)


def model_for(encoder, dev):
    hp = config.INFERENCE()
    hp.RUNTIME_TIMING = False
    hp.ENCODER = encoder
    hp.PERFORM_AGGREGATION = False
    torch.manual_seed(0)
    return L.pose_regressor.MODELS['PoseRegressor'].load_from_ckpt(None, hp).to(dev).eval()


def se_bytes_per_frame():
    return sum(4 * h * w * c * 4 * n for h, w, c, n in STAGES)


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pos = [a for a in sys.argv[1:] if a.endswith(".json")]
    out_path = pos[0] if pos else os.path.join(root, "profiles", "se_resnet.json")
    B, steps = arg("--batch", 32), arg("--steps", 10)
    if not torch.cuda.is_available():
        raise SystemExit("se_bench.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    lib = nat.lib()
    x = torch.stack([synth.make_image(i) for i in range(B)]).to(dev)
    res = {"device": torch.cuda.get_device_name(0), "batch": B, "frame": [480, 640], "steps": steps,
           "what": "ms per step of B frames: median (min, max) of device-event intervals, stream synchronised between steps, 3 warm-up steps"}
    side = torch.cuda.Stream(device=dev)          # (the engine replays its recorded graph on a stream of its own only)
    with torch.cuda.stream(side), torch.no_grad():
        for enc in ("se_resnet50", "resnet50"):
            m = model_for(enc, dev)
            res[enc + "_engine_ms"] = event_ms(lambda: m(x), steps)
            assert m._engines, "the native engine did not run"
            eng = next(iter(m._engines.values()))
            res[enc + "_graph_recorded"] = eng.graph_recorded()
            res[enc + "_plans"] = [p[2] for p in eng.conv_plans()]
            if enc == "se_resnet50":
                m.HPARAM.USE_NATIVE_ENGINE = False
                res[enc + "_torch_modules_ms"] = event_ms(lambda: m(x), steps)
            del m, eng
            torch.cuda.empty_cache()
        # the SE kernels alone, one stage at a time
        rows, total_ms = [], 0.0
        for h, w, c, n in STAGES:
            t = torch.randn((B, h, w, c), device=dev)
            r = torch.randn((B, h, w, c), device=dev)
            cr = c // REDUCTION
            w1, b1 = torch.randn((cr, c), device=dev) / c ** 0.5, torch.randn(cr, device=dev)
            w2, b2 = torch.randn((c, cr), device=dev) / cr ** 0.5, torch.randn(c, device=dev)
            gate = torch.empty((B, c), device=dev)
            scratch = torch.empty(lib.fpc_se_scratch_floats(B, h, w, c), device=dev)

            def gate_fn():
                nat.check(lib.fpc_se_gate(t.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), gate.data_ptr(),
                                          scratch.data_ptr(), B, h, w, c, REDUCTION, nat.stream()), "fpc_se_gate")

            def scale_fn():
                nat.check(lib.fpc_se_scale_add_relu(t.data_ptr(), gate.data_ptr(), r.data_ptr(), t.data_ptr(), B, h, w, c, nat.stream()),
                          "fpc_se_scale_add_relu")

            g_ms, s_ms = event_ms(gate_fn, steps), event_ms(scale_fn, steps)
            nbytes = 4 * B * h * w * c * 4
            floor_ms = nbytes / (COPY_TBPS * 1e12) * 1e3
            rows.append({"stage": [h, w, c], "blocks": n, "slabs": lib.fpc_se_pool_slabs(h, w, c), "gate_ms": g_ms, "scale_ms": s_ms,
                         "bytes_per_block": nbytes, "floor_ms_per_block": floor_ms,
                         "share_of_copy_rate": floor_ms / (g_ms[0] + s_ms[0])})
            total_ms += n * (g_ms[0] + s_ms[0])
            del t, r
            torch.cuda.empty_cache()
        res["se_kernels"] = rows
        res["se_kernels_ms_per_step"] = total_ms
        res["se_bytes_per_frame"] = se_bytes_per_frame()
        res["se_floor_ms_per_step"] = B * se_bytes_per_frame() / (COPY_TBPS * 1e12) * 1e3
        res["se_share_of_copy_rate"] = res["se_floor_ms_per_step"] / total_ms
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if not k.endswith("_plans")}))


if __name__ == "__main__":
    main()
