"""The squeeze-and-excitation block's training kernels alone, at the four stage shapes of a 640 x 480 frame:
python tools_dev/se_train_bench.py [out.json] [--batch 8] [--steps 20]

  * forward: fpc_se_gate_train (k_se_pool + k_se_excite<SAVE>) + fpc_se_scale_add_relu out of place;
  * backward: fpc_se_bwd (k_se_bwd_reduce + k_se_excite_bwd + k_se_param_grad + k_se_bwd_apply) with dres.

Beside each time stands a byte floor that is ARITHMETIC, not a measurement: the tensor passes the op cannot avoid — forward: read x and
res, write y (3 passes; the kernels read x a second time for the pool); backward: read gy, y, x for the reduction and gy, y for
the apply, write dx and dres (7 passes) — of B H W C x 4 bytes each, at the measured copy rate of DESIGN 4.4 (6.29 TB/s).

Every time is the median (min, max) of `steps` device-event intervals around one call each, the stream synchronised between calls,
after 3 warm-up calls.  Writes profiles/se_train_kernels.json."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from fastposecnn_amd import _native as nat
from se_bench import COPY_TBPS, REDUCTION, STAGES, arg, event_ms


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pos = [a for a in sys.argv[1:] if a.endswith(".json")]
    out_path = pos[0] if pos else os.path.join(root, "profiles", "se_train_kernels.json")
    B, steps = arg("--batch", 8), arg("--steps", 20)
    if not torch.cuda.is_available():
        raise SystemExit("se_train_bench.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    lib = nat.lib()
    rows, fwd_total, bwd_total = [], 0.0, 0.0
    for h, w, c, n in STAGES:
        cr = c // REDUCTION
        x, res, gy = (torch.randn((B, h, w, c), device=dev) for _ in range(3))
        y, dx, dres = (torch.empty((B, h, w, c), device=dev) for _ in range(3))
        w1, b1 = torch.randn((cr, c), device=dev) / c ** 0.5, torch.randn(cr, device=dev)
        w2, b2 = torch.randn((c, cr), device=dev) / cr ** 0.5, torch.randn(c, device=dev)
        gate, mean, hidden = torch.empty((B, c), device=dev), torch.empty((B, c), device=dev), torch.empty((B, cr), device=dev)
        dw1, db1, dw2, db2 = (torch.empty(s, device=dev) for s in ((cr, c), (cr,), (c, cr), (c,)))
        scratch = torch.empty(lib.fpc_se_scratch_floats(B, h, w, c), device=dev)
        scratch_b = torch.empty(lib.fpc_se_bwd_scratch_floats(B, h, w, c, REDUCTION), device=dev)
        p = lambda t: t.data_ptr()

        def fwd():
            nat.check(lib.fpc_se_gate_train(p(x), p(w1), p(b1), p(w2), p(b2), p(gate), p(mean), p(hidden), p(scratch), B, h, w, c,
                                            REDUCTION, nat.stream()), "fpc_se_gate_train")
            nat.check(lib.fpc_se_scale_add_relu(p(x), p(gate), p(res), p(y), B, h, w, c, nat.stream()), "fpc_se_scale_add_relu")

        def bwd():
            nat.check(lib.fpc_se_bwd(p(x), p(y), p(gy), p(gate), p(mean), p(hidden), p(w1), p(w2), p(dx), p(dres), p(dw1), p(db1),
                                     p(dw2), p(db2), p(scratch_b), B, h, w, c, REDUCTION, nat.stream()), "fpc_se_bwd")

        f_ms, b_ms = event_ms(fwd, steps), event_ms(bwd, steps)
        one = B * h * w * c * 4
        f_floor, b_floor = 3 * one / (COPY_TBPS * 1e12) * 1e3, 7 * one / (COPY_TBPS * 1e12) * 1e3
        rows.append({"stage": [h, w, c], "blocks": n, "slabs": lib.fpc_se_pool_slabs(h, w, c), "fwd_ms": f_ms, "bwd_ms": b_ms,
                     "tensor_bytes": one, "fwd_floor_ms_arithmetic": f_floor, "bwd_floor_ms_arithmetic": b_floor,
                     "fwd_share_of_copy_rate": f_floor / f_ms[0], "bwd_share_of_copy_rate": b_floor / b_ms[0]})
        fwd_total += n * f_ms[0]
        bwd_total += n * b_ms[0]
        del x, res, gy, y, dx, dres
        torch.cuda.empty_cache()
    out = {"device": torch.cuda.get_device_name(0), "batch": B, "frame": [480, 640], "steps": steps, "copy_rate_TBps": COPY_TBPS,
           "what": "ms per call: median (min, max) of device-event intervals, stream synchronised between calls, 3 warm-up calls; "
                   "floors are arithmetic (3 / 7 tensor passes at the copy rate)",
           "stages": rows, "fwd_ms_per_step_16_blocks": fwd_total, "bwd_ms_per_step_16_blocks": bwd_total}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
