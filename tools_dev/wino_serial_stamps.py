"""The serial path of k_conv_wino_h3 around its K loop, phase by phase, from a -DFPC_STAMP_WINO build (wino_stamps.py's hook: relu == 77
routes gn_part to the stamp buffer; FPC_WINO_SERIAL=1 makes the plain launch write a second, 16-word record per wave behind the
8-word ones).  One line per shape, shader-clock ticks, mean over waves and workgroups (the ledger of profiles/wino_serial_ledger.md):
    python tools_dev/wino_serial_stamps.py B Cin H W Cout
entry, cumulative since the kernel's first instruction: decode | weights requested | staging plan | ring zeroed | all issued, accumulators
zeroed | first operands landed | barrier | K loop begins;  exit, cumulative since the K loop's end: first barrier | Z stores | barrier |
reads + epilogue + last store issued | record reduction | last store acknowledged."""
import os, sys
os.environ["FPC_WINO_SERIAL"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from fastposecnn_amd import _native as nat
dev = torch.device("cuda:0"); L = nat.lib()
if not hasattr(L, "fpc_dbg_wino_diag"):
    sys.exit("wino_serial_stamps.py needs a diagnostic build of the library (build.build(extra=['-DFPC_STAMP_WINO']))")
B, Cin, Hi, Wi, Cout = (int(v) for v in sys.argv[1:6])
x = torch.randn((B, Hi, Wi, Cin), device=dev); w = torch.randn((Cout, Cin, 3, 3), device=dev) * 0.05
out = torch.empty((B, Hi, Wi, Cout), device=dev)
ws = torch.empty(L.fpc_conv2d_workspace_bytes(B, Hi, Wi, Cin, Cout, 3, 3), dtype=torch.uint8, device=dev)
nblk = -(-(-(-Wi // 2)) // 8) * -(-(-(-Hi // 2)) // 8) * B * (Cout // 64)
dbg = torch.zeros((nblk * 4 * (8 + 16),), dtype=torch.int64, device=dev)
sb, sh, sw, sc = x.stride(); st = torch.cuda.current_stream().cuda_stream
for _ in range(50):
    nat.check(L.fpc_conv2d(x.data_ptr(), sb, sh, sw, sc, w.data_ptr(), None, None, None, None, out.data_ptr(), dbg.data_ptr(), B, Hi, Wi,
                           Cin, Cout, 3, 3, 1, 1, 77, 0, 0, -9, ws.data_ptr(), ws.numel(), st), "conv")
torch.cuda.synchronize()
d = dbg.cpu().double()
a = d[:nblk * 32].view(nblk, 4, 8); f = d[nblk * 32:].view(nblk, 4, 16)
assert (f[:, :, 4] > 0).all(), "no serial-path records: is this the plain -9 launch of a diagnostic build?"
m = lambda t: t.mean().item()
issued = a[:, :, 0]; landed = issued + a[:, :, 1]; synced = landed + a[:, :, 2]
print("shape %d x %d x %d x %d -> %d: clock %.0f MHz, K loop %.0f ticks" % (B, Cin, Hi, Wi, Cout, m(a[:, :, 3] / a[:, :, 4] * 100.0), m(a[:, :, 3])))
print("  entry: decode %.0f | weights requested %.0f | plan %.0f | ring zeroed %.0f | issued, acc zeroed %.0f (%.0f) | landed %.0f | barrier %.0f | loop %.0f"
      % (m(f[:, :, 0]), m(f[:, :, 1]), m(f[:, :, 2]), m(f[:, :, 3]), m(f[:, :, 4]), m(issued), m(landed), m(synced), m(a[:, :, 6])))
print("  exit:  barrier %.0f | Z stores %.0f | barrier %.0f | reads, epilogue, last store %.0f | records %.0f | acknowledged %.0f"
      % (m(f[:, :, 8]), m(f[:, :, 9]), m(f[:, :, 10]), m(f[:, :, 11]), m(f[:, :, 12]), m(a[:, :, 7])))
