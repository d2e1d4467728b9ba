"""K-loop, entry and exit stamps of the packed k_conv_wino_h3 launches on the two tile maps, alternating on one device
(a -DFPC_STAMP_WINO build; relu == 77 routes gn_part to the stamp buffer, as tools_dev/wino_stamps.py):
    python -c "from fastposecnn_amd import build; build.build(extra=['-DFPC_STAMP_WINO'])"
    python tools_dev/wino_xshare_stamps.py [B Cin H W Cout] ...      (default: the three shapes of profiles/wino_serial_ledger.md)
A shape the orientation rule transposes is requested as -13 (row-split) and -11 (x-shared), any other as -12 and -10; the row-split
map leads each of the ROUNDS pairs.  Per request: shader cycles per PAIR of K-steps, entry -> loop, loop end -> last store
acknowledged (means over the waves of all workgroups that ran, and over the rounds the spread of those means)."""
import ctypes, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from fastposecnn_amd import _native as nat
dev = torch.device("cuda:0"); L = nat.lib()
if not hasattr(L, "fpc_dbg_wino_diag"):
    sys.exit("wino_xshare_stamps.py needs a diagnostic build of the library (-DFPC_STAMP_WINO)")
ROUNDS, LAUNCHES = 5, 20
shapes = [(32, 64, 120, 160, 64), (32, 128, 60, 80, 128), (32, 256, 120, 160, 128)]
if len(sys.argv) > 5:
    v = [int(a) for a in sys.argv[1:]]
    shapes = [tuple(v[i:i + 5]) for i in range(0, len(v) - 4, 5)]
for B, Cin, H, W, Cout in shapes:
    o9 = (ctypes.c_int64 * 9)()
    nat.check(L.fpc_wino_orient_geometry(H, W, B, Cin, 0, 1, o9), "geometry")
    tr = bool(o9[0])
    codes = (-13, -11) if tr else (-12, -10)
    xs = bool(L.fpc_wino_xshare_rule(H if tr else W)) and (tr or o9[1] > 1)
    x = torch.randn((B, H, W, Cin), device=dev); w = torch.randn((Cout, Cin, 3, 3), device=dev) * 0.05
    out = torch.empty((B, H, W, Cout), device=dev)
    ws = torch.empty(L.fpc_conv2d_workspace_bytes(B, H, W, Cin, Cout, 3, 3), dtype=torch.uint8, device=dev)
    nblk = -(-((W + 1) // 2) // 8) * -(-((H + 1) // 2) // 8) * B * (Cout // 64)      # the plain grid: no packed grid is larger
    dbg = torch.zeros((nblk, 4, 8), dtype=torch.int64, device=dev)
    sb, sh, sw, sc = x.stride(); st = torch.cuda.current_stream().cuda_stream
    rows = {c: [] for c in codes}
    for _ in range(ROUNDS):
        for c in codes:
            dbg.zero_()
            for _ in range(LAUNCHES):
                nat.check(L.fpc_conv2d(x.data_ptr(), sb, sh, sw, sc, w.data_ptr(), None, None, None, None, out.data_ptr(), dbg.data_ptr(),
                                       B, H, W, Cin, Cout, 3, 3, 1, 1, 77, 0, 0, c, ws.data_ptr(), ws.numel(), st), "conv")
            torch.cuda.synchronize()
            d = dbg.cpu().double().reshape(-1, 8)
            d = d[d[:, 5] > 0]      # the waves of the workgroups this launch has
            rows[c].append((d.shape[0] // 4, (d[:, 3] / (d[:, 5] / 2)).mean().item(), d[:, 6].mean().item(), d[:, 7].mean().item(),
                            (d[:, 3] / d[:, 4] * 100.0).mean().item()))
    print(f"{B} x {Cin} x {H} x {W} -> {Cout}  ({'transposed' if tr else 'stored orientation'}, {'x-shared map taken' if xs else 'ROW-SPLIT ON BOTH REQUESTS'})")
    for c in codes:
        t = torch.tensor(rows[c])
        print(f"  request {c}: workgroups {int(t[0, 0])}  cycles per pair {t[:, 1].mean():8.1f} (rounds {t[:, 1].min():.1f} .. {t[:, 1].max():.1f})"
              f"  entry {t[:, 2].mean():7.0f} ({t[:, 2].min():.0f} .. {t[:, 2].max():.0f})  exit {t[:, 3].mean():7.0f} ({t[:, 3].min():.0f} .. {t[:, 3].max():.0f})"
              f"  clock {t[:, 4].mean():.0f} MHz")
    a, b = torch.tensor(rows[codes[0]]), torch.tensor(rows[codes[1]])
    print(f"  x-shared - row-split: pair {b[:, 1].mean() - a[:, 1].mean():+.1f} cycles ({(b[:, 1].mean() / a[:, 1].mean() - 1) * 100:+.2f} %), "
          f"entry {b[:, 2].mean() - a[:, 2].mean():+.0f}, exit {b[:, 3].mean() - a[:, 3].mean():+.0f}")
