"""k_conv_wino_h3 on the four shapes of tools_dev/wino_orient_ab.py (requests -9 and -11 alternating), for comparing TWO BUILDS of the
library: each build lives in its own checkout and runs in its own process,
    rocprofv3 --kernel-trace --output-format csv -d OUT/<tag><k> -- python tools_dev/wino_serial_site_ab.py run <checkout>
with the builds alternating (parent, branch, parent, branch: N launches per shape, request and process), and
    python tools_dev/wino_serial_site_ab.py parse parent=<csv>[,<csv>..] branch=<csv>[,<csv>..]
prints per shape and request the median of each build's launches (all its traces together) and the difference."""
import csv, os, statistics, sys

SHAPES = [("layer1", 32, 64, 120, 160, 64), ("s2.0-unfolded", 32, 256, 120, 160, 128), ("layer2", 32, 128, 60, 80, 128), ("s3.0", 32, 256, 60, 80, 128)]
WARM, N = 3, 10


def run(root):
    sys.path.insert(0, os.path.abspath(root))
    import torch
    from fastposecnn_amd import _native as nat
    dev = torch.device("cuda:0")
    L = nat.lib()
    for name, B, Cin, H, W, Cout in SHAPES:
        g = torch.Generator().manual_seed(Cin + H)
        x = torch.randn((B, H, W, Cin), generator=g).to(dev)
        w = (torch.randn((Cout, Cin, 3, 3), generator=g) * 0.05).to(dev)
        out = torch.empty((B, H, W, Cout), device=dev)
        ws = torch.empty(L.fpc_conv2d_workspace_bytes(B, H, W, Cin, Cout, 3, 3), dtype=torch.uint8, device=dev)
        sb, sh, sw, sc = x.stride()
        st = torch.cuda.current_stream().cuda_stream
        for i in range(WARM + N):
            for ns in (-9, -11):
                nat.check(L.fpc_conv2d(x.data_ptr(), sb, sh, sw, sc, w.data_ptr(), None, None, None, None, out.data_ptr(), None, B, H, W, Cin,
                                       Cout, 3, 3, 1, 1, 0, 0, 0, ns, ws.data_ptr(), ws.numel(), st), "conv")
            torch.cuda.synchronize()
    print("done")


def times(path):
    """{(shape index, request index): [us]} of one trace"""
    rows = [r for r in csv.DictReader(open(path)) if "k_conv_wino_h3" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per = 2 * (WARM + N)
    assert len(rows) == per * len(SHAPES), (path, len(rows))
    out = {}
    for si in range(len(SHAPES)):
        blk = rows[si * per:(si + 1) * per]
        for v in (0, 1):
            out[(si, v)] = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in blk[2 * WARM + v::2]]
    return out


def parse(args):
    sides = {}
    for a in args:
        tag, paths = a.split("=")
        acc = {}
        for p in paths.split(","):
            for k, v in times(p).items():
                acc.setdefault(k, []).extend(v)
        sides[tag] = acc
    (ta, A), (tb, Bv) = list(sides.items())
    for si, s in enumerate(SHAPES):
        for v, rq in enumerate((-9, -11)):
            a, b = A[(si, v)], Bv[(si, v)]
            ma, mb = statistics.median(a), statistics.median(b)
            print("%-14s %dx%dx%dx%d->%d request %3d  %s %8.1f us (%.1f-%.1f, n=%d) | %s %8.1f us (%.1f-%.1f, n=%d) | %+.2f %%"
                  % (s[0], s[1], s[2], s[3], s[4], s[5], rq, ta, ma, min(a), max(a), len(a), tb, mb, min(b), max(b), len(b), 100 * (mb / ma - 1)))


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    else:
        parse(sys.argv[2:])
