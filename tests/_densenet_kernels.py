"""What the DenseNet kernel tests share (tests/test_gpu_densenet.py, tests/test_gpu_densenet_sweep.py): the twice-launched, canaried,
pattern-filled output buffer, the kernel bar, the operands and the float64 reference of fpc_dense_pw, the packed launch of
fpc_dense_conv3x3, and the launch arithmetic of csrc/densenet.hip restated, so that a test can say which grid its case runs on."""
import torch

NAN = float("nan")


def _twice(dev, prefill, launch):
    """Two launches into fresh buffers: 64 NaN canaries, `prefill` (CPU f32, NaN wherever the kernel must write, a pattern wherever it
    must not), 64 NaN canaries.  The canaries intact, the pattern intact bit for bit, nothing left unwritten, both runs the same
    bits.  Returns the first run's body (CPU, flat)."""
    n = prefill.numel()
    keep = ~torch.isnan(prefill.view(-1))
    outs = []
    for _ in range(2):
        buf = torch.full((n + 128,), NAN)
        buf[64:64 + n] = prefill.view(-1)
        buf = buf.to(dev)
        y = buf[64:64 + n]
        assert y.data_ptr() % 16 == 0
        assert launch(y.data_ptr()) == 0
        torch.cuda.synchronize()
        host = buf.cpu()
        assert torch.isnan(host[:64]).all() and torch.isnan(host[64 + n:]).all(), "a canary was overwritten"
        body = host[64:64 + n]
        assert torch.equal(body[keep].view(torch.int32), prefill.view(-1)[keep].view(torch.int32)), "wrote outside its slice"
        assert not torch.isnan(body[~keep]).any(), "unwritten outputs"
        outs.append(body)
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    return outs[0]


def _pitched(M, ld, lo, hi):
    """[M][ld] pre-fill: NaN in columns [lo, hi), a pattern of finite values (no two neighbours alike) elsewhere."""
    t = (torch.arange(M * ld, dtype=torch.float32) % 977 - 400.0).view(M, ld) * 0.25
    t[:, lo:hi] = NAN
    return t


def _bar(out, ref, what):
    err = (out.double() - ref).abs().max().item()
    print(what, "err", err, "ref max", ref.abs().max().item())
    assert err <= 2e-5 * max(1.0, ref.abs().max().item()), (what, err)


# ---------------------------------------------------------------------------------------------------------------- fpc_dense_pw

def _pw_operands(g, M, K, ldi, whole, rows=128):
    """in [M][ldi] with NaN behind channel K, s1 / t1 [K], w [rows][K], s2 / t2 [rows] (a narrower Cout takes their first rows)."""
    if whole:
        x = torch.randint(-4, 5, (M, K), generator=g).float()
        s1, t1 = torch.randint(1, 3, (K,), generator=g).float(), torch.randint(-3, 4, (K,), generator=g).float()
        w = torch.randint(-2, 3, (rows, K), generator=g).float()
        s2, t2 = torch.randint(1, 4, (rows,), generator=g).float(), torch.randint(-5, 6, (rows,), generator=g).float()
    else:
        x = torch.randn((M, K), generator=g)
        s1, t1 = (torch.rand(K, generator=g) + 0.5), torch.randn(K, generator=g) * 0.5
        w = torch.randn((rows, K), generator=g) * 2.0 / K ** 0.5
        s2, t2 = (torch.rand(rows, generator=g) + 0.5) * 2.0, torch.randn(rows, generator=g)
    xin = torch.full((M, ldi), NAN)
    xin[:, :K] = x
    return x, xin, s1, t1, w, s2, t2


def _pw_ref(x, s1, t1, w, s2, t2, Cout, pre, act, affine=True):
    a = x.double()
    if pre:
        a = (a * s1.double() + t1.double()).clamp_min(0.0)
    v = a @ w[:Cout].double().t()
    if affine:
        v = v * s2[:Cout].double() + t2[:Cout].double()
    return v.clamp_min(0.0) if act else v


# ----------------------------------------------------------------------------------------------------------- fpc_dense_conv3x3

def _conv_run(dev, x, w, c0, ldo, form):
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    B, _, H, W = x.shape
    xd = x.permute(0, 2, 3, 1).contiguous().to(dev)
    wd = w.contiguous().to(dev)
    wt = torch.full((9 * 32 * 128 + 64,), NAN, device=dev)
    assert L.fpc_dense_conv3x3_pack(wd.data_ptr(), wt.data_ptr(), nat.stream()) == 0
    assert torch.isnan(wt[9 * 32 * 128:]).all() and not torch.isnan(wt[:9 * 32 * 128]).any()
    assert torch.equal(wt[:9 * 32 * 128].view(9, 32, 128).cpu(), w.permute(2, 3, 0, 1).reshape(9, 32, 128))
    out = _twice(dev, _pitched(B * H * W, ldo, c0, c0 + 32), lambda y: L.fpc_dense_conv3x3(xd.data_ptr(), wt.data_ptr(), y, B, H, W, c0, ldo,
                                                                                          form, nat.stream()))
    return out.view(B, H, W, ldo)[..., c0:c0 + 32].permute(0, 3, 1, 2)


# ------------------------------------------------------------------------- the launch arithmetic of csrc/densenet.hip, restated

def _bands(grid):
    """A grid of 8 or more workgroups is rounded up to a multiple of 8 (launch_dense_pw, launch_dense_conv3's tile form; the split
    form launches exactly one workgroup per tile) and walked in eight contiguous bands (xcd_block); below 8, in launch order.
    Returns (grid, band): band 0 = launch order, band 1 = the permutation is the identity."""
    if grid >= 8:
        grid = (grid + 7) // 8 * 8
    return grid, (grid // 8 if grid % 8 == 0 else 0)


def conv3_launch(M, form):
    """launch_dense_conv3: (tiles, their pixels, workgroups, band, waves or workgroups past the last tile)."""
    if form:
        tiles = (M + 63) // 64
        grid, band = _bands((tiles + 3) // 4)
        return dict(tiles=tiles, rows=64, grid=grid, band=band, idle=4 * grid - tiles)
    tiles = (M + 15) // 16
    return dict(tiles=tiles, rows=16, grid=tiles, band=tiles // 8 if tiles % 8 == 0 else 0, idle=0)


def pw_launch(M, Cout, form):
    """launch_dense_pw: form 1 a wave per 32 x 32 tile, four to a workgroup; form 0 a workgroup per 16 x 16 tile."""
    tile = 32 if form else 16
    mtiles, ntiles = (M + tile - 1) // tile, Cout // tile
    waves = mtiles * ntiles
    grid, band = _bands((waves + 3) // 4 if form else waves)
    return dict(mtiles=mtiles, ntiles=ntiles, waves=waves, grid=grid, band=band, idle=(4 * grid if form else grid) - waves)
