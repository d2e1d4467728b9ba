"""Phase 2 of the folded s2.0 (csrc/wino_h3.hip, FOLD) reads p3 as its nearest x2 upsample, so transform row 2 of every tile is an
exact zero and the wave that owns the row only stages its share of the input there (fpc_net_set_fold_idle_row, default 1).  With
the switch at 0 that wave runs the phase on its zeros as before.  ResNet18 engines with every 3x3 / stride-1 site on form 9 and
the fold forced, at p2 shapes whose patches are all border patches with a ragged one (16 x 24), carry a seam at an odd frame count
(24 x 32, the shape the orientation rule transposes: both orientations) and hold a patch with no border (48 x 48):
  1. switch 1 EQUALS (torch.equal) switch 0 on s2.0's output of the four decoders and on the logits;
  2. s2.0 against float64 of the same c2 / p3 at 2e-5 of the tensor's scale with the switch at 1;
  3. a recorded graph replays the plain run bit for bit, and the switch drops the recorded graph."""
import ctypes

import pytest
import torch

from test_gpu_p2_fold import _check_seg6, _model

pytestmark = pytest.mark.gpu

SHAPES = [(2, 64, 96), (3, 96, 128), (1, 192, 192)]      # (B, image H, W): p2 = 16 x 24, 24 x 32, 48 x 48


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(dev):
    import fastposecnn_amd.lib as L
    from fastposecnn_amd import _native
    _native.lib()
    return L


def _fold_engine(lib, dev, B, H, W):
    from fastposecnn_amd.engine import NetEngine
    m, _ = _model(lib, encoder="resnet18")
    m = m.to(dev)
    eng = NetEngine(m, B, H, W, dev, autotune=False, split_precision=3)
    eng.force_winograd(9)
    eng.force_fold(1)
    assert any(p[2] == 5000 for p in eng.conv_plans()), "s2.0 is not folded"
    return m, eng


def _transposes(B, H2, W2):
    """whether the orientation rule transposes the folded s2.0 at a p2 of H2 x W2 (the library's own geometry)"""
    from fastposecnn_amd import _native as nat
    out = (ctypes.c_int64 * 9)()
    nat.check(nat.lib().fpc_wino_orient_geometry(H2, W2, B, 64, 1, 1, out), "fpc_wino_orient_geometry")
    return int(out[0]) == 1


def _run(eng, x):
    with torch.no_grad():
        logits, _ = eng.forward(x)
    torch.cuda.synchronize()
    out = {f"d{d}.seg6": eng.tensor(f"d{d}.seg6").detach().clone() for d in range(4)}
    out.update({"logits." + k: v.detach().clone() for k, v in logits.items()})
    return out


def test_the_shapes_cover_both_orientations():
    assert [_transposes(B, H // 4, W // 4) for B, H, W in SHAPES] == [False, True, False]


@pytest.mark.parametrize("B,H,W", SHAPES, ids=lambda v: str(v))
def test_idle_row_equals_every_row(lib, dev, B, H, W):
    from fastposecnn_amd import synth
    m, eng = _fold_engine(lib, dev, B, H, W)
    x = torch.stack([synth.make_image(i, H, W) for i in range(B)]).to(dev)
    for orient in ((1, 0) if _transposes(B, H // 4, W // 4) else (1,)):
        eng.set_wino_orient(orient)
        eng.set_fold_idle_row(1)
        idle = _run(eng, x)
        _check_seg6(m, eng, list(range(B)))
        eng.set_fold_idle_row(0)
        every = _run(eng, x)
        for k, v in idle.items():
            assert not torch.isnan(v).any(), (orient, k)
            assert torch.equal(v, every[k]), (orient, k, "the idle row changed a result")


@pytest.mark.parametrize("B,H,W", SHAPES, ids=lambda v: str(v))
def test_graph_replay_equals_the_plain_run(lib, dev, B, H, W):
    from fastposecnn_amd import _native as nat, synth
    m, eng = _fold_engine(lib, dev, B, H, W)
    xs = [torch.stack([synth.make_image(i + j, H, W) for j in range(B)]).to(dev) for i in range(2)]
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        plain = [_run(eng, x) for x in xs]
        assert not eng.graph_recorded()
        nat.check(eng._lib.fpc_net_set_graph(eng._h, 1), "fpc_net_set_graph")
        replay = [_run(eng, x) for x in xs + xs][2:]
        assert eng.graph_recorded()
        for a, b in zip(plain, replay):
            for k in a:
                assert torch.equal(a[k], b[k]), k
        eng.set_fold_idle_row(1)      # unchanged: the graph stays
        assert eng.graph_recorded()
        eng.set_fold_idle_row(0)
        assert not eng.graph_recorded()
        every = _run(eng, xs[0])
        for k in every:
            assert torch.equal(every[k], plain[0][k]), k
    side.synchronize()
