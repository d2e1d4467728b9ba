"""CPU checks of what tests/test_gpu_batch_forms.py relies on (tests/_batch_forms.py): the encoder sites read off the modules
against counts by plain arithmetic, the frame size of each family's batch against the rule that picks it (host arithmetic of the
library's form functions; no compute calls into the HIP library), and the condition the batch tests put on their own inputs."""
import pytest

import _batch_forms as BF
import _densenet_model as D


@pytest.fixture(scope="module")
def hiplib():
    from fastposecnn_amd import build, _native
    build.build()
    return _native.lib()


@pytest.fixture(scope="module")
def encoders():
    import fastposecnn_amd.lib as L
    return {name: D.model(L, name)[0].encoder for name in BF.SHAPES}


def test_sites_read_off_the_modules(encoders):
    """densenet121: 58 layers of a 1x1 to 128 channels and a 3x3 of 128 -> 32, three transitions behind their pool; mobilenet_v2: 16
    expand and 17 project sites and the last 1x1; efficientnet-b0: 15 expand and 16 project sites (the gates' 1x1s and _conv_head,
    which forward does not run, are no sites)."""
    dn = BF.sites(encoders["densenet121"])
    assert len(dn) == 2 * 58 + 3 and sum(kind == "conv3" for _, kind, *_ in dn) == 58
    assert [s[2:] for s in dn if "transition" in s[0]] == [(8, 256, 128), (16, 512, 256), (32, 1024, 512)]      # (twice the module's stride)
    c, stride, layers = 64, 4, iter(s for s in dn if "transition" not in s[0])
    for n in (6, 12, 24, 16):
        for j in range(n):
            assert next(layers)[1:] == ("pw", stride, c + 32 * j, 128) and next(layers)[1:] == ("conv3", stride, 128, 32)
        c, stride = (c + 32 * n) // 2, 2 * stride
    mb = BF.sites(encoders["mobilenet_v2"])
    assert len(mb) == 16 + 17 + 1 and mb[0][1:] == ("pw", 2, 32, 16) and mb[-1][1:] == ("pw", 32, 320, 1280)
    assert all(kind == "pw" for _, kind, *_ in mb) and sorted({s[2] for s in mb}) == [2, 4, 8, 16, 32]
    ef = BF.sites(encoders["efficientnet-b0"])
    assert len(ef) == 15 + 16 and ef[0][1:] == ("pw", 2, 32, 16) and ef[-1][1:] == ("pw", 32, 1152, 320)
    assert not any("_se_" in s[0] or "_conv_head" in s[0] for s in ef) and max(s[3] for s in ef) == 1152


def test_the_batch_shapes_follow_their_rule(hiplib, encoders):
    for name, enc in encoders.items():
        H, W = BF.SHAPES[name]
        full = BF.form_set(BF.site_forms(hiplib, enc, BF.BATCH, *BF.FULL))
        here = BF.site_forms(hiplib, enc, BF.BATCH, H, W)
        assert H % 32 == 0 and W % 32 == 0 and (H // 32) * (W // 32) % 2 == 1 and H * W < BF.FULL[0] * BF.FULL[1]
        assert full <= BF.form_set(here), name
        assert BF.smallest_shape(hiplib, enc, full) == (96, 352), name
    assert BF.SHAPES["mobilenet_v2"] == BF.SHAPES["efficientnet-b0"] == (96, 352)
    # densenet121 at 96 x 352 against 352 x 416: the large-batch forms on block 1 alone / on blocks 1 and 2 (3x3) and 1 .. 3 (1x1)
    dn = encoders["densenet121"]
    by_block = lambda rows, kind: [sorted({r[5] for r in rows if r[1] == kind and f"denseblock{b}" in r[0]}) for b in (1, 2, 3, 4)]
    least = BF.site_forms(hiplib, dn, BF.BATCH, 96, 352)
    assert by_block(least, "conv3") == [[1], [0], [0], [0]] and by_block(least, "pw") == [[1], [1], [0], [0]]
    here = BF.site_forms(hiplib, dn, BF.BATCH, *BF.SHAPES["densenet121"])
    assert by_block(here, "conv3") == [[1], [1], [0], [0]] and by_block(here, "pw") == [[1], [1], [1], [0]]
    full = BF.site_forms(hiplib, dn, BF.BATCH, *BF.FULL)
    assert by_block(full, "conv3") == [[1], [1], [0], [0]] and by_block(full, "pw") == [[1], [1], [1], [1]]
    per_frame = {b: next(r[2] for r in here if f"denseblock{b}." in r[0]) // BF.BATCH for b in (1, 2, 3, 4)}
    assert per_frame == {1: 9152, 2: 2288, 3: 572, 4: 143} and per_frame[2] % 64 and per_frame[3] % 32 and per_frame[4] % 16


@pytest.mark.parametrize("name", ["mobilenet_v2", "efficientnet-b0"])
def test_the_batch_tests_frames_are_well_conditioned(name):
    """What tests/test_gpu_batch_forms.py asks of its own inputs (tests/test_densenet_encoder.py holds densenet121's): torch's f32 CPU
    forward of frames 0, 17 and 31 stays within a quarter of the network bar 1e-4 max(1, |ref|max) of float64 on c2 .. c5 and every
    logit, so the bar measures the engine and not the conditioning of the draw."""
    import fastposecnn_amd.lib as L
    x = BF.frames(name)
    assert tuple(x.shape) == (3, 3) + BF.SHAPES[name]
    for err, scale in BF.f32_errors(L, name, x):
        assert err <= 0.25 * 1e-4 * max(1.0, scale), err
