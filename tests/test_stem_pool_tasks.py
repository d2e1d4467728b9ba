"""Task arithmetic of the fused stem + max-pool launch (fpc_stem_pool_tasks, host only): bands of 10 pool rows x strips of 32 pool
columns cover every pooled pixel exactly once, and what the launch computes more than once stays under 10 % of the stem's outputs."""
import ctypes

import pytest

BAND = 10


@pytest.fixture(scope="module")
def hiplib():
    from fastposecnn_amd import _native
    return _native.lib()


def _tasks(L, Ho, Wo):
    out = (ctypes.c_int64 * 4)()
    assert L.fpc_stem_pool_tasks(Ho, Wo, out) == 0
    return tuple(out)


@pytest.mark.parametrize("H,W", [(480, 640), (96, 128), (40, 256), (88, 384), (1080, 1920)])
def test_bands_and_strips_cover_every_pool_pixel_once(hiplib, H, W):
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    bands, strips, computed, exist = _tasks(hiplib, Ho, Wo)
    Hp, Wp = Ho // 2, Wo // 2
    seen = [[0] * Wp for _ in range(Hp)]
    rows = 0
    for bd in range(bands):
        r0, nr = bd * BAND, min(BAND, Hp - bd * BAND)
        assert nr >= 1
        for st in range(strips):
            for r in range(r0, r0 + nr):
                for c in range(32 * st, 32 * st + 32):
                    seen[r][c] += 1
        # conv rows 2 r0 - 1 .. 2 (r0 + nr) - 1, those inside the image
        rows += sum(1 for y in range(2 * r0 - 1, 2 * (r0 + nr)) if 0 <= y < Ho)
    assert all(v == 1 for row in seen for v in row)
    assert exist == Ho * Wo
    assert computed == rows * Wo + bands * (strips - 1) * 32      # + one 32-pixel halo tile per task right of strip 0


def test_recompute_share_at_the_headline_frame(hiplib):
    bands, strips, computed, exist = _tasks(hiplib, 240, 320)
    assert (bands, strips) == (12, 5)
    assert bands * strips * 32 == 1920                    # wave tasks of a 32-frame batch: under the 2 048 waves of 256 workgroups
    assert 0.0 < computed / exist - 1.0 < 0.10            # 6.6 %: 11 overlap rows of 240 and 48 halo tiles of 32 pixels


def test_refused_shapes(hiplib):
    out = (ctypes.c_int64 * 4)()
    for Ho, Wo in ((241, 320), (240, 96), (0, 64)):
        assert hiplib.fpc_stem_pool_tasks(Ho, Wo, out) == -1
