"""The XCD-banded workgroup order (csrc/conv_device.hpp: xcd_logical, xcd_span) through its host probe fpc_xcd_order, no GPU:
  * the block remap is a permutation of [0, grid) that puts block b into the (b % 8)-th eighth when grid % 8 == 0, else the identity;
  * the spans of all blocks and slots visit every item of [0, total) exactly once;
  * at the largest item count the launchers admit, on the largest grid, no 32-bit index of a walk wraps;
  * the probe refuses what it says it refuses."""
import ctypes
from collections import Counter

import pytest

WALK_LIMIT = (1 << 32) - 4096 * 256 - 8      # csrc/common.hpp: kWalkLimit


@pytest.fixture(scope="module")
def hiplib():
    from fastposecnn_amd import _native
    return _native.lib()


def _order(L, grid, block, total, per_block, slot):
    out = (ctypes.c_int64 * 4)()
    assert L.fpc_xcd_order(grid, block, total, per_block, slot, out) == 0, (grid, block, total, per_block, slot)
    return tuple(out)


@pytest.mark.parametrize("grid", list(range(1, 73)) + [256, 4096])
def test_the_remap_is_a_permutation_into_eighths(hiplib, grid):
    logical = [_order(hiplib, grid, b, 0, 1, 0)[0] for b in range(grid)]
    if grid % 8:
        assert logical == list(range(grid))
        return
    assert sorted(logical) == list(range(grid))
    for b, l in enumerate(logical):
        assert (b % 8) * grid // 8 <= l < (b % 8 + 1) * grid // 8, (grid, b, l)


@pytest.mark.parametrize("grid", [1, 3, 8, 16, 24, 40])
@pytest.mark.parametrize("per_block", [8, 16, 32, 256])
def test_the_walks_visit_every_item_once(hiplib, grid, per_block):
    for total in (0, 1, 7, 8, 9, 63, 64, 65, 1000, 4099):
        seen = Counter()
        for b in range(grid):
            for s in range(per_block):
                _, first, end, step = _order(hiplib, grid, b, total, per_block, s)
                assert step >= 1
                seen.update(range(first, end, step))
        assert seen == Counter(range(total)), (grid, per_block, total)


def test_no_index_wraps_at_the_walk_limit(hiplib):
    total, grid, per_block = WALK_LIMIT - 1, 4096, 256
    for b in range(grid):
        for s in (0, per_block - 1):      # first grows with the slot: the two ends
            _, first, end, step = _order(hiplib, grid, b, total, per_block, s)
            # the probe widens the kernel's 32-bit words: a wrapped one would show as a small value, so hold them to the exact integers
            per = (total + 7) // 8
            lo = (b % 8) * per
            assert first == lo + (b // 8) * per_block + s and end == min(lo + per, total) and step == grid // 8 * per_block
            assert max(first, end, end - 1 + step) < 1 << 32, (b, s, first, end, step)


def test_refusals(hiplib):
    out = (ctypes.c_int64 * 4)()
    ok = dict(grid=8, block=0, total=100, per_block=16, slot=0)
    assert hiplib.fpc_xcd_order(*ok.values(), out) == 0
    for bad in (dict(grid=0), dict(grid=-8), dict(block=-1), dict(block=8), dict(per_block=0), dict(slot=-1), dict(slot=16),
                dict(total=-1), dict(total=WALK_LIMIT)):
        assert hiplib.fpc_xcd_order(*{**ok, **bad}.values(), out) == -1, bad
    assert hiplib.fpc_xcd_order(*{**ok, "total": WALK_LIMIT - 1}.values(), out) == 0
    assert hiplib.fpc_xcd_order(*ok.values(), None) == -1
