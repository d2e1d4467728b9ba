"""The piece arithmetic of the split-precision convolution forms, emulated in numpy and held to the bound the kernels' headers print.

split_h2 (csrc/common.hpp, and the same two conversions in k_wino_pack_fp16 / k_pack_weight_h3): x = h1 + h2 + rest, h1 = fp16(x) and
h2 = fp16(x - h1), both by v_cvt_pkrtz_f16_f32 — round toward zero, subnormals kept, no infinity (the largest finite value instead).
split_bf3: x = p1 + p2 + p3, each the high 16 bits of what is left.

The bound of |rest| as a function of |x| (h2_bound below), derived from the conversions and checked here against the emulation:
  * h1 keeps the 11 leading bits of x, the residual (13 bits, exact in f32) starts at most at bit 12, h2 keeps 11 bits from its own
    leading bit: what is left are at most the last TWO of x's 24 bits, |rest| <= 3 * 2^-24 * 2^ceil(log2 |x|) <= 3 * 2^-23 |x|
    (1.5 * 2^-22: below 2^-21, NOT below 2^-22 — attained by every mantissa with all 24 bits set);
  * fp16's subnormal spacing is 2^-24: a piece below 2^-14 is a multiple of it, so |rest| < 2^-24 whatever |x| is, and that is the
    smaller bound below |x| = 2^-2 (for |x| < 2^-24 both pieces are zero and rest = x);
  * h1 is pinned at 65 504 from |x| = 2^16 on and h2 carries |x| - 65 504 on 11 bits: |rest| < 2^-10 (|x| - 65 504), up to 32 at
    |x| = 131 008 = 2 * 65 504, where h2 is pinned as well and rest = |x| - 131 008.
The three bf16 pieces are exact for every finite f32 (8 + 8 + 8 bits; masking knows no range).

tests/test_gpu_conv_operands.py propagates h2_bound through the convolutions."""
import os

import numpy as np

F16_MAX = 65504.0
H2_REL = 3.0 * 2.0 ** -23        # |rest| <= H2_REL |x| while both pieces are normal fp16 values
H2_ABS = 2.0 ** -24              # |rest| < H2_ABS as well: fp16's subnormal spacing
H2_FULL = 2.0 ** 16              # h1 is pinned from here on: the relative bound ends
H2_SAT = 2.0 * F16_MAX           # both pieces pinned


def rtz_f16(x):
    """float32 array -> the fp16 value v_cvt_pkrtz_f16_f32 gives, as float32: truncated to fp16's grid (11 significant bits, spacing
    2^-24 below 2^-14), +-65 504 beyond the range.  NaN stays NaN."""
    x = np.asarray(x, np.float32)
    a = np.abs(x).astype(np.float64)
    _, e = np.frexp(a)                                         # a = m 2^e, m in [0.5, 1)
    q = np.ldexp(1.0, np.maximum(e - 11, -24))                 # spacing of the fp16 grid at a
    t = np.minimum(np.floor(a / q) * q, F16_MAX)
    return np.where(np.isnan(x), x, np.copysign(t, x)).astype(np.float32)


def split_h2(x):
    """-> (h1, h2, rest): the pieces as float32 (fp16-representable), rest in float64."""
    x = np.asarray(x, np.float32)
    h1 = rtz_f16(x)
    r = x - h1                                                 # f32, as in the kernel; exact
    assert np.array_equal((x.astype(np.float64) - h1)[np.isfinite(x)], r.astype(np.float64)[np.isfinite(x)])
    h2 = rtz_f16(r)
    return h1, h2, x.astype(np.float64) - h1 - h2


def split_bf3(x):
    """-> (p1, p2, p3, rest): each piece the high 16 bits of what is left (csrc/common.hpp: split_bf3)."""
    x = np.ascontiguousarray(x, np.float32)
    hi = lambda v: (v.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    p1 = hi(x)
    r = (x - p1).astype(np.float32)
    p2 = hi(r)
    q = (r - p2).astype(np.float32)
    p3 = hi(q)
    return p1, p2, p3, x.astype(np.float64) - p1 - p2 - p3


def h2_bound(ax):
    """|rest| of split_h2 as a function of |x| (float64 array, finite): see the module docstring."""
    ax = np.asarray(ax, np.float64)
    low = np.minimum(ax, H2_ABS)
    mid = H2_REL * ax
    top = np.where(ax >= H2_SAT, ax - H2_SAT + 32.0, 2.0 ** -10 * (ax - F16_MAX))
    return np.where(ax < 0.25, low, np.where(ax < H2_FULL, mid, top))


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


def _random_values(n, rng):
    """n float32 values with uniform mantissa bits and exponents over 2^-30 .. 2^18, both signs."""
    bits = rng.integers(0, 1 << 23, n, dtype=np.uint32) | (rng.integers(127 - 30, 127 + 18, n, dtype=np.uint32) << np.uint32(23))
    bits |= rng.integers(0, 2, n, dtype=np.uint32) << np.uint32(31)
    return bits.view(np.float32)


def test_rtz_f16_is_the_truncating_conversion():
    """Against numpy's own float16 on what both define: a value on fp16's grid comes back unchanged (subnormals included), one
    between two grid points goes to the one nearer zero, and nothing becomes infinite."""
    rng = np.random.default_rng(0)
    h = rng.integers(0, 0x7C00, 20000).astype(np.uint16).view(np.float16).astype(np.float32)      # every class of finite fp16
    assert np.array_equal(rtz_f16(h), h) and np.array_equal(rtz_f16(-h), -h)
    with np.errstate(over="ignore"):
        up = np.nextafter(h.astype(np.float16), np.float16(np.inf)).astype(np.float32)
    inside = (h + (up - h) * np.float32(0.75)).astype(np.float32)                                  # exact: the gap is a power of two
    ok = np.isfinite(up)
    assert np.array_equal(rtz_f16(inside[ok]), h[ok]) and np.array_equal(rtz_f16(-inside[ok]), -h[ok])
    assert np.array_equal(rtz_f16(_f32([65519.0, 65520.0, 1e6, 3e38, np.inf])), _f32([F16_MAX] * 5))
    assert np.array_equal(rtz_f16(_f32([2.0 ** -25, 2.0 ** -24, 1.75 * 2.0 ** -24, 0.0])), _f32([0.0, 2.0 ** -24, 2.0 ** -24, 0.0]))
    assert np.isnan(rtz_f16(_f32([np.nan]))[0])


def test_fp16_pair_bound_on_random_values():
    x = _random_values(1_000_000, np.random.default_rng(1))
    h1, h2, rest = split_h2(x)
    ax = np.abs(x).astype(np.float64)
    assert (np.abs(rest) <= h2_bound(ax)).all()
    assert (np.sign(rest) * np.sign(x) >= 0).all()              # truncation: the residual never has the other sign (it adds coherently)
    inside = (ax >= 0.25) & (ax < H2_FULL)
    worst = (np.abs(rest[inside]) / ax[inside]).max()
    assert 2.0 ** -22 < worst <= H2_REL                         # the 2^-22 once printed in the headers does not hold
    assert np.abs(rest[ax < 0.25]).max() < H2_ABS
    assert np.abs(rest[ax < 0.25]).max() > 2.0 ** -25           # ... nor does 2^-25 absolute


def test_fp16_pair_bound_on_the_worst_mantissas_of_every_binade():
    """All 24 bits set and 1 + 2^-23, in every binade from 2^-26 to 2^17: the bound holds, and the all-ones mantissa ATTAINS it wherever
    both pieces are normal fp16 values (3 * 2^-23 of the binade's 2^e, the last two bits of x)."""
    for e in range(-26, 18):
        full, least = np.float32((2.0 - 2.0 ** -23) * 2.0 ** e), np.float32((1.0 + 2.0 ** -23) * 2.0 ** e)
        for x in (full, least, -full, -least):
            h1, h2, rest = split_h2(np.array([x]))
            ax = abs(float(x))
            assert abs(rest[0]) <= h2_bound(np.array([ax]))[0], (e, x)
            assert float(h1[0]) + float(h2[0]) + rest[0] == float(x)
        rest_full = abs(split_h2(np.array([full]))[2][0])
        if -2 <= e <= 15:
            assert rest_full == 3.0 * 2.0 ** (e - 23), e           # bits 23 and 24 of x are lost
        elif -24 <= e < -2:
            assert rest_full == 2.0 ** -24 - 2.0 ** (e - 23), e    # everything of x below fp16's subnormal spacing
        elif e < -24:
            assert rest_full == float(full), e                     # both pieces are zero
        elif e == 16:
            assert rest_full == 2.0 ** 17 - 2.0 ** -7 - H2_SAT     # 131 071.99 saturates both pieces
            rest_least = abs(split_h2(np.array([least]))[2][0])    # 65 536.008 = 65 504 + 32.008: still 11 bits of the excess
            assert rest_least == 2.0 ** -7


def test_fp16_pair_above_the_first_pieces_range_loses_precision_before_it_saturates():
    """Between 2^16 and 131 008 the first piece is pinned at 65 504 and the second carries the excess on 11 bits: the error grows to
    2^-12 of the value (the headers once named 131 008 as the only limit).  Beyond 131 008 the pair is 131 008."""
    x = _f32([65536.0, 65567.99, 70000.123, 100000.5, 131007.99, 131008.0, 131009.0, 1e6])
    h1, h2, rest = split_h2(x)
    assert (np.abs(rest) <= h2_bound(np.abs(x).astype(np.float64))).all()
    assert np.array_equal(h1, _f32([F16_MAX] * 8)) and np.array_equal(h2[-3:], _f32([F16_MAX] * 3))
    assert rest[0] == 0.0 and rest[3] == 0.5 and rest[4] > 31.0 and rest[-1] == 1e6 - H2_SAT
    assert rest[4] / float(x[4]) > 2.0 ** -12.1


def test_three_bf16_pieces_are_exact_at_every_scale():
    rng = np.random.default_rng(2)
    x = _random_values(1_000_000, rng)
    for s in (2.0 ** -60, 1.0, 2.0 ** 60, 2.0 ** 100):
        xs = (x * np.float32(s)).astype(np.float32)
        p1, p2, p3, rest = split_bf3(xs)
        assert not rest.any()
        for p in (p1, p2, p3):
            assert not (p.view(np.uint32) & np.uint32(0xFFFF)).any()                   # a bf16 value
    for e in range(-26, 18):
        for m in (2.0 - 2.0 ** -23, 1.0 + 2.0 ** -23):
            assert not split_bf3(np.array([m * 2.0 ** e], np.float32))[3].any()


def test_the_printed_constants_are_the_emulated_ones():
    """Every place that states the fp16 pair's bound names the emulated constants."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert H2_REL == 3 * 2.0 ** -23 and H2_ABS == 2.0 ** -24
    for rel in ("fastposecnn_amd/csrc/wino_h2.hip", "fastposecnn_amd/csrc/common.hpp", "fastposecnn_amd/csrc/conv_igemm.hip",
                "include/fpc.h"):
        text = open(os.path.join(repo, rel)).read()
        assert "3 * 2^-23" in text and "2^-24" in text, rel
    design = open(os.path.join(repo, "DESIGN.md"), encoding="utf-8").read()
    assert "3·2⁻²³" in design and "2⁻²⁴ absolute" in design
