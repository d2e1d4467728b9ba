"""fpc_net_guard_ranges (csrc/net.hip), host arithmetic only: which sites synthetic survey records demote, and to which plans.

The nets are created as tests/golden/make_plan_contract.py creates them: no device, no parameters.  Without loaded parameters the
three-product images are not packed, so fpc_net_force_direct_h3 / fpc_net_force_stem_pool refuse (the contract file records that),
and the fp16-piece plans these tests can put a site on are the Winograd forms -8 / -9 and the folded s2.0.  The 6000 + split plans
go through the same function on the device in tests/test_gpu_act_range.py (the saturating network), plan 3100 in its
test_fused_stem_is_surveyed_and_demoted, on a frame the fused launch takes."""
import ctypes
import importlib.util
import json
import os
import struct

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FPC_EINVAL = -1
LO, HI = 2.0 ** -2, 2.0 ** 14
FP16_CODES = lambda c: c in (-8, -9, -10, 3100, 5000) or 6000 <= c < 6200 or 7000 <= c < 7100


def _bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def _below(x):
    """the next float32 below x > 0"""
    return struct.unpack("<f", struct.pack("<I", _bits(x) - 1))[0]


# record kinds: (name, [max bits, non-finite count, visited, reserved], demotes)
KINDS = [
    ("at-lo", [_bits(LO), 0, 1000, 0], False),
    ("below-lo", [_bits(_below(LO)), 0, 1000, 0], True),
    ("below-hi", [_bits(_below(HI)), 0, 1000, 0], False),
    ("at-hi", [_bits(HI), 0, 1000, 0], True),
    ("zero", [0, 0, 1000, 0], False),
    ("unsurveyed", [_bits(1e30), 7, 0, 0], False),
    ("non-finite", [_bits(1.0), 1, 1000, 0], True),
    ("non-finite-only", [0, 3, 0xFFFFFFFF, 0], True),
    ("subnormal", [1, 0, 1000, 0], True),
    ("ordinary", [_bits(3.5), 0, 1000, 0], False),
]


@pytest.fixture(scope="module")
def gen():
    from fastposecnn_amd import build
    build.build()
    spec = importlib.util.spec_from_file_location("make_plan_contract", os.path.join(GOLDEN, "make_plan_contract.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def L():
    from fastposecnn_amd import _native
    return _native.lib()


def _fp16_net(gen, L, cfg, form=9, fold=True):
    """split level 3 and every fp16-piece switch that works without parameters"""
    n = gen.Net(L, *cfg)
    assert L.fpc_net_set_split_precision(n.h, 3) == 0
    assert L.fpc_net_force_winograd(n.h, form) > 0
    if fold and cfg[1] == 1:
        assert L.fpc_net_force_fold(n.h, 1) == 1
    return n


def _guard(L, n, rows, lo=LO, hi=HI, sites=None):
    flat = [v for r in rows for v in r]
    return L.fpc_net_guard_ranges(n.h, (ctypes.c_uint32 * len(flat))(*flat), len(rows) if sites is None else sites, lo, hi)


def _guarded(L, n):
    return [i for i in range(L.fpc_net_conv_count(n.h)) if L.fpc_net_guarded(n.h, i)]


def _expected(before, rows_kind, fold_site, lat_site, base):
    """the plans the rule names: a demoted Winograd site on -7 with everything else of its report unchanged; the demoted fold as the
    unfolded pair — s2.0 on -7 and the p2 lateral back on the plan it had before the fold"""
    want = [list(p) for p in before]
    demoted = []
    for i, (p, kind) in enumerate(zip(before, rows_kind)):
        if not FP16_CODES(p[2]) or p[2] == 5000 or not kind[2]:
            continue
        want[i][2] = -7
        demoted.append(i)
        if i == fold_site:
            want[lat_site] = list(base[lat_site])
    return want, demoted


@pytest.mark.parametrize("form", [9, 8])
@pytest.mark.parametrize("cfg_index", [0, 2, 4])
def test_records_demote_exactly_the_sites_the_rule_names(gen, L, cfg_index, form):
    cfg = gen.NETS[cfg_index]
    base_net = gen.Net(L, *cfg)
    base = base_net.plans()
    base_net.close()
    n = _fp16_net(gen, L, cfg, form, fold=form == 9)
    try:
        before = n.plans()
        sites = len(before)
        fp16 = [i for i, p in enumerate(before) if FP16_CODES(p[2]) and p[2] != 5000]
        assert len(fp16) >= 10, before
        folded = [i for i, p in enumerate(before) if p[2] == 5000]
        fold_site = lat_site = -1
        if folded:
            lat_site = folded[0]
            fold_site = max(fp16)      # s2.0: the last 3x3 site of decoder 0
        # every kind on some fp16-piece site (round robin), and on every other site a record that WOULD demote
        kinds = [KINDS[3]] * sites
        for k, i in enumerate(fp16):
            kinds[i] = KINDS[k % len(KINDS)]
        if fold_site >= 0:
            kinds[fold_site] = KINDS[3]      # the fold itself is demoted
        assert {k[0] for i, k in enumerate(kinds) if i in fp16} == {k[0] for k in KINDS}
        want, demoted = _expected(before, kinds, fold_site, lat_site, base)
        assert demoted and len(demoted) < len(fp16)
        ws = L.fpc_net_workspace_bytes(n.h)

        assert _guard(L, n, [k[1] for k in kinds], sites=sites + 1) == FPC_EINVAL
        assert _guard(L, n, [k[1] for k in kinds], sites=sites - 1) == FPC_EINVAL
        assert _guard(L, n, [k[1] for k in kinds], lo=1.0, hi=1.0) == FPC_EINVAL
        assert n.plans() == before and _guarded(L, n) == []

        assert _guard(L, n, [k[1] for k in kinds]) == len(demoted)
        after = n.plans()
        assert after == want, [(i, b, a, w) for i, (b, a, w) in enumerate(zip(before, after, want)) if a != w]
        assert _guarded(L, n) == demoted
        # no site that was not on an fp16-piece form changed (the p2 lateral reported "folded away": part of the fold)
        assert all(a == b for i, (a, b) in enumerate(zip(after, before)) if not FP16_CODES(b[2]))
        # idempotent
        assert _guard(L, n, [k[1] for k in kinds]) == 0
        assert n.plans() == after and _guarded(L, n) == demoted
        # the workspace is the contract's
        with open(os.path.join(GOLDEN, "plan_contract.json")) as f:
            golden = json.load(f)["nets"][cfg_index]
        assert golden["net"][3:] == list(cfg[3:])
        assert L.fpc_net_workspace_bytes(n.h) == ws == golden["workspace_bytes"]

        # copy_plans carries the demotions (another batch size of the same frame)
        dst = gen.Net(L, cfg[0], cfg[1], cfg[2], 1, cfg[4], cfg[5])
        try:
            assert L.fpc_net_set_split_precision(dst.h, 3) == 0
            assert L.fpc_net_copy_plans(dst.h, n.h) == 0
            assert _guarded(L, dst) == demoted
            assert [p[2] for p in dst.plans()] == [p[2] for p in after]
            assert _guard(L, dst, [k[1] for k in kinds]) == 0
        finally:
            dst.close()

        # an explicit request afterwards wins
        assert L.fpc_net_force_winograd(n.h, 9) > 0
        assert _guarded(L, n) == []
        assert all(p[2] == -9 for i, p in enumerate(n.plans()) if i in fp16)
        # ... and the same records demote the same Winograd sites again (the fold was not asked for again)
        assert _guard(L, n, [k[1] for k in kinds]) == len(demoted)
        assert _guarded(L, n) == demoted
    finally:
        n.close()


def test_a_plan_without_fp16_piece_sites_is_left_alone(gen, L):
    """split level 1 plans (every Winograd site on -7) and the heuristic plans: records that would demote change nothing"""
    cfg = gen.NETS[0]
    for force in (0, 7):
        n = gen.Net(L, *cfg)
        try:
            if force:
                assert L.fpc_net_force_winograd(n.h, force) > 0
            before = n.plans()
            assert not any(FP16_CODES(p[2]) for p in before)
            for kind in KINDS:
                assert _guard(L, n, [kind[1]] * len(before)) == 0
            assert n.plans() == before and _guarded(L, n) == []
        finally:
            n.close()


def test_custom_bounds_and_null_arguments(gen, L):
    cfg = gen.NETS[0]
    n = _fp16_net(gen, L, cfg)
    try:
        sites = L.fpc_net_conv_count(n.h)
        row = [_bits(3.5), 0, 10, 0]
        assert _guard(L, n, [row] * sites) == 0
        assert L.fpc_net_guard_ranges(None, (ctypes.c_uint32 * (4 * sites))(), sites, LO, HI) == FPC_EINVAL
        assert L.fpc_net_guard_ranges(n.h, None, sites, LO, HI) == FPC_EINVAL
        assert _guard(L, n, [row] * sites, lo=-1.0) == FPC_EINVAL
        assert _guard(L, n, [row] * sites, lo=float("nan")) == FPC_EINVAL
        assert L.fpc_net_guarded(n.h, -1) == 0 and L.fpc_net_guarded(n.h, sites) == 0
        fp16 = sum(1 for p in n.plans() if FP16_CODES(p[2]) and p[2] != 5000)
        assert _guard(L, n, [row] * sites, lo=4.0, hi=8.0) == fp16      # 3.5 < lo = 4
        assert not any(FP16_CODES(p[2]) for p in n.plans())
    finally:
        n.close()


def test_the_fold_is_demoted_by_either_of_its_two_records(gen, L):
    """The folded s2.0 reads c2 (its own record) and p3 (surveyed into the record of the p2 lateral site, which does not run while it
    is folded away)."""
    cfg = gen.NETS[0]
    ok, bad, none = [_bits(3.5), 0, 10, 0], [_bits(2.0 ** -9), 0, 10, 0], [0, 0, 0, 0]
    for own, lateral, want in ((ok, ok, 0), (ok, none, 0), (bad, ok, 1), (ok, bad, 1), (none, bad, 0)):
        n = _fp16_net(gen, L, cfg)
        try:
            plans = n.plans()
            lat_site = [i for i, p in enumerate(plans) if p[2] == 5000][0]
            fold_site = max(i for i, p in enumerate(plans) if p[2] == -9)
            rows = [none] * len(plans)
            rows[fold_site], rows[lat_site] = own, lateral
            assert _guard(L, n, rows) == want, (own, lateral)
            assert _guarded(L, n) == ([fold_site] if want else [])
            assert (n.plans()[fold_site][2], n.plans()[lat_site][2] == 5000) == ((-7, False) if want else (-9, True))
        finally:
            n.close()


def test_copy_plans_keeps_the_demotions_of_both_sides(gen, L):
    """a site dst demoted itself stays demoted when src, which never demoted it, is copied over it"""
    cfg = gen.NETS[0]
    src, dst = _fp16_net(gen, L, cfg), _fp16_net(gen, L, cfg)
    try:
        plans = src.plans()
        fp16 = [i for i, p in enumerate(plans) if p[2] == -9]
        a, b = fp16[0], fp16[1]
        none, bad = [0, 0, 0, 0], [_bits(HI), 0, 10, 0]
        rows = [none] * len(plans)
        rows[a] = bad
        assert _guard(L, src, rows) == 1
        rows = [none] * len(plans)
        rows[b] = bad
        assert _guard(L, dst, rows) == 1
        assert L.fpc_net_copy_plans(dst.h, src.h) == 0
        assert _guarded(L, dst) == sorted([a, b])
        assert dst.plans()[a][2] == -7 and dst.plans()[b][2] == -7      # b: src's plan for it is -9, dst's demotion holds
        assert _guarded(L, src) == [a]
    finally:
        src.close()
        dst.close()


def test_survey_next_refuses_a_plan_without_parameters(gen, L):
    """fpc_net_survey_next's argument checks that need no device; the rest is in tests/test_gpu_act_range.py"""
    n = gen.Net(L, *gen.NETS[0])
    try:
        sites = L.fpc_net_conv_count(n.h)
        rec = (ctypes.c_uint32 * (4 * sites))()
        assert L.fpc_net_survey_next(n.h, ctypes.addressof(rec), sites) == FPC_EINVAL      # not loaded
        assert L.fpc_net_survey_next(None, ctypes.addressof(rec), sites) == FPC_EINVAL
        assert L.fpc_net_survey_next(None, None, sites) == FPC_EINVAL
        assert L.fpc_net_survey_next(n.h, None, sites) == 0                                  # NULL disarms, always
    finally:
        n.close()
