"""The depthwise family (csrc/depthwise.hip) computes, bit for bit, what the two encoders' separate copies of these kernels computed.
On the launches tools_dev/depthwise_digest.py lists — every entry (fpc_dwconv3x3, fpc_mbconv_dw and the _dgrad / _wgrad of both), every
(k, stride) and activation code, on shapes where every tap pads, with strip, block and slice tails, 126 workgroups, more than 256
channel quads, fewer units than pixel slots and, for the pad-1 entries at stride 2, odd extents —, outputs pre-filled with NaN:
  1. every output element is written;
  2. the SHA-256 of every output equals the one committed in tests/golden/depthwise_digests.json, which that script wrote on the
     commit before the family was made one;
  3. the "same"-pad entries at (3, 1) and the pad-1 entries at stride 1 are one convolution: on the same operands, the same bits."""
import functools
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _load_tool():
    spec = importlib.util.spec_from_file_location("depthwise_digest", os.path.join(HERE, "..", "tools_dev", "depthwise_digest.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


tool = _load_tool()
with open(os.path.join(HERE, "golden", "depthwise_digests.json")) as f:
    GOLDEN = json.load(f)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(dev):
    """The loaded library: a missing one fails here, once, not in every case."""
    from fastposecnn_amd import _native
    return _native.lib()


@functools.lru_cache(maxsize=None)
def _outputs(op):
    """{case name: (case, output)} of one operation, computed once and left unchanged."""
    dev = torch.device("cuda:0")
    return {case[0]: (case, tool.run_case(dev, case)) for case in tool.cases() if case[2] == op}


def test_the_golden_file_names_exactly_the_listed_launches():
    cases = tool.cases()
    assert set(GOLDEN) == {c[0] for c in cases} and len(cases) == len(GOLDEN) and all(len(v) == 64 for v in GOLDEN.values())
    for family, op in [(f, o) for f in ("dw3", "mb") for o in tool.OPS]:
        sel = [c for c in cases if c[1] == family and c[2] == op]
        acts = {c[6] for c in sel}
        assert acts == ({0} if op != "fwd" else {0, 1} if family == "dw3" else {0, 1, 2}), (family, op, acts)
        assert {c[3] for c in sel} == set(tool.SHAPES) | ({tool.ODD} if family == "dw3" else set())
        assert {(c[4], c[5]) for c in sel} == ({(3, 1), (3, 2)} if family == "dw3" else set(tool.KS))
    assert all(c[5] == 2 and c[1] == "dw3" for c in cases if c[3] == tool.ODD)


@pytest.mark.parametrize("op", tool.OPS)
def test_digests_equal_the_commit_before(lib, dev, op):
    bad = []
    for name, (case, out) in _outputs(op).items():
        assert not torch.isnan(out).any(), (name, "unwritten outputs")
        if tool.digest(out) != GOLDEN[name]:
            bad.append(name)
    assert not bad, f"{len(bad)} outputs differ from the commit before, the first: {bad[:6]}"


@pytest.mark.parametrize("op", tool.OPS)
def test_same_pad_3x3_stride_1_is_the_pad_1_convolution(lib, dev, op):
    outs = _outputs(op)
    pairs = 0
    for name, (case, out) in outs.items():
        if case[1] == "dw3" and case[5] == 1:
            twin = "mb-" + name[len("dw3-"):].replace("-s1-", "-k3s1-")
            assert torch.equal(out, outs[twin][1]), (name, twin)
            pairs += 1
    assert pairs == len(tool.SHAPES) * (2 if op == "fwd" else 1)
