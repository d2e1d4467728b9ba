"""The kernels that run in the XCD-banded workgroup order (csrc/conv_device.hpp: xcd_logical, xcd_span) compute, bit for bit, what
they computed while each carried its own copy of the order.  On the launches tools_dev/xcd_order_digest.py lists — per kernel instance
a grid below 8 (the plain order), a multiple of 8 (the banded order) and one of at least 9 that is no multiple of 8 (rounded up where
the launcher rounds: the surplus ids must leave without writing), and four network forwards for the kernels no entry reaches alone —,
outputs pre-filled with NaN:
  1. every output element is written;
  2. the SHA-256 of every output equals the one committed in tests/golden/xcd_order_digests.json, which that script wrote on the
     commit before the copies became calls of the one helper."""
import functools
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _load_tool():
    spec = importlib.util.spec_from_file_location("xcd_order_digest", os.path.join(HERE, "..", "tools_dev", "xcd_order_digest.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


tool = _load_tool()
with open(os.path.join(HERE, "golden", "xcd_order_digests.json")) as f:
    GOLDEN = json.load(f)
KINDS = sorted({c[1] for c in tool.cases()})


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
def _outputs(kind):
    """{case name: outputs} of one kind of entry, computed once and left unchanged."""
    dev = torch.device("cuda:0")
    return {case[0]: tool.run_case(dev, case) for case in tool.cases() if case[1] == kind}


def test_the_golden_file_names_exactly_the_listed_launches():
    cases = tool.cases()
    names = [c[0] for c in cases]
    assert len(set(names)) == len(names) and set(GOLDEN) == set(names) and all(len(v) == 64 for v in GOLDEN.values())
    # three grids per instance: every tag family ends in a, b and c (the 32 x 32 forms of the f32 1x1 have no grid below 8)
    stems = {}
    for n in names:
        if n[-2:] in ("-a", "-b", "-c", "-d"):
            stems.setdefault(n[:-2], set()).add(n[-1])
    for stem, tags in stems.items():
        want = {"b", "c"} if "-nt1" in stem or "-nt2" in stem else {"c"} if "-nt3" in stem or "-nt5" in stem else {"a", "b", "c"}
        assert tags >= want, (stem, tags)


@pytest.mark.parametrize("kind", KINDS)
def test_digests_equal_the_commit_before(lib, dev, kind):
    bad = []
    for name, outs in _outputs(kind).items():
        assert tool.unwritten(outs) == 0, (name, "unwritten outputs")
        if tool.digest(outs) != GOLDEN[name]:
            bad.append(name)
    assert not bad, f"{len(bad)} outputs differ from the commit before, the first: {bad[:6]}"
