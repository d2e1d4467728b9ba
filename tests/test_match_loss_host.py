"""CPU-side checks of the device matching and matched losses (csrc/match_loss.hip): the ABI declarations, the argument
checks that run before any launch, and the paths of matching.batchwise_find_matches_device / loss.total_loss_device that
the host decides without device data."""
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fpc_match_assign", "fpc_matched_losses", "fpc_matched_losses_backward")


def test_entries_are_declared_and_bound():
    from fastposecnn_amd import _native
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "fpc.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fpc_[a-z0-9_]+)\s*\(", hdr))
    for name in NAMES:
        assert name in _native._SIGNATURES and name in declared, name
    limit = int(re.search(r"#define FPC_MATCH_MAX_INSTANCES (\d+)", hdr).group(1))
    import fastposecnn_amd.lib  # noqa: F401
    import matching as mg
    assert limit >= 1024 and mg.MAX_INSTANCES == limit
    assert re.search(r"#define FPC_ABI_VERSION 11\b", hdr)


def test_none_cases_need_no_library(monkeypatch):
    import fastposecnn_amd.lib  # noqa: F401
    import matching as mg
    from fastposecnn_amd import _native

    def no_library():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_native, "lib", no_library)
    some = {"class_ids": torch.ones(3, dtype=torch.int64), "instance_masks": torch.zeros(3, 4, 4)}
    empty = {k: v[:0] for k, v in some.items()}
    assert mg.batchwise_find_matches_device(None, some) is None
    assert mg.batchwise_find_matches_device(some, {}) is None
    assert mg.batchwise_find_matches_device(empty, some) is None
    assert mg.batchwise_find_matches_device(some, empty) is None


def test_cpu_tensors_are_refused():
    import fastposecnn_amd.lib  # noqa: F401
    import matching as mg
    some = {"class_ids": torch.ones(3, dtype=torch.int64), "instance_masks": torch.zeros(3, 4, 4)}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mg.batchwise_find_matches_device(some, some)


def test_match_assign_rejects_bad_arguments_before_launching():
    from fastposecnn_amd import build, _native
    import fastposecnn_amd.lib  # noqa: F401
    import matching as mg
    build.build()
    L = _native.lib()
    p = 4096          # never dereferenced: every call below must return before a launch
    assert L.fpc_match_assign(p, p, p, mg.MAX_INSTANCES + 1, 3, p, p, p, None) == -1
    assert L.fpc_match_assign(p, p, p, 3, mg.MAX_INSTANCES + 1, p, p, p, None) == -1
    assert L.fpc_match_assign(None, p, p, 2, 2, p, p, p, None) == -1
    assert L.fpc_match_assign(p, p, p, -1, 2, p, p, p, None) == -1
    assert L.fpc_match_assign(None, None, None, 0, 5, None, None, None, None) == 0      # n1 == 0: a no-op


def test_total_loss_device_without_matches_is_total_loss():
    """The case of test_eval_losses.py::test_total_loss_arithmetic."""
    import fastposecnn_amd.lib  # noqa: F401
    import loss as L
    crit = L.head_training_criterion()
    torch.manual_seed(0)
    ml = torch.randn(1, 7, 6, 8, requires_grad=True)
    out = {"logits": {"mask": ml}}
    batch = {"mask": torch.randint(0, 7, (1, 6, 8))}
    want, want_rep = L.total_loss(crit, out, batch, None)
    before = dict(L.counters)
    got, got_rep = L.total_loss_device(crit, out, batch, None)
    assert L.counters == before                  # neither path is counted: there is nothing to match
    assert torch.equal(got, want) and list(got_rep) == list(want_rep)
    for task, d in want_rep.items():
        assert list(got_rep[task]) == list(d)
        for k, v in d.items():
            g = got_rep[task][k]
            assert g.dtype == v.dtype and (torch.equal(g, v) or (bool(torch.isnan(g)) and bool(torch.isnan(v)))), (task, k)
    got.backward()
    assert ml.grad is not None and torch.isfinite(ml.grad).all()
