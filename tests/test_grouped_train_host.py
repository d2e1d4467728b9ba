"""CPU-side checks of the native grouped-convolution training path (no GPU): the C ABI additions are declared and listed with the
right argument counts, the ABI version did not move, the switch is off by default, and CPU tensors never reach the kernels."""
import os
import re
import subprocess
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRIES = {      # name -> number of arguments in include/fpc.h
    "fpc_conv2d_grouped_dgrad_workspace_bytes": 2,
    "fpc_conv2d_grouped_dgrad": 12,
    "fpc_conv2d_grouped_wgrad_workspace_bytes": 5,
    "fpc_conv2d_grouped_wgrad": 15,
}


def _header():
    hdr = open(os.path.join(REPO, "include", "fpc.h")).read()
    return hdr, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_header_declares_the_four_entries():
    _, code = _header()
    for name, nargs in ENTRIES.items():
        m = re.search(r"\b(size_t|int)\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, f"{name} is not declared in include/fpc.h"
        assert len(m.group(2).split(",")) == nargs, (name, m.group(2))
        assert m.group(1) == ("size_t" if name.endswith("_bytes") else "int")


def test_abi_version_is_still_11():
    hdr, _ = _header()
    assert re.search(r"#define\s+FPC_ABI_VERSION\s+11\b", hdr)


def test_native_lists_the_four_entries():
    from fastposecnn_amd import _native
    for name, nargs in ENTRIES.items():
        assert name in _native.EXPORTED
        restype, argtypes = _native._SIGNATURES[name]
        assert len(argtypes) == nargs, (name, len(argtypes))


def test_switch_is_off_when_the_variable_is_unset():
    env = {k: v for k, v in os.environ.items() if k != "FPC_TRAIN_NATIVE_GROUPED"}
    code = ("from fastposecnn_amd.lib import train_conv\n"
            "assert train_conv.NATIVE_GROUPED is False\n"
            "assert all(train_conv.counters[k] == 0 for k in ('grouped_fwd_native', 'grouped_dgrad_native', 'grouped_wgrad_native'))\n")
    subprocess.run([sys.executable, "-c", code], cwd=REPO, env=env, check=True, timeout=300)
    env["FPC_TRAIN_NATIVE_GROUPED"] = "1"
    subprocess.run([sys.executable, "-c", code.replace("is False", "is True")], cwd=REPO, env=env, check=True, timeout=300)


def test_cpu_tensors_take_torch_with_the_switch_forced_on(monkeypatch):
    from fastposecnn_amd.lib import train_conv
    monkeypatch.setattr(train_conv, "NATIVE_GROUPED", True)
    monkeypatch.setattr(train_conv, "ENABLED", True)
    g = torch.Generator().manual_seed(0)
    x = torch.randn((2, 128, 9, 12), generator=g)
    w = torch.randn((128, 4, 3, 3), generator=g)
    b = torch.randn(128, generator=g)
    before = dict(train_conv.counters)
    for stride in (1, 2):
        assert torch.equal(train_conv.conv2d(x, w, b, stride, 1, 32), F.conv2d(x, w, b, stride, 1, 1, 32))
    assert dict(train_conv.counters) == before
