"""The engine's host-side plan at 9 to 32 classes (no GPU): fpc_net_create* accept 2 <= classes <= 32, the parameter table
follows the model built from HPARAM.SELECTED_CLASSES, the head widths are {C, 4G, 3G, 3G} (G = C - 1), the workspace grows with
the class count, and a plan whose heads are wider than one 32-channel tile is created whatever FPC_MERGE_SPLIT says."""
import ctypes
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hiplib():
    from fastposecnn_amd import build, _native
    build.build()
    return _native.lib()


def _create(hiplib, classes, B=2, H=64, W=96):
    h = ctypes.c_void_p()
    return hiplib.fpc_net_create(b"resnet18", classes, B, H, W, ctypes.byref(h)), h


@pytest.mark.parametrize("classes", [9, 10, 17, 32])
def test_plan_is_created_and_its_parameter_table_is_the_models(hiplib, classes):
    import fastposecnn_amd.lib as L
    from fastposecnn_amd import config
    hp = config.INFERENCE()
    hp.ENCODER = "resnet18"
    hp.SELECTED_CLASSES = ["bg"] + ["obj%d" % i for i in range(1, classes)]
    m = L.pose_regressor.MODELS['PoseRegressor'].load_from_ckpt(None, hp)
    assert m.classes == classes
    sd = dict(m.named_parameters())
    sd.update(dict(m.named_buffers()))
    rc, h = _create(hiplib, classes)
    assert rc == 0
    try:
        n = hiplib.fpc_net_param_count(h)
        names = [hiplib.fpc_net_param_name(h, i).decode() for i in range(n)]
        assert len(set(names)) == n
        numel = {}
        for i, name in enumerate(names):
            assert name in sd, name
            numel[name] = hiplib.fpc_net_param_numel(h, i)
            assert sd[name].numel() == numel[name], name
        assert [k for k in sd if k not in set(names) and not k.endswith("num_batches_tracked")] == []
        G = classes - 1
        for head, ch in (("segmentation_head", classes), ("rotation_head", 4 * G), ("translation_head", 3 * G), ("scales_head", 3 * G)):
            assert numel[head + ".0.weight"] == ch * 128, head
            assert numel[head + ".0.bias"] == ch, head
    finally:
        hiplib.fpc_net_destroy(h)


def test_workspace_grows_with_the_class_count(hiplib):
    sizes = []
    for classes in (8, 9, 10, 32):
        rc, h = _create(hiplib, classes)
        assert rc == 0, classes
        sizes.append(hiplib.fpc_net_workspace_bytes(h))
        hiplib.fpc_net_destroy(h)
    assert sizes[0] < sizes[1] < sizes[2] < sizes[3], sizes


@pytest.mark.parametrize("classes", [1, 33, 64, 0, -3])
def test_counts_outside_2_to_32_are_refused(hiplib, classes):
    rc, _ = _create(hiplib, classes)
    assert rc == -1
    h = ctypes.c_void_p()
    r50 = (ctypes.c_int * 4)(3, 4, 6, 3)
    assert hiplib.fpc_net_create_encoder(4, r50, classes, 1, 64, 64, ctypes.byref(h)) == -1
    assert hiplib.fpc_net_create_encoder_ex(4, r50, 32, 4, classes, 1, 64, 64, ctypes.byref(h)) == -1
    assert hiplib.fpc_net_create_encoder_se(r50, 16, classes, 1, 64, 64, ctypes.byref(h)) == -1


def test_descriptor_plans_at_22_classes(hiplib):
    r50 = (ctypes.c_int * 4)(3, 4, 6, 3)
    G = 21
    for make in (lambda h: hiplib.fpc_net_create_encoder(4, r50, 22, 1, 64, 64, ctypes.byref(h)),            # Bottleneck
                 lambda h: hiplib.fpc_net_create_encoder_ex(4, r50, 32, 4, 22, 1, 64, 64, ctypes.byref(h)),  # ResNeXt
                 lambda h: hiplib.fpc_net_create_encoder_se(r50, 16, 22, 1, 64, 64, ctypes.byref(h))):       # SE-ResNet
        h = ctypes.c_void_p()
        assert make(h) == 0
        try:
            n = hiplib.fpc_net_param_count(h)
            numel = {hiplib.fpc_net_param_name(h, i).decode(): hiplib.fpc_net_param_numel(h, i) for i in range(n)}
            assert numel["segmentation_head.0.weight"] == 22 * 128 and numel["rotation_head.0.weight"] == 4 * G * 128
            assert numel["translation_head.0.bias"] == 3 * G and numel["scales_head.0.bias"] == 3 * G
            assert hiplib.fpc_net_workspace_bytes(h) > 0
        finally:
            hiplib.fpc_net_destroy(h)


def test_one_pass_switch_does_not_refuse_a_wide_plan(hiplib):
    """FPC_MERGE_SPLIT=0 selects the one-pass merge + head (heads of at most 32 channels); a 10-class plan (a 36-channel
    quaternion head) is created all the same and takes the two passes.  The value is read once per process: a fresh child."""
    code = ("import ctypes\n"
            "from fastposecnn_amd import _native\n"
            "L = _native.lib()\n"
            "h = ctypes.c_void_p()\n"
            "rc = L.fpc_net_create(b'resnet18', 10, 2, 64, 96, ctypes.byref(h))\n"
            "ws = L.fpc_net_workspace_bytes(h) if rc == 0 else -1\n"
            "print('RC', rc, ws)\n")
    env = dict(os.environ, FPC_MERGE_SPLIT="0", PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=REPO, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    tok = r.stdout.split()
    assert tok[0] == "RC" and int(tok[1]) == 0 and int(tok[2]) > 0, r.stdout
