"""The model the DenseNet engine tests run (tests/test_gpu_densenet.py) and the condition tests/test_densenet_encoder.py puts on it:
a PoseRegressor on a DenseNet encoder with random BatchNorm and GroupNorm statistics and affines, test_gpu_efficientnet_b0.py's draw."""
import torch

SMALL_SHAPES = [(2, 64, 96), (1, 96, 64), (3, 32, 32)]      # (B, H, W) of the engine tests; at 32 x 32 block 4 runs on a 1 x 1 map


def model(lib, encoder, seed=0):
    from fastposecnn_amd import config
    hp = config.INFERENCE()
    hp.RUNTIME_TIMING = False
    hp.ENCODER = encoder
    hp.PERFORM_AGGREGATION = False
    torch.manual_seed(seed)
    m = lib.pose_regressor.MODELS['PoseRegressor'].load_from_ckpt(None, hp)
    g = torch.Generator().manual_seed(seed + 1)
    for name, mod in m.named_modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
            mod.running_var.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
            mod.weight.data.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
            mod.bias.data.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
        if isinstance(mod, torch.nn.GroupNorm):
            mod.weight.data.copy_(torch.rand(mod.num_channels, generator=g) + 0.5)
            mod.bias.data.copy_(torch.randn(mod.num_channels, generator=g) * 0.1)
    return m.eval(), hp


def images(B, H, W):
    from fastposecnn_amd import synth
    return torch.stack([synth.make_image(i, H, W) for i in range(B)])
