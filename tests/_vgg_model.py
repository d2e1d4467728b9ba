"""The model the VGG engine tests run (tests/test_gpu_vgg.py) and the condition tests/test_vgg_encoder.py puts on it: a PoseRegressor
on a VGG encoder.  The convolutions keep the module's He initialisation (kaiming_normal, fan_out: activations stay O(1) through the
16 layers of vgg19 and inside the fp16-piece forms' stated range), their biases and every BatchNorm and GroupNorm get random
statistics and affines (tests/_densenet_model.py's draw), so a bias or a fold that is dropped shows."""
import copy

import torch

NAMES = ["vgg11", "vgg11_bn", "vgg13", "vgg13_bn", "vgg16", "vgg16_bn", "vgg19", "vgg19_bn"]
CONFIGS = {"vgg11": (1, 1, 2, 2, 2), "vgg13": (2, 2, 2, 2, 2), "vgg16": (2, 2, 3, 3, 3), "vgg19": (2, 2, 4, 4, 4)}      # convolutions per block
CHANNELS = (64, 128, 256, 512, 512)
# (encoder, B, H, W) of the engine tests: the 1/32 map is 2 x 3, and one odd-sized map of 3 x 5
ENGINE_CASES = [("vgg11", 2, 64, 96), ("vgg16_bn", 2, 64, 96), ("vgg19", 2, 64, 96), ("vgg13_bn", 1, 96, 160)]
SEED = 0      # picked on the CPU (tests/test_vgg_encoder.py: torch's own f32 forward stays within a quarter of the network bar)


def model(lib, encoder, seed=SEED):
    from fastposecnn_amd import config
    hp = config.INFERENCE()
    hp.RUNTIME_TIMING = False
    hp.ENCODER = encoder
    hp.PERFORM_AGGREGATION = False
    torch.manual_seed(seed)
    m = lib.pose_regressor.MODELS['PoseRegressor'].load_from_ckpt(None, hp)
    g = torch.Generator().manual_seed(seed + 1)
    for name, mod in m.named_modules():
        if isinstance(mod, torch.nn.Conv2d) and name.startswith("encoder.") and mod.bias is not None:
            mod.bias.data.copy_(torch.randn(mod.out_channels, generator=g) * 0.1)
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


def f32_errors(lib, encoder, x):
    """[(|f32 - float64|max, |float64|max)] of the six feature levels and the five logits: torch's own f32 CPU forward of the engine
    tests' model on frames x against its float64 forward."""
    m, hp = model(lib, encoder)
    hp.USE_NATIVE_ENGINE = False
    m64 = copy.deepcopy(m).double()
    m64.HPARAM = hp
    with torch.no_grad():
        got = list(m.encoder(x)) + list(m.pure_model_forward(x).values())
        ref = list(m64.encoder(x.double())) + list(m64.pure_model_forward(x.double()).values())
    assert len(ref) == 11
    return [((a.double() - r).abs().max().item(), r.abs().max().item()) for a, r in zip(got, ref)]
