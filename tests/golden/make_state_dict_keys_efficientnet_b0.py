"""Writes state_dict_keys_efficientnet_b0.txt: the state-dict keys of smp's EfficientNetEncoder("efficientnet-b0") in order, from the
published definition alone (efficientnet_pytorch: EfficientNet.__init__ registers _conv_stem, _bn0, _blocks, _conv_head, _bn1, _fc —
smp deletes _fc only —; MBConvBlock.__init__ registers _expand_conv and _bn0 (not where expand_ratio = 1), _depthwise_conv, _bn1,
_se_reduce, _se_expand (both with bias), _project_conv, _bn2; no other convolution has a bias; a BatchNorm2d holds weight, bias,
running_mean, running_var, num_batches_tracked).  It imports nothing from this package."""
import os

# (repeat, kernel, stride, expand ratio, input, output)
BLOCKS = [(1, 3, 1, 1, 32, 16), (2, 3, 2, 6, 16, 24), (2, 5, 2, 6, 24, 40), (3, 3, 2, 6, 40, 80), (3, 5, 1, 6, 80, 112),
          (4, 5, 2, 6, 112, 192), (1, 3, 1, 6, 192, 320)]
BN = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")


def bn(prefix):
    return [f"{prefix}.{k}" for k in BN]


def keys():
    out = ["_conv_stem.weight"] + bn("_bn0")
    idx = 0
    for repeat, _, _, expand, _, _ in BLOCKS:
        for _ in range(repeat):
            p = f"_blocks.{idx}"
            if expand != 1:
                out += [f"{p}._expand_conv.weight"] + bn(f"{p}._bn0")
            out += [f"{p}._depthwise_conv.weight"] + bn(f"{p}._bn1")
            out += [f"{p}._se_reduce.weight", f"{p}._se_reduce.bias", f"{p}._se_expand.weight", f"{p}._se_expand.bias"]
            out += [f"{p}._project_conv.weight"] + bn(f"{p}._bn2")
            idx += 1
    return out + ["_conv_head.weight"] + bn("_bn1")


if __name__ == "__main__":
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "state_dict_keys_efficientnet_b0.txt"), "w") as f:
        f.write("\n".join(keys()) + "\n")
