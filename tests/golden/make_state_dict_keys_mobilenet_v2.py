"""Writes state_dict_keys_mobilenet_v2.txt: the state-dict keys of torchvision.models.mobilenet_v2(...).features in order, from the
published definition alone (MobileNetV2.__init__ and InvertedResidual.__init__: Conv2dNormActivation = [conv (no bias), BatchNorm2d,
ReLU6]; a BatchNorm2d holds weight, bias, running_mean, running_var, num_batches_tracked).  It imports nothing from this package."""
import os

SETTING = [(1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1)]
BN = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")


def conv_bn(prefix):
    return [prefix + ".0.weight"] + [f"{prefix}.1.{k}" for k in BN]


def keys():
    out = conv_bn("features.0")
    idx = 1
    for t, _, n, _ in SETTING:
        for _ in range(n):
            p = f"features.{idx}.conv"
            k = 0
            if t != 1:
                out += conv_bn(f"{p}.0")
                k = 1
            out += conv_bn(f"{p}.{k}")
            out += [f"{p}.{k + 1}.weight"] + [f"{p}.{k + 2}.{b}" for b in BN]
            idx += 1
    return out + conv_bn(f"features.{idx}")


if __name__ == "__main__":
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "state_dict_keys_mobilenet_v2.txt"), "w") as f:
        f.write("\n".join(keys()) + "\n")
