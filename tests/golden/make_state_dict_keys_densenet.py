"""Writes state_dict_keys_densenet{121,169,201}.txt: the state-dict keys of smp's DenseNetEncoder in order, from the published
definition alone (torchvision.models.densenet: DenseNet.__init__ registers features.conv0, norm0, relu0, pool0, then per block
denseblockN — a _DenseBlock of denselayer1 .. L, each _DenseLayer registering norm1, relu1, conv1, norm2, relu2, conv2 — and, behind
every block but the last, transitionN — norm, relu, conv, pool — then norm5, then the classifier, which smp deletes; no convolution has
a bias; a BatchNorm2d holds weight, bias, running_mean, running_var, num_batches_tracked).  It imports nothing from this package."""
import os

BLOCKS = {"densenet121": (6, 12, 24, 16), "densenet169": (6, 12, 32, 32), "densenet201": (6, 12, 48, 32)}
BN = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")


def bn(prefix):
    return [f"{prefix}.{k}" for k in BN]


def keys(name):
    out = ["features.conv0.weight"] + bn("features.norm0")
    blocks = BLOCKS[name]
    for b, layers in enumerate(blocks, 1):
        for j in range(1, layers + 1):
            p = f"features.denseblock{b}.denselayer{j}"
            out += bn(f"{p}.norm1") + [f"{p}.conv1.weight"] + bn(f"{p}.norm2") + [f"{p}.conv2.weight"]
        if b < len(blocks):
            out += bn(f"features.transition{b}.norm") + [f"features.transition{b}.conv.weight"]
    return out + bn("features.norm5")


if __name__ == "__main__":
    for name in BLOCKS:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), f"state_dict_keys_{name}.txt"), "w") as f:
            f.write("\n".join(keys(name)) + "\n")
