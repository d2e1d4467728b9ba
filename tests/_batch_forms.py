"""What tests/test_gpu_batch_forms.py runs and what the host tests ask of it: per encoder family the frame size of the batch-32 engine
test, the three frames of the batch that are compared with float64, the 1x1 / 3x3 sites of the encoder read off the MODULE (forward
hooks on its convolutions: channels, and the map size as a stride of the input), and the kernel form each site takes at a batch
shape, from the library's own form functions (host arithmetic: fpc_dense_pw_form, fpc_dense_conv3x3_form, fpc_conv1x1_f32_form,
fpc_mbconv_pw_form).  The model and its draw are tests/_densenet_model.py's, which takes any encoder's name."""
import torch

BATCH = 32
FRAMES = (0, 17, 31)            # the first, an interior and the last frame of the batch: the ones held against float64
FULL = (480, 640)               # the workload's frame
# H, W of each family's batch: multiples of 32 with (H / 32)(W / 32) odd, at which the batch's sites take every form a site of
# 32 x 480 x 640 takes.  For mobilenet_v2 and efficientnet-b0 the smallest such frame (by pixels, then by H: smallest_shape below).
# For densenet121 a larger one, at which block 2 still runs the 3x3's tile form and block 3 the 1x1's 32 x 32 tiles as they do at
# full size, on maps (2288 and 572 pixels a frame) whose tiles straddle frames; 96 x 352 would reach those forms on block 1 alone,
# where a frame is a whole number of tiles.  tests/test_batch_forms_host.py holds both statements.
SHAPES = {"densenet121": (352, 416), "mobilenet_v2": (96, 352), "efficientnet-b0": (96, 352)}
CHANNELS = {"densenet121": (256, 512, 1024, 1024), "mobilenet_v2": (24, 32, 96, 1280), "efficientnet-b0": (24, 40, 112, 320)}


def sites(encoder):
    """[(name, kind, stride, Cin, Cout)] of every dense 1x1 convolution the encoder's forward runs on a map (kind "pw"), and of a
    DenseNet's 3x3 convolutions (kind "conv3"), in call order.  `stride` is the input's extent over the extent of the map the ENGINE
    runs the site on, read from one forward of a 64 x 64 frame: the module's own map, but for a DenseNet transition, whose 1x1 the
    plan runs behind the 2 x 2 mean (the same linear map on a quarter of the pixels), so its stride is twice the module's.  The gates'
    1x1 convolutions (on a 1 x 1 map whatever the frame: the gate kernel's, no 1x1 site) are left out by their input size at 64 x 64,
    where the deepest map is still 2 x 2."""
    from fastposecnn_amd.lib import backbone as bb
    found, hooks = [], []
    family = bb.encoder_family(encoder.name)
    in_transition = {id(m.conv) for m in encoder.modules() if type(m).__name__ == "Transition"}

    def hook(name):
        def fn(mod, args, out):
            h, w = args[0].shape[2:]
            k = mod.kernel_size
            if (h, w) == (1, 1) or mod.groups != 1:
                return
            assert h == w and 64 % h == 0, (name, h, w)
            stride = 64 // h * (2 if id(mod) in in_transition else 1)
            if k == (1, 1):
                found.append((name, "pw", stride, mod.in_channels, mod.out_channels))
            elif k == (3, 3) and family == "densenet" and mod.stride == (1, 1):
                found.append((name, "conv3", stride, mod.in_channels, mod.out_channels))
        return fn

    for name, mod in encoder.named_modules():
        if isinstance(mod, torch.nn.Conv2d):
            hooks.append(mod.register_forward_hook(hook(name)))
    was = encoder.training
    try:
        with torch.no_grad():
            encoder.eval()(torch.zeros(1, 3, 64, 64))
    finally:
        for h in hooks:
            h.remove()
        encoder.train(was)
    return found


def site_forms(L, encoder, B, H, W):
    """[(name, kind, M, Cin, Cout, form)] at a batch of B frames of H x W; a refused shape (-1) is an error."""
    from fastposecnn_amd.lib import backbone as bb
    assert H % 32 == 0 and W % 32 == 0
    family = bb.encoder_family(encoder.name)
    out = []
    for name, kind, stride, cin, cout in sites(encoder):
        h, w = H // stride, W // stride
        if kind == "conv3":
            assert (cin, cout) == (128, 32), name
            form = L.fpc_dense_conv3x3_form(B, h, w)
        elif family == "densenet":
            form = L.fpc_dense_pw_form(B * h * w, cin, cout)
        elif family == "efficientnet":
            form = L.fpc_mbconv_pw_form(B, h * w, cin, cout)
        else:
            assert family == "mobilenet_v2", family
            form = L.fpc_conv1x1_f32_form(B * h * w, cin, cout)
        assert form >= 0, (name, B, h, w, cin, cout)
        out.append((name, kind, B * h * w, cin, cout, form))
    return out


def form_set(rows):
    return {(kind, form) for _, kind, _, _, _, form in rows}


def smallest_shape(L, encoder, want):
    """The smallest H x W (multiples of 32, (H / 32)(W / 32) odd, H <= W <= 640, by pixels and then by H) at which the batch's sites
    take every (kind, form) of `want`; None where only a larger frame does."""
    cands = sorted((32 * a * 32 * b, 32 * a, 32 * b) for a in range(1, 21, 2) for b in range(a, 21, 2))
    for _, H, W in cands:
        if want <= form_set(site_forms(L, encoder, BATCH, H, W)):
            return H, W
    return None


def f32_errors(lib, encoder_name, x):
    """[(|f32 - float64|max, |float64|max)] of c2 .. c5 and the five logits: torch's own f32 CPU forward of the engine tests' model
    (tests/_densenet_model.py's draw) on frames x against its float64 forward."""
    import copy
    import _densenet_model as D
    m, hp = D.model(lib, encoder_name)
    hp.USE_NATIVE_ENGINE = False
    m64 = copy.deepcopy(m).double()
    m64.HPARAM = hp
    with torch.no_grad():
        got = list(m.encoder(x)[2:]) + list(m.pure_model_forward(x).values())
        ref = list(m64.encoder(x.double())[2:]) + list(m64.pure_model_forward(x.double()).values())
    assert len(ref) == 9
    return [((a.double() - r).abs().max().item(), r.abs().max().item()) for a, r in zip(got, ref)]


def frames(encoder_name):
    """The three frames of the batch that are held against float64, at the family's size."""
    from fastposecnn_amd import synth
    H, W = SHAPES[encoder_name]
    return torch.stack([synth.make_image(i, H, W) for i in FRAMES])
