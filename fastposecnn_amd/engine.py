"""Host side of the backbone engine (`fpc_net_*` in include/fpc.h, csrc/net.hip).

A `NetEngine` binds one PoseRegressor's parameters to a native plan for a fixed (B, H, W): the C
side repacks the weights once (OHWI, padded; BatchNorm folded), then every `forward` is a single C
call that enqueues the whole frame's kernels on torch's current stream.  torch only owns the
memory: parameters, the workspace and the output tensors.

A plan takes 2 to 32 classes (background included), like every later stage; the library refuses more
(`fpc_net_create*` -> FPC_EINVAL, raised by `nat.check`).
"""
import ctypes
import operator

import torch

from fastposecnn_amd import _native as nat


_DATA_PTR = torch.Tensor.data_ptr
_VERSION = operator.attrgetter('_version')

class NetEngine:

    def __init__(self, model, B, H, W, device, autotune=True, tune_mode=0, graph=False, split_precision=False):
        L = nat.lib()
        self._lib = L
        self.B, self.H, self.W, self.device = B, H, W, device
        self.classes = model.classes
        h = ctypes.c_void_p()
        from fastposecnn_amd.lib import backbone
        name = model.encoder.name
        by_name = backbone.encoder_family(name) in ("mobilenet_v2", "efficientnet", "densenet", "vgg")      # a plan fpc_net_create builds by name, no descriptor
        block, layers = (0, [0] * 4) if by_name else backbone.encoder_layout(name)
        groups, width = (1, 64) if by_name else backbone.encoder_groups(name)
        reduction = 0 if by_name else backbone.encoder_reduction(name)
        arr, tail = (ctypes.c_int * 4)(*layers), (self.classes, B, H, W, ctypes.byref(h))
        if by_name:
            nat.check(L.fpc_net_create(name.encode(), *tail), "fpc_net_create")
        elif reduction:     # SE-ResNet: the Bottleneck with the stride on conv1 and the squeeze-and-excitation gate
            nat.check(L.fpc_net_create_encoder_se(arr, reduction, *tail), "fpc_net_create_encoder_se")
        elif groups > 1:    # ResNeXt: Bottleneck with a grouped conv2
            nat.check(L.fpc_net_create_encoder_ex(block, arr, groups, width, *tail), "fpc_net_create_encoder_ex")
        elif block == 1:    # the named nets, as always
            nat.check(L.fpc_net_create(name.encode(), *tail), "fpc_net_create")
        else:               # Bottleneck encoders by their descriptor
            nat.check(L.fpc_net_create_encoder(block, arr, *tail), "fpc_net_create_encoder")
        self._h = h
        self._names = [L.fpc_net_param_name(h, i).decode() for i in range(L.fpc_net_param_count(h))]
        nbytes = L.fpc_net_workspace_bytes(h)
        with torch.cuda.device(device):
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
            assert self._ws.data_ptr() % 256 == 0
        self.reloads = 0
        self.generation = 0          # the owner's count of unversioned writes when this plan was last bound (pose_regressor.py)
        self.guard_forwards = 0      # forwards this plan ran under HPARAM.ENGINE_RANGE_GUARD (pose_regressor.py: which of them survey)
        self.bind(model)
        if split_precision:
            nat.check(L.fpc_net_set_split_precision(h, int(split_precision)), "fpc_net_set_split_precision")
        if autotune:
            # one (discarded) forward that times every candidate tiling per convolution on this device
            nat.check(L.fpc_net_autotune_next(h, int(tune_mode)), "fpc_net_autotune_next")
            self.forward(torch.zeros((B, 3, H, W), dtype=torch.float32, device=device), want_logits=False)
        if graph:
            nat.check(L.fpc_net_set_graph(h, 1), "fpc_net_set_graph")

    def bind(self, model):
        """(Re)pack the model's current parameters into the plan's workspace.  The tuned tilings are kept; a
        recorded graph is dropped by the library and re-captured on the next forward."""
        L, h, device = self._lib, self._h, self.device
        tensors = dict(model.named_parameters())
        tensors.update(dict(model.named_buffers()))
        params = []                 # keeps the tensors alive: the plan reads some of them in place
        for i, name in enumerate(self._names):
            if name not in tensors:
                raise RuntimeError(f"fastposecnn_amd: the model has no parameter {name!r} (smp naming expected)")
            t = tensors[name]
            if t.device != device or t.dtype != torch.float32 or not t.is_contiguous():
                raise RuntimeError(f"fastposecnn_amd: parameter {name!r} must be a contiguous f32 tensor on {device}")
            if t.numel() != L.fpc_net_param_numel(h, i):
                raise RuntimeError(f"fastposecnn_amd: parameter {name!r} has {t.numel()} elements, expected "
                                   f"{L.fpc_net_param_numel(h, i)}")
            params.append(t)
        self._params = params
        n = len(params)
        ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in params])
        with torch.cuda.device(device):
            nat.check(L.fpc_net_load_params(h, ptrs, n, self._ws.data_ptr(), self._ws.numel(), nat.stream()),
                      "fpc_net_load_params")
        self._stamp = self._fingerprint()
        self.reloads += 1

    def _fingerprint(self):
        # (storage address, in-place version) of every bound tensor: changes on load_state_dict (of the model or of
        # any sub-module), optimizer / EMA steps, p.copy_(), .to() — anything but a write through `p.data`, which
        # PyTorch itself does not version
        # (two C-level maps: a Python-level loop over the ~200 tensors cost 35 us of every streamed frame's 390 on the host)
        return (tuple(map(_DATA_PTR, self._params)), tuple(map(_VERSION, self._params)))

    def stale(self):
        """True when a bound parameter was rewritten or replaced since it was packed (packed conv weights and folded
        BatchNorm are a snapshot; biases / GroupNorm / head weights are read in place)."""
        return self._fingerprint() != self._stamp

    def conv_plans(self):
        out = []
        buf = (ctypes.c_int * 5)()
        for i in range(self._lib.fpc_net_conv_count(self._h)):
            self._lib.fpc_net_conv_plan(self._h, i, buf)
            out.append(tuple(buf))
        return out

    def copy_plans_from(self, other):
        """Run this engine on the plans `other` (same network and frame size, another batch) was autotuned to; the range guard's
        demotions and fallback plans come along."""
        nat.check(self._lib.fpc_net_copy_plans(self._h, other._h), "fpc_net_copy_plans")

    def force_winograd(self, form):
        """Every 3x3 / stride-1 site on Winograd form `form` (8 = fp16 x 2 pieces); returns the number of sites changed."""
        rc = self._lib.fpc_net_force_winograd(self._h, int(form))
        if rc < 0:
            nat.check(rc, "fpc_net_force_winograd")
        return rc

    def force_fold(self, on):
        """s2.0 with the FPN p2 level folded in (on = 1) or on plain form -9 (on = 0); returns 1 when the plan changed."""
        rc = self._lib.fpc_net_force_fold(self._h, int(on))
        if rc < 0:
            nat.check(rc, "fpc_net_force_fold")
        return rc

    def force_direct_h3(self, on):
        """Every site with the three-product direct form's image on that form (on = 1) or back on the f32 tiling (on = 0);
        returns the number of sites changed."""
        rc = self._lib.fpc_net_force_direct_h3(self._h, int(on))
        if rc < 0:
            nat.check(rc, "fpc_net_force_direct_h3")
        return rc

    def force_stem_pool(self, on):
        """The stem and its max-pool as one launch (on = 1, split level 3) or back on stem kernel + max-pool (on = 0); returns 1
        when the plan changed."""
        rc = self._lib.fpc_net_force_stem_pool(self._h, int(on))
        if rc < 0:
            nat.check(rc, "fpc_net_force_stem_pool")
        return rc

    def survey(self, x, want_logits=True):
        """One forward that also surveys the activations (fpc_net_survey_next): in front of every convolution site's launch one pass
        over what the site's current plan reads.  Returns (logits, cat, records): the outputs of an ordinary forward, bit for bit, and
        an int64 CPU tensor [sites, 4] — per site the bits of max |x| over the finite elements, the number of non-finite elements,
        the number of elements visited (saturating at 2^32 - 1; 0: the site did not run), and a reserved word.  It changes no plan;
        it reads the records back, so it synchronises the stream."""
        if tuple(x.shape) != (self.B, 3, self.H, self.W) or x.device != self.device:      # before arming: forward() would refuse it
            raise RuntimeError("NetEngine.survey: input shape / device does not match the plan")
        sites = self._lib.fpc_net_conv_count(self._h)
        with torch.cuda.device(self.device):
            rec = torch.zeros((sites, 4), dtype=torch.int32, device=self.device)
            nat.check(self._lib.fpc_net_survey_next(self._h, rec.data_ptr(), sites), "fpc_net_survey_next")
        try:
            logits, cat = self.forward(x, want_logits=want_logits)
        finally:      # the library disarms when its forward returns; this covers a forward that never reached it
            self._lib.fpc_net_survey_next(self._h, None, sites)
        return logits, cat, rec.cpu().to(torch.int64) & 0xFFFFFFFF

    @staticmethod
    def record_max(records):
        """max |x| of every record of `survey` as float32 values [sites]."""
        return (records[:, 0] & 0xFFFFFFFF).to(torch.int32).view(torch.float32) if records.dtype == torch.int64 \
            else records[:, 0].contiguous().view(torch.float32)

    def guard_ranges(self, records, lo=2.0 ** -2, hi=2.0 ** 14):
        """Demote every site on an fp16-piece form whose record (of `survey`) shows a non-finite element, max |x| >= hi or
        0 < max |x| < lo to its best range-free plan (fpc_net_guard_ranges; host arithmetic).  Returns the indices of the sites
        demoted by this call; they stay demoted (`guarded`)."""
        sites = self._lib.fpc_net_conv_count(self._h)
        flat = [int(v) & 0xFFFFFFFF for v in records.reshape(-1).tolist()]
        if len(flat) != 4 * sites:
            raise RuntimeError("NetEngine.guard_ranges: records must be [sites, 4]")
        before = set(self.guarded())
        rc = self._lib.fpc_net_guard_ranges(self._h, (ctypes.c_uint32 * len(flat))(*flat), sites, float(lo), float(hi))
        if rc < 0:
            nat.check(rc, "fpc_net_guard_ranges")
        return [i for i in self.guarded() if i not in before]

    def guarded(self):
        """The sites that stand demoted by `guard_ranges`."""
        return [i for i in range(self._lib.fpc_net_conv_count(self._h)) if self._lib.fpc_net_guarded(self._h, i)]

    def graph_recorded(self):
        return bool(self._lib.fpc_net_graph_recorded(self._h))

    def set_wino_pack(self, on):
        """Form-9 Winograd launches cut their tile patches out of canvas rows of several frames where that needs fewer patches
        (on = 1, the library's default) or keep one frame per patch row (on = 0).  The plans do not change."""
        nat.check(self._lib.fpc_net_set_wino_pack(self._h, int(on)), "fpc_net_set_wino_pack")

    def set_wino_orient(self, on):
        """Form-9 Winograd launches run transposed at the sites whose shape asks for it (on = 1, the library's default: tile columns a
        multiple of 8, tile rows not) or all in the stored orientation (on = 0).  Repacks those sites' weight images; the plans and
        the workspace do not change."""
        nat.check(self._lib.fpc_net_set_wino_orient(self._h, int(on)), "fpc_net_set_wino_orient")

    def set_wino_xshare(self, on):
        """Packed form-9 Winograd launches use the x-shared tile map where the frame's tile-column count is even (on = 1, the
        library's default) or the row-split map everywhere (on = 0).  The same results bit for bit; plans and images do not change."""
        nat.check(self._lib.fpc_net_set_wino_xshare(self._h, int(on)), "fpc_net_set_wino_xshare")

    def set_wino_fast_exit(self, on):
        """Workgroups of the four-wave Winograd kernels whose patch lies wholly inside its frame leave through the fast exit, which
        tests no pixel (on = 1, the library's default), or all through the general one (on = 0).  The same results bit for bit."""
        nat.check(self._lib.fpc_net_set_wino_fast_exit(self._h, int(on)), "fpc_net_set_wino_fast_exit")

    def set_fold_idle_row(self, on):
        """In the p3 phase of the folded s2.0 the wave of the zero transform row only stages its share of the input (on = 1, the
        library's default), or runs the phase on its zeros like the other three (on = 0).  The same results bit for bit."""
        nat.check(self._lib.fpc_net_set_fold_idle_row(self._h, int(on)), "fpc_net_set_fold_idle_row")

    def wino_blocks(self):
        """Workgroups of all form-9 launches of the last forward that launched its kernels."""
        return int(self._lib.fpc_net_wino_blocks(self._h))

    def force_pointwise(self, on):
        """Every eligible 1x1 site on k_conv1x1 (on = 1) or back on k_conv_igemm (on = 0); returns the number of sites changed."""
        rc = self._lib.fpc_net_force_pointwise(self._h, int(on))
        if rc < 0:
            nat.check(rc, "fpc_net_force_pointwise")
        return rc

    def flops(self):
        """(direct-convolution FLOP, FLOP the current plans execute, Winograd share) of one forward over the batch."""
        buf = (ctypes.c_double * 3)()
        nat.check(self._lib.fpc_net_flops(self._h, buf), "fpc_net_flops")
        return tuple(buf)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._lib.fpc_net_destroy(h)
            self._h = None

    def forward(self, x, want_logits=True):
        """x f32 [B,3,H,W] -> (logits dict | None, categorical dict incl. 'mask')."""
        B, H, W, C, dev = self.B, self.H, self.W, self.classes, self.device
        G = C - 1
        if tuple(x.shape) != (B, 3, H, W) or x.device != dev:
            raise RuntimeError("NetEngine.forward: input shape / device does not match the plan")
        if x.dtype != torch.float32 or not x.is_contiguous():
            x = x.float().contiguous()
        f32 = dict(dtype=torch.float32, device=dev)
        logits = None
        lp = [None] * 5
        if want_logits:
            logits = {'mask': torch.empty((B, C, H, W), **f32), 'quaternion': torch.empty((B, 4 * G, H, W), **f32),
                      'scales': torch.empty((B, 3 * G, H, W), **f32), 'xy': torch.empty((B, 2 * G, H, W), **f32),
                      'z': torch.empty((B, G, H, W), **f32)}
            lp = [logits[k].data_ptr() for k in ('mask', 'quaternion', 'scales', 'xy', 'z')]
        cat = {'mask': torch.empty((B, H, W), dtype=torch.int64, device=dev),
               'quaternion': torch.empty((B, 4, H, W), **f32), 'scales': torch.empty((B, 3, H, W), **f32),
               'xy': torch.empty((B, 2, H, W), **f32), 'z': torch.empty((B, H, W), **f32)}
        # the foreground of the class mask also as bit words (1/64 of its bytes): the connected-component labelling reads
        # those instead of the i64 mask; they ride on the mask tensor (aggregation_layer.fg_bits_of), not in the dict
        bits = None
        if W % 64 == 0 and self._lib.fpc_cc_bits_supported(B, H, W):
            bits = torch.empty((B, self._lib.fpc_mask_bits_words(H, W)), dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            nat.check(self._lib.fpc_net_forward_bits(self._h, x.data_ptr(), *lp, cat['mask'].data_ptr(),
                                                     cat['quaternion'].data_ptr(), cat['scales'].data_ptr(),
                                                     cat['xy'].data_ptr(), cat['z'].data_ptr(), nat.ptr(bits), nat.stream()),
                      "fpc_net_forward_bits")
        if bits is not None:
            cat['mask']._fpc_fg_bits = (bits, cat['mask']._version)
        return logits, cat

    def tensor(self, name):
        """Intermediate activation as an NHWC view into the workspace (tests)."""
        p = ctypes.c_void_p()
        H, W, C = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        nat.check(self._lib.fpc_net_tensor(self._h, name.encode(), ctypes.byref(p), ctypes.byref(H), ctypes.byref(W),
                                           ctypes.byref(C)), "fpc_net_tensor")
        off = p.value - self._ws.data_ptr()
        n = self.B * H.value * W.value * C.value
        return self._ws[off:off + 4 * n].view(torch.float32).view(self.B, H.value, W.value, C.value)
