"""The input side of the inference path on the device: colour frame -> network tensor.

Mirrors what F/tools/dataset.py does per sample on the host in numpy, for frames that are already decoded:

    NOCSDataset.__getitem__ (:249-262)   preprocessing_fn(image) -> transpose(2,0,1) -> / max|.| -> img_as_float32
    my_collate_fn (:453-529)             stack the per-sample arrays, concatenate agg_data, add 'sample_ids'

`preprocess_frames` runs the first chain on the GPU (fpc_preprocess_u8: two kernels, bit-identical to the numpy
chain), `FrameUploader` owns the pinned staging buffers and the host->device copy stream in front of it, and
`my_collate_fn` keeps the reference's collate semantics for callers that bring their own samples.

File decoding (:158-176: skimage.io.imread of `*_color.png` / `*_mask.png`, cv2.imread of `*_depth.png`) is native too
(csrc/png_decode.hip over zlib; libpng's headers are not in the image): `imread_png` returns what imread returns,
`read_frame_files` mirrors the first lines of `__getitem__` (image, mask with background 255 -> 0, standardised depth),
and `FrameUploader.upload_png` decodes a batch of colour files straight into its pinned staging slot on a few host
threads.  Opt-in, `upload_png(..., decode="device")` of both uploaders leaves the host the container walk and one copy of
the compressed bytes: csrc/png_device.hip inflates and un-filters on the uploader's stream.

The ground-truth half of a dataset item (round 4, SURVEY.md 8f rank 3 remainder): `NOCSDataset` / `CAMERADataset` /
`REALDataset` mirror F/tools/dataset.py:99-434 — the directory walk for `*_color.png` frames with wanted instances
(:278-357), `__getitem__` (:138-272: file reads, `*_meta+.json`, distractor and class filtering of the instance mask, the
per-instance ground truth of `generate_agg_data` :373-434, z <= 0 rejection, class mask, preprocessing chain) — and return the
reference's sample dict key for key (pinned by tests/golden/nocs_sample.npz, which the reference's own class wrote:
oracle/gen_golden.py).  `evaluate.py:148` and the training step feed `batchwise_find_matches` from exactly this dict.
Augmentation is not mirrored (the reference has it commented out, :239-242).

The same ground truth built on the device: `NOCSDataset.gt_item` is the half of `__getitem__` that the side file alone
decides, `GroundTruthUploader` uploads the instance-id masks beside it and has fpc_gt_build (csrc/gt_build.hip) write the
class mask and the per-instance planes where `my_collate_fn` would copy them to; `build_gt_host` states in numpy what that
kernel computes.  `__getitem__` and `my_collate_fn` are unchanged.
"""
import ctypes
import os
import pathlib

import numpy as np
import torch

from fastposecnn_amd import _native as nat
from fastposecnn_amd.tools import data_manipulation as dm
from fastposecnn_amd.tools import json_tools as jt

# segmentation_models_pytorch's preprocessing parameters for the resnet encoders, mobilenet_v2, efficientnet-b0, densenet121 / 169 / 201 and the VGGs with "imagenet" weights
# (smp.encoders.get_preprocessing_params; upstream package, absent from the reference tree): RGB, range [0, 1]
IMAGENET_PARAMS = {"input_space": "RGB", "input_range": [0, 1], "mean": [0.485, 0.456, 0.406],
                   "std": [0.229, 0.224, 0.225]}

VGG_NAMES = tuple(n + s for n in ("vgg11", "vgg13", "vgg16", "vgg19") for s in ("", "_bn"))      # (exact names: no prefix match)


def get_preprocessing_params(encoder_name="resnet18", pretrained="imagenet"):
    """smp.encoders.get_preprocessing_params for the encoders this package builds (lib/backbone.py)."""
    if pretrained != "imagenet" or not str(encoder_name).startswith(("resnet", "resnext", "se_resnet", "mobilenet_v2", "efficientnet-b0", "densenet121", "densenet169", "densenet201")) \
            and str(encoder_name) not in VGG_NAMES:
        raise ValueError("no preprocessing parameters for encoder %r / weights %r" % (encoder_name, pretrained))
    return {k: (list(v) if isinstance(v, list) else v) for k, v in IMAGENET_PARAMS.items()}


def preprocess_frames(images_u8, params=None, out=None):
    """images_u8: uint8 CUDA tensor [B,H,W,3] (or [H,W,3]) as skimage.io.imread returns frames ->
    f32 [B,3,H,W] ([3,H,W]), bit-identical to F/tools/dataset.py:249-262 applied to each frame."""
    params = params or IMAGENET_PARAMS
    if params.get("input_space", "RGB") != "RGB":
        raise ValueError("only RGB input space (the resnet encoders)")
    nat.require_gpu(images_u8, what="preprocess_frames")
    if images_u8.dtype != torch.uint8:
        # dataset.py:256 skips the max-normalisation for uint8 only because a preprocessing_fn always ran before;
        # float input has no reference behaviour to mirror here
        raise TypeError("preprocess_frames takes the decoded uint8 frame")
    single = images_u8.dim() == 3
    x = images_u8.unsqueeze(0) if single else images_u8
    if x.dim() != 4 or x.shape[-1] != 3:
        raise ValueError("expected [B,H,W,3] uint8, got %s" % (tuple(images_u8.shape),))
    x = x.contiguous()
    B, H, W, _ = x.shape
    dev = x.device
    if out is None:
        out = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
    elif out.shape != (B, 3, H, W) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        raise ValueError("out must be a contiguous f32 [B,3,H,W] tensor on the frames' device")
    mean = (ctypes.c_double * 3)(*params["mean"])
    std = (ctypes.c_double * 3)(*params["std"])
    rng = params.get("input_range")
    range01 = 1 if (rng is not None and rng[1] == 1) else 0
    L = nat.lib()
    with torch.cuda.device(dev):
        ws = nat.workspace("pre", dev, L.fpc_preprocess_workspace_bytes(B))
        nat.check(L.fpc_preprocess_u8(nat.ptr(x), B, H, W, mean, std, range01, nat.ptr(out), nat.ptr(ws), ws.numel(),
                                      nat.stream()), "fpc_preprocess_u8")
    return out[0] if single else out


def imread_png(src, rgb8=False):
    """A PNG file (path) or its bytes -> numpy array as skimage.io.imread / cv2.imread(path, -1) return it: [H,W] or
    [H,W,C] uint8, uint16 for 16-bit files, palette expanded to RGB (channel order R,G,B,A: cv2 would give B,G,R).
    rgb8=True: always [H,W,3] uint8 (grey replicated, alpha dropped)."""
    data = src if isinstance(src, (bytes, bytearray, memoryview)) else open(os.fspath(src), "rb").read()
    buf = np.frombuffer(data, dtype=np.uint8)
    L = nat.lib()
    info = (ctypes.c_int32 * 5)()
    nat.check(L.fpc_png_info(buf.ctypes.data, buf.size, info), "fpc_png_info")
    W, H, depth, ctype, C = (int(v) for v in info)
    if rgb8:
        out = np.empty((H, W, 3), np.uint8)
        nat.check(L.fpc_png_decode(buf.ctypes.data, buf.size, out.ctypes.data, out.nbytes, 3), "fpc_png_decode")
        return out
    out = np.empty((H, W, C), np.uint16 if depth == 16 else np.uint8)
    nat.check(L.fpc_png_decode(buf.ctypes.data, buf.size, out.ctypes.data, out.nbytes, 0), "fpc_png_decode")
    return out[:, :, 0] if C == 1 else out


def standardize_depth(depth_rgb_or_u16):
    """F/tools/data_manipulation.py:153-163 for an array in R,G,B order (the reference sees cv2's B,G,R: its channels
    [1], [2] are G, R): a 3-channel file encodes depth as G * 256 + R; a 16-bit grey file is the depth."""
    d = depth_rgb_or_u16
    if d.ndim == 3:
        return (d[:, :, 1].astype(np.uint16) * np.uint16(256) + d[:, :, 0].astype(np.uint16)).astype(np.uint16)
    if d.ndim == 2 and d.dtype == np.uint16:
        return d
    raise ValueError("unsupported depth image")


def read_frame_files(color_path, camera=True):
    """The file reads of NOCSDataset.__getitem__ (F/tools/dataset.py:158-176): {'image': u8 [H,W,3|4] as stored,
    'mask': float64 [H,W] with the background 255 set to 0 (first channel of the CAMERA set's RGBA masks),
    'depth': uint16 [H,W]}.  Missing mask / depth files are left out."""
    color_path = os.fspath(color_path)
    out = {"image": imread_png(color_path)}
    mask_fp = color_path.replace("_color.png", "_mask.png")
    if os.path.exists(mask_fp):
        m = imread_png(mask_fp)
        m = (m[:, :, 0] if (camera and m.ndim == 3) else m).astype("float")
        m[m == 255] = 0
        out["mask"] = m
    depth_fp = color_path.replace("_color.png", "_depth.png")
    if os.path.exists(depth_fp):
        out["depth"] = standardize_depth(imread_png(depth_fp))
    return out


class _DevicePngDecoder:
    """One slot of the device decode path (csrc/png_device.hip): a pinned staging buffer for the COMPRESSED bytes of up to `n`
    files, their descriptors and statuses.  `pack` is the host's whole share (container walk, CRCs, one copy of the IDAT
    payloads); `enqueue` puts the copy, the two kernels and the status read-back on the current stream."""

    def __init__(self, n, height, width, device):
        L = nat.lib()
        self.n, self.H, self.W, self.device = int(n), int(height), int(width), device
        nbytes = int(L.fpc_png_pack_bytes(self.n, self.H, self.W))
        if nbytes < 1:
            raise ValueError("no device PNG decode for %d files of %d x %d" % (n, height, width))
        self.z_host = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        self.z_dev = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.desc_host = torch.zeros((self.n, 8), dtype=torch.int64).pin_memory()
        self.desc_dev = torch.empty((self.n, 8), dtype=torch.int64, device=device)
        self.status_host = torch.zeros(self.n, dtype=torch.int32).pin_memory()
        self.status_dev = torch.empty(self.n, dtype=torch.int32, device=device)
        self._desc_np, self._status_np = self.desc_host.numpy(), self.status_host.numpy()
        self.done = None                     # event: the statuses of the last enqueue are in status_host
        self.count = 0

    def wait(self):
        """The pinned buffers are free to be rewritten; RuntimeError for a file of the last enqueue that did not decode."""
        if self.done is None:
            return
        self.done.synchronize()
        self.done = None
        bad = np.nonzero(self._status_np[:self.count])[0]
        if bad.size:
            raise RuntimeError("device PNG decode failed for file %d of the batch (status %d, include/fpc.h FPC_INF_* / FPC_PNG_*)"
                               % (int(bad[0]), int(self._status_np[bad[0]])))

    def pack(self, files, mode):
        """-> (bytes to copy, largest bytes-per-pixel); the caller has called wait()."""
        B = len(files)
        bufs = [np.frombuffer(f, dtype=np.uint8) for f in files]
        ptrs = (ctypes.c_void_p * B)(*[b.ctypes.data for b in bufs])
        sizes = (ctypes.c_size_t * B)(*[b.size for b in bufs])
        used = ctypes.c_size_t(0)
        nat.check(nat.lib().fpc_png_pack_batch(ptrs, sizes, B, self.H, self.W, int(mode), self.z_host.data_ptr(), self.z_host.numel(),
                                               self.desc_host.data_ptr(), ctypes.byref(used)), "fpc_png_pack_batch")
        d = self._desc_np[:B]
        self.count = B
        return int(used.value), int((d[:, 4] * d[:, 6] // 8).max())

    def enqueue(self, used, max_bpp, mode, out, frame_bytes):
        """On the current stream: compressed bytes to the device, decode into `out` (file i at i * frame_bytes), statuses back."""
        B, L = self.count, nat.lib()
        self.z_dev[:used].copy_(self.z_host[:used], non_blocking=True)
        self.desc_dev[:B].copy_(self.desc_host[:B], non_blocking=True)
        ws = nat.workspace("pngdev", self.device, L.fpc_png_decode_device_workspace_bytes(B, self.H, self.W, max_bpp))
        nat.check(L.fpc_png_decode_device(nat.ptr(self.z_dev), used, nat.ptr(self.desc_dev), B, self.H, self.W, int(mode), max_bpp,
                                          nat.ptr(out), int(frame_bytes), nat.ptr(self.status_dev), nat.ptr(ws), ws.numel(),
                                          nat.stream()), "fpc_png_decode_device")
        self.status_host[:B].copy_(self.status_dev[:B], non_blocking=True)
        self.done = torch.cuda.Event()
        self.done.record()


class FrameUploader:
    """Host frames -> network tensors: pinned staging + asynchronous H2D copy + preprocess_frames, buffered `slots` deep
    on its own HIP stream so the copy of batch i+1 overlaps the network of batch i.  `upload(frames)` returns
    (tensor, event); wait on the event (stream.wait_event) before the first consumer kernel.

    Slot ownership: the tensor returned by an upload is overwritten `slots` uploads later.  Pass `consumed` (an event
    recorded after its last reader) to have the uploader wait for it on the device; without it the caller guarantees
    that the readers are done by then — FrameStreamer does when slots >= frames in flight + 2, because a ticket is
    collected (host wait on the frame) before more than that many newer frames are submitted.  (No event is recorded
    on the caller's stream by default: on the legacy null stream — PyTorch's default stream — every record / wait
    drags all other streams in, measured 1.6 ms of host time per upload beside four busy frame streams.)
    The staging copy is a single-threaded numpy copy: torch's intra-op thread pool takes milliseconds to wake up for a
    0.9 MB copy once the calling thread has been busy elsewhere (measured 4.9 ms per frame against 0.2 ms)."""

    def __init__(self, batch, height, width, device="cuda:0", slots=2, params=None):
        self.device = torch.device(device)
        self.params = params or IMAGENET_PARAMS
        self.stream = torch.cuda.Stream(device=self.device)
        shape = (batch, height, width, 3)
        self._host = [torch.empty(shape, dtype=torch.uint8).pin_memory() for _ in range(slots)]
        self._host_np = [h.numpy() for h in self._host]
        self._dev = [torch.empty(shape, dtype=torch.uint8, device=self.device) for _ in range(slots)]
        self._out = [torch.empty((batch, 3, height, width), dtype=torch.float32, device=self.device) for _ in range(slots)]
        self._free = [None] * slots          # event: the slot's previous output has been consumed
        self._busy = [None] * slots          # event: the slot's H2D copy has left the pinned buffer
        self._png = [None] * slots           # decode="device": the slot's _DevicePngDecoder, built at first use
        self._i = 0

    def upload(self, frames, consumed=None):
        """frames: uint8 array / CPU tensor [B,H,W,3].  `consumed`: event after which the tensor returned by THIS call
        may be overwritten (waited for on the device when the slot comes round again); see the class docstring."""
        k = self._i % len(self._host)
        self._i += 1
        src = frames if isinstance(frames, np.ndarray) else frames.numpy()
        if self._busy[k] is not None:
            self._busy[k].synchronize()      # the pinned buffer is about to be rewritten by the CPU
        np.copyto(self._host_np[k], src)
        return self._enqueue(k, consumed)

    def upload_png(self, files, consumed=None, threads=4, decode="host"):
        """files: B PNG files as bytes (`*_color.png`, all of the uploader's H x W): decoded by `threads` host threads
        straight into the pinned staging slot (fpc_png_decode_batch: RGB8, alpha dropped), then the same copy and kernels.
        decode="device": the host only walks the containers and copies the compressed bytes; inflate and un-filter run on
        the uploader's stream (fpc_png_decode_device, mode 3), then the same preprocessing.  A file that does not decode
        raises RuntimeError at the next upload_png on its slot or at check_decoded(), whichever comes first."""
        if decode not in ("host", "device"):
            raise ValueError("decode must be 'host' or 'device'")
        k = self._i % len(self._host)
        self._i += 1
        B, H, W, _ = self._host_np[k].shape
        if len(files) != B:
            raise ValueError(f"expected {B} files, got {len(files)}")
        if self._png[k] is not None:
            self._png[k].wait()
        if decode == "device":
            if self._png[k] is None:
                self._png[k] = _DevicePngDecoder(B, H, W, self.device)
            dec = self._png[k]
            used, max_bpp = dec.pack(files, 3)
            return self._enqueue(k, consumed, lambda: dec.enqueue(used, max_bpp, 3, self._dev[k], H * W * 3))
        if self._busy[k] is not None:
            self._busy[k].synchronize()
        bufs = [np.frombuffer(f, dtype=np.uint8) for f in files]
        ptrs = (ctypes.c_void_p * B)(*[b.ctypes.data for b in bufs])
        sizes = (ctypes.c_size_t * B)(*[b.size for b in bufs])
        nat.check(nat.lib().fpc_png_decode_batch(ptrs, sizes, B, self._host_np[k].ctypes.data, H, W, int(threads)),
                  "fpc_png_decode_batch")
        return self._enqueue(k, consumed)

    def check_decoded(self):
        """Synchronises with every device decode enqueued so far; RuntimeError for a file that did not decode."""
        for dec in self._png:
            if dec is not None:
                dec.wait()

    def _enqueue(self, k, consumed, device_png=None):
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            if self._free[k] is not None:
                self.stream.wait_event(self._free[k])
            if device_png is not None:
                device_png()                 # compressed bytes up, frames decoded into _dev[k]
            else:
                self._dev[k].copy_(self._host[k], non_blocking=True)
            self._busy[k] = torch.cuda.Event()
            self._busy[k].record()
            preprocess_frames(self._dev[k], self.params, out=self._out[k])
            done = torch.cuda.Event()
            done.record()
        self._free[k] = consumed
        return self._out[k], done


class PngFramePrefetcher:
    """Decoded frames ahead of the consumer: `workers` host threads run the native PNG decoder (ctypes releases the GIL)
    `ahead` batches in front of `next()`.  A 640x480 colour PNG takes ~10 ms of zlib + un-filtering on one core, the
    streamed pipeline consumes a frame every 0.8 ms: the pool, not the GPU, sets the rate from encoded files.

        pre = PngFramePrefetcher(lambda i: [bytes of the B files of batch i], n_batches, B, H, W)
        for frames in pre:            # uint8 [B, H, W, 3]
            tensor, ready = uploader.upload(frames)
    """

    def __init__(self, read_batch, n_batches, batch, height, width, workers=12, ahead=None):
        from concurrent.futures import ThreadPoolExecutor
        self.read_batch, self.n, self.shape = read_batch, int(n_batches), (batch, height, width, 3)
        self.ahead = int(ahead) if ahead else max(2, -(-2 * workers // max(1, batch)))
        self._pool = ThreadPoolExecutor(max_workers=workers)
        self._pending, self._next = [], 0
        nat.lib()

    def _decode_one(self, buf, dst):
        nat.check(nat.lib().fpc_png_decode(buf.ctypes.data, buf.size, dst.ctypes.data, dst.nbytes, 3), "fpc_png_decode")

    def _read_and_decode(self, i, out):
        """Pool task of batch i: read its files (the I/O of a cold page cache or slow storage stays off the consumer's
        thread), then one decode task per FILE (a batch of 32 decoded by one worker kept 2 of 14 workers busy: 350 img/s at
        batch 32).  Returns the per-file futures; the buffers stay referenced by them."""
        bufs = [np.frombuffer(f, dtype=np.uint8) for f in self.read_batch(i)]
        if len(bufs) != out.shape[0]:
            raise ValueError(f"read_batch({i}) returned {len(bufs)} files for a batch of {out.shape[0]}")
        return [self._pool.submit(self._decode_one, b, out[j]) for j, b in enumerate(bufs)]

    def _submit(self, i):
        out = np.empty(self.shape, np.uint8)
        return out, self._pool.submit(self._read_and_decode, i, out)

    def __iter__(self):
        return self

    def __next__(self):
        while self._next < self.n and len(self._pending) < self.ahead:
            self._pending.append(self._submit(self._next))
            self._next += 1
        if not self._pending:
            self._pool.shutdown(wait=False)
            raise StopIteration
        out, reader = self._pending.pop(0)
        for f in reader.result():      # (a reader never waits for its decode tasks inside the pool: no worker can starve them)
            f.result()
        return out


# ------------------------------------------------------------------------------------------------ ground-truth samples

# F/tools/project.py:78-126
CAMERA_CLASSES = ['bg', 'bottle', 'bowl', 'camera', 'can', 'laptop', 'mug']
CAMERA_SYMMETRIC_CLASSES = ['bowl', 'can', 'bottle']
REAL_SYMMETRIC_CLASSES = ['bowl', 'can', 'bottle']
INTRINSICS = {'CAMERA': np.array([[577.5, 0, 319.5], [0., 577.5, 239.5], [0., 0., 1.]]),
              'REAL': np.array([[591.0125, 0, 322.525], [0, 590.16775, 244.11084], [0, 0, 1]])}


def smp_preprocess_input(x, mean=None, std=None, input_space="RGB", input_range=None, **kwargs):
    """segmentation_models_pytorch's `preprocess_input` (encoders/_preprocessing.py; upstream package, absent from the
    reference tree): the host-side form of what fpc_preprocess_u8 does on the device, float64 like numpy's defaults."""
    if input_space == "BGR":
        x = x[..., ::-1].copy()
    if input_range is not None:
        if x.max() > 1 and input_range[1] == 1:
            x = x / 255.0
    if mean is not None:
        x = x - np.array(mean)
    if std is not None:
        x = x / np.array(std)
    return x


def get_preprocessing_fn(encoder_name="resnet18", pretrained="imagenet"):
    """smp.encoders.get_preprocessing_fn (F/tools/dataset.py:567)."""
    import functools
    return functools.partial(smp_preprocess_input, **get_preprocessing_params(encoder_name, pretrained))


def get_preprocessing(preprocessing_fn):
    """F/tools/transforms/pose_regression.py:22-28 (an albumentations Compose of one Lambda on the image): a callable
    `sample = f(**sample)` that applies preprocessing_fn to sample['image'] and passes every other key through."""
    def apply(**sample):
        sample = dict(sample)
        sample['image'] = preprocessing_fn(sample['image'])
        return sample
    return apply


def to_tensor(x, **kwargs):
    """F/tools/transforms/general.py:7-8"""
    return x.transpose(2, 0, 1) if len(x.shape) == 3 else x


class NOCSDataset(torch.utils.data.Dataset):
    """F/tools/dataset.py:99-434.  dataset_dir: a pathlib.Path (or str) searched recursively for `*_color.png` frames
    whose `*_meta+.json` holds at least one instance of the wanted `classes` (names from CLASSES; default: all)."""

    CLASSES = CAMERA_CLASSES
    SYMMETRIC_CLASSES = CAMERA_SYMMETRIC_CLASSES
    INTRINSICS = INTRINSICS['CAMERA']
    CAMERA_MASKS = True            # masks are RGBA files whose first channel holds the instance ids (REAL: single channel)

    def __init__(self, dataset_dir, max_size=None, classes=None, augmentation=None, preprocessing=None):
        if classes is None:
            classes = self.CLASSES
        self.classes = classes
        self.class_values_map = {self.CLASSES.index(cls.lower()): self.classes.index(cls) for cls in self.classes}
        self.symmetric_classes = [self.classes.index(cls.lower()) for cls in self.SYMMETRIC_CLASSES if cls in self.classes]
        self.images_fps = self.get_image_paths_in_dir(pathlib.Path(dataset_dir), max_size=max_size)
        self.augmentation = augmentation
        self.preprocessing = preprocessing

    def __len__(self):
        return len(self.images_fps)

    def get_image_paths_in_dir(self, dir_path, max_size=None):
        """The frames of the data set in the reference's order (F/tools/dataset.py:295-352): directories level by level
        (breadth-first, children in the file system's listing order), inside a directory the `*color*.png` frames in
        listing order, kept when their side file lists an instance of a wanted class; the walk stops after the first
        directory that brings the count to `max_size`."""
        from collections import deque
        frames, todo = [], deque([dir_path])
        while todo and (max_size is None or len(frames) < max_size):
            here = todo.popleft()
            entries = list(here.iterdir())
            frames.extend(self.remove_empty_samples([e for e in entries if e.is_file() and e.suffix == '.png' and 'color' in e.name]))
            todo.extend(e for e in entries if e.is_dir())
        return frames if max_size is None else frames[:max_size]

    def remove_empty_samples(self, file_paths):
        good = []
        for fp in file_paths:
            json_data = jt.load_from_json(str(fp).replace('_color.png', '_meta+.json'))
            if any(class_value in self.class_values_map for class_value in json_data['instance_dict'].values()):
                good.append(fp)
        return good

    def __getitem__(self, i):
        color_fp = str(self.images_fps[i])
        image = imread_png(color_fp)
        mask = imread_png(color_fp.replace('_color.png', '_mask.png'))
        mask = (mask[:, :, 0] if self.CAMERA_MASKS else mask).astype('float')
        mask[mask == 255] = 0                                      # background
        depth = standardize_depth(imread_png(color_fp.replace('_color.png', '_depth.png')))
        json_data = jt.load_from_json(color_fp.replace('_color.png', '_meta+.json'))

        # Which pixels survive: instances the side file lists (distractor objects are not listed) whose class is one of
        # the wanted ones (F/tools/dataset.py:183-228).  Two 256-entry tables indexed by the mask's instance id — id -> id
        # and id -> class index — replace the reference's per-instance sweeps over the image.
        good_json_data = self.wanted_instances(json_data)
        id_of = np.zeros(256, dtype=mask.dtype)
        class_of = np.zeros(256, dtype=mask.dtype)
        for inst_id, c in good_json_data['instance_dict'].items():
            id_of[inst_id] = inst_id
            class_of[inst_id] = c
        pixel_ids = mask.astype(np.intp)
        good_instances_mask = id_of[pixel_ids]

        agg_data = self.generate_agg_data(good_instances_mask, good_json_data)
        if (agg_data['z'] <= 0).any():                             # invalid / corrupt sample
            return None
        class_mask = class_of[pixel_ids]

        sample = {'clean_image': image, 'image': image, 'mask': class_mask, 'depth': depth}
        if self.preprocessing:
            sample = self.preprocessing(**sample)
        sample['image'] = to_tensor(sample['image'])               # numpy_to_torch(): the image target only
        if sample['image'].dtype != np.uint8:
            sample['image'] /= np.max(np.abs(sample['image']))
        sample.update({
            'path': self.images_fps[i],
            'image': sample['image'].astype(np.float32),           # skimage.img_as_float32 of a float array
            'mask': sample['mask'].astype('long'),
            'depth': sample['depth'].astype('float32'),
            'agg_data': agg_data,
        })
        return sample

    def wanted_instances(self, json_data):
        """The side file restricted to the instances of a wanted class, in file order: {'instance_dict': {instance id:
        class index in self.classes}, and every per-instance key stacked over the rows kept}."""
        listed = [(int(k), c) for k, c in json_data['instance_dict'].items()]
        rows = [r for r, (_, c) in enumerate(listed) if c in self.class_values_map]
        good_json_data = {'instance_dict': {}}
        for r in rows:
            inst_id, c = listed[r]
            good_json_data['instance_dict'][inst_id] = self.class_values_map[c]
        if rows:
            for key, per_instance in json_data.items():
                if key != 'instance_dict':
                    good_json_data[key] = np.stack([per_instance[r] for r in rows])
        return good_json_data

    def gt_item(self, i):
        """The half of `__getitem__` that the side file alone decides — no pixel is touched, no mask file is read:
        {'path', 'mask_path', 'ids' (instance id per row of agg_data: side-file order after the class filter),
        'class_values' (class index per row), 'valid' (False where `__getitem__` returns None: an instance with z <= 0),
        'table' (the float64 per-instance blocks of `generate_agg_data` but instance_masks)}.  GroundTruthUploader builds
        the pixel half on the device from these and the mask's instance ids.  Instance ids are the mask's byte values
        1 .. 254 (0 and 255 are background): a side file that lists another one raises ValueError (the host path lets
        id 0 through and then miscounts its instances)."""
        color_fp = str(self.images_fps[i])
        return self.gt_from_side_file(jt.load_from_json(color_fp.replace('_color.png', '_meta+.json')), self.images_fps[i],
                                      color_fp.replace('_color.png', '_mask.png'))

    def gt_from_side_file(self, json_data, path=None, mask_path=None):
        """`gt_item` for a side file that is already loaded."""
        for key in json_data['instance_dict']:
            if not 1 <= int(key) <= 254:
                raise ValueError("%s lists instance id %s: ids are the mask's byte values 1 .. 254" % (path, key))
        good_json_data = self.wanted_instances(json_data)
        ids = list(good_json_data['instance_dict'])
        table = self.instance_table(good_json_data, len(ids))
        return {'path': path, 'mask_path': mask_path, 'ids': ids, 'class_values': list(good_json_data['instance_dict'].values()),
                'valid': not (table['z'] <= 0).any(), 'table': table}

    def get_random_batched_sample(self, batch_size=1, device=None):
        ids = np.random.choice(np.arange(len(self)), size=batch_size, replace=False)
        return my_collate_fn([self[int(k)] for k in ids], device)

    def generate_agg_data(self, instances_mask, json_data):
        """Per-instance ground truth, one row per entry of the side file's instance_dict in file order
        (F/tools/dataset.py:373-434): n = the number of instance ids present in the mask; class / symmetric ids, the
        instance's binary mask, quaternion, scales / norm factor, and from the RT matrices the projected origin (flipped to
        the other coordinate style), z, T and R (tools/data_manipulation.py).  Filled one fancy-indexed block per key."""
        n = np.unique(instances_mask).size - 1
        inst = np.array(list(json_data['instance_dict'])).reshape(len(json_data['instance_dict']))
        return self.instance_table(json_data, n, lambda block: block(instances_mask[None] == inst[:, None, None],
                                                                     *instances_mask.shape))

    def instance_table(self, json_data, n, instance_masks=None):
        """The per-instance blocks of `generate_agg_data` for n rows, one fancy-indexed block per key.  `instance_masks`
        (a callable on the block builder) adds that key in its place; without it the table is the part of agg_data that
        the side file alone decides (`gt_item`)."""
        listed = list(json_data['instance_dict'].items())             # (instance id, class id)
        k = len(listed)
        cls = np.array([c for _, c in listed], dtype=np.float64).reshape(k)
        per_instance = dict(dm.extract_xyz_R_T_from_RTs(json_data['RTs'], self.INTRINSICS),      # xy, z, T, R
                            quaternion=json_data['quaternions'], scales=json_data['scales'], RT=json_data['RTs'])

        def block(values, *shape):
            out = np.zeros((n,) + shape)
            out[:k] = np.asarray(values, dtype=np.float64).reshape((-1,) + shape)[:k]
            return out

        agg_data = {
            'class_ids': block(cls), 'symmetric_ids': block(np.isin(cls, self.symmetric_classes)),
            **({'instance_masks': instance_masks(block)} if instance_masks else {}),
            'quaternion': block(per_instance['quaternion'], 4),
            'scales': block(per_instance['scales'], 3) / np.expand_dims(json_data['norm_factors'], axis=1),
            'xy': block(per_instance['xy'], 2)[:, ::-1],              # (row, col) -> the other style
            'z': block(per_instance['z'], 1), 'T': block(per_instance['T'], 3),
            'R': block(per_instance['R'], 3, 3), 'RT': block(per_instance['RT'], 4, 4),
        }
        return agg_data


class CAMERADataset(NOCSDataset):
    pass


class REALDataset(NOCSDataset):
    SYMMETRIC_CLASSES = REAL_SYMMETRIC_CLASSES
    INTRINSICS = INTRINSICS['REAL']
    CAMERA_MASKS = False


def my_collate_fn(batch, device=None):
    """F/tools/dataset.py:453-529: drop None samples; stack array-valued keys; concatenate every agg_data entry along
    axis 0 and add agg_data['sample_ids'] (the sample index repeated once per instance)."""
    batch = [s for s in batch if s is not None]
    if not batch:
        return None
    columns, agg = {}, {"sample_ids": []}
    for sample_id, sample in enumerate(batch):
        for key, value in sample.items():
            if key != "agg_data":
                columns.setdefault(key, []).append(value)
        if "agg_data" in sample:
            for subkey, value in sample["agg_data"].items():
                agg.setdefault(subkey, []).append(value)
            agg["sample_ids"].append(np.repeat(np.array(sample_id), sample["agg_data"]["class_ids"].shape[0]))

    def put(a):
        t = torch.from_numpy(a)
        return t.to(device) if device else t

    out = {key: (put(np.stack(vals)) if isinstance(vals[0], np.ndarray) else vals) for key, vals in columns.items()}
    out["agg_data"] = {subkey: put(np.concatenate(vals, axis=0)) for subkey, vals in agg.items()}
    return out


# ------------------------------------------------------------------------------------- ground-truth batches on the device

# the float64 per-instance keys of agg_data in generate_agg_data's order, with their row shapes
GT_TABLE_KEYS = (('class_ids', ()), ('symmetric_ids', ()), ('quaternion', (4,)), ('scales', (3,)), ('xy', (2,)), ('z', (1,)),
                 ('T', (3,)), ('R', (3, 3)), ('RT', (4, 4)))
_MASK_ELEM = {torch.float64: 8, torch.float32: 4, torch.uint8: 1}


def gt_tables(items):
    """`gt_item` dicts of B frames -> (row_of int16 [B,256], class_of uint8 [B,256], first_row int32 [B+1], n): the rows of
    agg_data are the frames' instances in order, so frame b owns rows first_row[b] .. first_row[b+1] - 1.  Ids that no
    item lists (distractors, unwanted classes, the background 0 and 255) map to row -1 and class 0."""
    B = len(items)
    row_of = np.full((B, 256), -1, np.int16)
    class_of = np.zeros((B, 256), np.uint8)
    first_row = np.zeros(B + 1, np.int32)
    n = 0
    for b, item in enumerate(items):
        for inst_id, c in zip(item['ids'], item['class_values']):
            row_of[b, inst_id] = n
            class_of[b, inst_id] = c
            n += 1
        first_row[b + 1] = n
    return row_of, class_of, first_row, n


def build_gt_host(ids_u8, pix_stride, row_of, class_of, first_row, n, mask_dtype=np.float64):
    """What fpc_gt_build computes, in numpy.  ids_u8: uint8 [B,H,W] (pix_stride 1) or [B,H,W,pix_stride] (the id is channel
    0) -> (class_mask int64 [B,H,W], instance_masks mask_dtype [n,H,W], pix_count int32 [n])."""
    ids_u8 = np.asarray(ids_u8)
    B, H, W = ids_u8.shape[:3]
    ids = ids_u8.reshape(B, -1)[:, ::pix_stride]
    frames = np.arange(B)[:, None]
    class_mask = np.asarray(class_of)[frames, ids].astype(np.int64).reshape(B, H, W)
    rows = np.asarray(row_of)[frames, ids]
    inst = np.zeros((n, H, W), mask_dtype)
    for b in range(B):
        for r in range(max(int(first_row[b]), 0), min(int(first_row[b + 1]), n)):
            inst[r] = (rows[b] == r).reshape(H, W)
    return class_mask, inst, np.count_nonzero(inst.reshape(n, -1), axis=1).astype(np.int32)


class GroundTruthUploader:
    """Instance-id masks + `NOCSDataset.gt_item` dicts -> the ground-truth half of a batch on the device, the twin of
    FrameUploader: pinned staging, asynchronous H2D copies and one fpc_gt_build launch on its own stream, `slots` deep.
    `upload(...)` / `upload_png(...)` return (batch_dict, event); wait on the event before the first consumer kernel.

    batch_dict['mask'] (int64 [B',H,W]) and batch_dict['agg_data'] carry the keys, dtypes, shapes and values of
    `my_collate_fn([ds[i] for i in ...], device)`, 'sample_ids' included; only 'instance_masks' takes `mask_dtype`
    (float64 as the reference; float32 or uint8 on request — uint8 is what batchwise_get_2d_iou reads without a
    conversion pass).  On top come agg_data['pixel_counts'] (int32 [n]) and, `with_depth`, batch_dict['depth'] (float32).
    Every value is a contiguous view `[:n]` / `[:B']` of a slot buffer: nothing is allocated per upload.

    What the host bytes cost: the id planes (H W channels bytes a frame) and two small tables cross the bus; the float64
    planes (8 H W bytes an instance) are written by the device at its own rate.

    Slot ownership is FrameUploader's: the dict returned by an upload is overwritten `slots` uploads later; pass
    `consumed` (an event recorded after its last reader) to have the uploader wait for it on the device.

    An instance the side file lists but the mask does not contain: the host path raises for it (n < k in
    generate_agg_data); this path cannot know without a synchronisation, so it emits the row with an all-zero plane and
    pixel_counts == 0.  `GroundTruthUploader.check(batch_dict)` synchronises and raises ValueError for such a batch."""

    def __init__(self, batch, height, width, channels, device="cuda:0", slots=2, max_instances=256,
                 mask_dtype=torch.float64, with_depth=False):
        if mask_dtype not in _MASK_ELEM:
            raise ValueError("mask_dtype must be torch.float64, torch.float32 or torch.uint8")
        if not 1 <= channels <= 4:
            raise ValueError("channels must be 1 .. 4")
        self.device = torch.device(device)
        self.shape = (batch, height, width, channels)
        self.max_instances, self.mask_dtype, self.with_depth = int(max_instances), mask_dtype, bool(with_depth)
        self.stream = torch.cuda.Stream(device=self.device)
        B, H, W, M = batch, height, width, self.max_instances
        # one buffer for the integer tables: sample_ids i64 [M] | first_row i32 [B+1] | row_of i16 [B,256] | class_of u8 [B,256]
        o_first = 8 * M
        o_row = o_first + -(-4 * (B + 1) // 16) * 16
        o_cls = o_row + 512 * B
        self._cuts = (o_first, o_row, o_cls, o_cls + 256 * B)
        widths = [int(np.prod(s, dtype=np.int64)) for _, s in GT_TABLE_KEYS]
        self._offs = np.concatenate([[0], np.cumsum(widths)]) * M          # the float64 table, key by key
        self._slots = []
        for _ in range(slots):
            s = {'ids_host': torch.empty(self.shape, dtype=torch.uint8).pin_memory(),
                 'ids_dev': torch.empty(self.shape, dtype=torch.uint8, device=self.device),
                 'int_host': torch.zeros(self._cuts[3], dtype=torch.uint8).pin_memory(),
                 'int_dev': torch.empty(self._cuts[3], dtype=torch.uint8, device=self.device),
                 'f64_host': torch.zeros(int(self._offs[-1]), dtype=torch.float64).pin_memory(),
                 'f64_dev': torch.empty(int(self._offs[-1]), dtype=torch.float64, device=self.device),
                 'class_mask': torch.empty((B, H, W), dtype=torch.int64, device=self.device),
                 'inst': torch.empty((M, H, W), dtype=mask_dtype, device=self.device),
                 'count': torch.empty(M, dtype=torch.int32, device=self.device)}
            if self.with_depth:        # a depth file is 16-bit grey or R,G,B(,A) bytes: at most four bytes a pixel
                s['depth_host'] = torch.empty(B * H * W * 4, dtype=torch.uint8).pin_memory()      # frames packed at their own size
                s['depth_dev'] = torch.empty(B * H * W * 4, dtype=torch.uint8, device=self.device)
                s['depth'] = torch.empty((B, H, W), dtype=torch.float32, device=self.device)
            s['ids_np'], s['int_np'], s['f64_np'] = s['ids_host'].numpy(), s['int_host'].numpy(), s['f64_host'].numpy()
            s['tables'] = self._carve(s['int_np'], lambda a, dt: a.view(dt))
            s['tables_dev'] = self._carve(s['int_dev'], lambda a, dt: a.view(getattr(torch, np.dtype(dt).name)))
            self._slots.append(s)
        self._free = [None] * slots          # event: the slot's previous batch has been consumed
        self._busy = [None] * slots          # event: the slot's H2D copies have left the pinned buffers
        self._i = 0
        self._pool = None
        self._png = [[None, None] for _ in range(slots)]      # decode="device": the slot's mask and depth _DevicePngDecoder

    def _carve(self, raw, view):
        """(sample_ids, first_row, row_of, class_of) views of the integer buffer."""
        a, b, c, d = self._cuts
        return view(raw[:a], np.int64), view(raw[a:a + 4 * (self.shape[0] + 1)], np.int32), view(raw[b:c], np.int16), raw[c:d]

    def _next_slot(self, items):
        B = len(items)
        if not 1 <= B <= self.shape[0]:
            raise ValueError(f"expected 1 .. {self.shape[0]} items, got {B}")
        for item in items:
            if not item['valid']:
                raise ValueError(f"{item['path']}: an invalid item (z <= 0); drop the frame before uploading it")
        n = sum(len(item['ids']) for item in items)
        if n > self.max_instances:
            raise ValueError(f"{n} instances in the batch, the uploader holds {self.max_instances}")
        k = self._i % len(self._slots)
        self._i += 1
        if self._busy[k] is not None:
            self._busy[k].synchronize()      # the pinned buffers are about to be rewritten by the CPU
        return k, self._slots[k]

    def upload(self, id_planes, items, consumed=None, depth=None):
        """id_planes: uint8 array / CPU tensor [B',H,W,channels] ([B',H,W] when channels == 1), the mask files as decoded;
        items: the B' `gt_item` dicts.  depth (with_depth): uint16 [B',H,W] or uint8 [B',H,W,3|4] as decoded."""
        k, s = self._next_slot(items)
        B = len(items)
        src = id_planes if isinstance(id_planes, np.ndarray) else id_planes.numpy()
        np.copyto(s['ids_np'][:B], src.reshape((B,) + self.shape[1:]))
        kind = None
        if self.with_depth:
            if depth is None:
                raise ValueError("this uploader was built with_depth: pass the decoded depth planes")
            d = depth if isinstance(depth, np.ndarray) else depth.numpy()
            kind = self._depth_kind(16 if d.dtype == np.uint16 else 8, d.shape[3] if d.ndim == 4 else 1)
            flat = np.ascontiguousarray(d).reshape(-1).view(np.uint8)
            np.copyto(s['depth_host'].numpy()[:flat.size], flat)
        return self._enqueue(k, items, consumed, kind)

    def upload_png(self, mask_files, items, consumed=None, threads=4, depth_files=None, decode="host"):
        """mask_files: the B' `*_mask.png` files as bytes, decoded as stored (fpc_png_decode mode 0) by `threads` host
        threads straight into the pinned slot; their size and channel count must be the uploader's (ValueError).
        depth_files (with_depth): the `*_depth.png` files, all 16-bit grey or all colour-coded.
        decode="device": the compressed bytes are uploaded and fpc_png_decode_device (mode 0) writes the planes the host
        path would have copied; a file that does not decode raises RuntimeError at the next upload_png on its slot or
        at check_decoded()."""
        if decode not in ("host", "device"):
            raise ValueError("decode must be 'host' or 'device'")
        k, s = self._next_slot(items)
        for dec in self._png[k]:
            if dec is not None:
                dec.wait()
        B = len(items)
        if len(mask_files) != B:
            raise ValueError(f"{B} items, {len(mask_files)} mask files")
        _, H, W, C = self.shape
        jobs = [(f, s['ids_np'][j]) for j, f in enumerate(mask_files)]
        for f, _ in jobs:
            if self._png_info(f) != (W, H, 8, C):
                raise ValueError("a mask file is not %d x %d with %d 8-bit channels" % (W, H, C))
        kind = None
        if self.with_depth:
            if depth_files is None or len(depth_files) != B:
                raise ValueError("this uploader was built with_depth: pass one depth file per item")
            infos = {self._png_info(f) for f in depth_files}
            if len(infos) != 1 or next(iter(infos))[:2] != (W, H):
                raise ValueError("the depth files are not all %d x %d of one format" % (W, H))
            _, _, bits, ch = next(iter(infos))
            kind = self._depth_kind(bits, ch)
            nbytes = H * W * ch * bits // 8
            jobs += [(f, s['depth_host'].numpy()[j * nbytes:(j + 1) * nbytes]) for j, f in enumerate(depth_files)]
        if decode == "device":
            decs = self._png[k]
            for j in range(2 if kind is not None else 1):
                if decs[j] is None:
                    decs[j] = _DevicePngDecoder(self.shape[0], H, W, self.device)
            packed = [decs[0].pack(mask_files, 0)] + ([decs[1].pack(depth_files, 0)] if kind is not None else [])

            def device_png():
                decs[0].enqueue(*packed[0], 0, s['ids_dev'], H * W * C)
                if kind is not None:
                    decs[1].enqueue(*packed[1], 0, s['depth_dev'], nbytes)
            return self._enqueue(k, items, consumed, kind, device_png)
        if threads > 1 and len(jobs) > 1:
            if self._pool is None or self._pool[0] != int(threads):      # kept between uploads: starting threads costs a decode
                from concurrent.futures import ThreadPoolExecutor
                self._pool = (int(threads), ThreadPoolExecutor(max_workers=int(threads)))
            list(self._pool[1].map(lambda job: self._png_decode(*job), jobs))
        else:
            for job in jobs:
                self._png_decode(*job)
        return self._enqueue(k, items, consumed, kind)

    @staticmethod
    def _png_info(data):
        buf = np.frombuffer(data, dtype=np.uint8)
        info = (ctypes.c_int32 * 5)()
        nat.check(nat.lib().fpc_png_info(buf.ctypes.data, buf.size, info), "fpc_png_info")
        return int(info[0]), int(info[1]), int(info[2]), int(info[4])          # width, height, bit depth, channels

    @staticmethod
    def _png_decode(data, out):
        buf = np.frombuffer(data, dtype=np.uint8)
        nat.check(nat.lib().fpc_png_decode(buf.ctypes.data, buf.size, out.ctypes.data, out.nbytes, 0), "fpc_png_decode")

    @staticmethod
    def _depth_kind(bits, channels):
        """(src_kind, channels) of fpc_depth_decode for what standardize_depth takes."""
        if bits == 16 and channels == 1:
            return 1, 1
        if bits == 8 and channels in (3, 4):
            return 0, channels
        raise ValueError("unsupported depth image")

    def check_decoded(self):
        """Synchronises with every device decode enqueued so far; RuntimeError for a file that did not decode."""
        for decs in self._png:
            for dec in decs:
                if dec is not None:
                    dec.wait()

    def _enqueue(self, k, items, consumed, depth_kind, device_png=None):
        s = self._slots[k]
        B, (_, H, W, C) = len(items), self.shape
        row_of, class_of, first_row, n = gt_tables(items)
        sample_ids, t_first, t_row, t_cls = s['tables']
        sample_ids[:n] = np.repeat(np.arange(B), np.diff(first_row))
        t_first[:B + 1], t_row[:256 * B], t_cls[:256 * B] = first_row, row_of.reshape(-1), class_of.reshape(-1)
        M = self.max_instances
        for (key, shape), off in zip(GT_TABLE_KEYS, self._offs):
            w = int(np.prod(shape, dtype=np.int64))
            dst = s['f64_np'][off:off + n * w].reshape((n,) + shape)
            r = 0
            for item in items:
                m = len(item['ids'])
                dst[r:r + m] = item['table'][key]
                r += m
        L = nat.lib()
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            if self._free[k] is not None:
                self.stream.wait_event(self._free[k])
            if device_png is not None:
                device_png()                 # compressed bytes up, id (and depth) planes decoded into ids_dev / depth_dev
            else:
                s['ids_dev'][:B].copy_(s['ids_host'][:B], non_blocking=True)
            s['int_dev'].copy_(s['int_host'], non_blocking=True)
            s['f64_dev'].copy_(s['f64_host'], non_blocking=True)
            if depth_kind is not None and device_png is None:
                used = B * H * W * (2 if depth_kind[0] == 1 else depth_kind[1])
                s['depth_dev'][:used].copy_(s['depth_host'][:used], non_blocking=True)
            self._busy[k] = torch.cuda.Event()
            self._busy[k].record()
            d_sample, d_first, d_row, d_cls = s['tables_dev']
            nat.check(L.fpc_gt_build(nat.ptr(s['ids_dev']), C, H * W * C, B, H, W, nat.ptr(d_row), nat.ptr(d_cls), nat.ptr(d_first), n,
                                     nat.ptr(s['class_mask']), nat.ptr(s['inst']), _MASK_ELEM[self.mask_dtype], nat.ptr(s['count']),
                                     nat.stream()), "fpc_gt_build")
            if depth_kind is not None:
                nat.check(L.fpc_depth_decode(nat.ptr(s['depth_dev']), depth_kind[0], depth_kind[1], B, H, W, nat.ptr(s['depth']),
                                             nat.stream()), "fpc_depth_decode")
            done = torch.cuda.Event()
            done.record()
        self._free[k] = consumed
        agg = {'sample_ids': d_sample[:n]}
        for (key, shape), off in zip(GT_TABLE_KEYS, self._offs):
            w = int(np.prod(shape, dtype=np.int64))
            agg[key] = s['f64_dev'][off:off + M * w].view((M,) + shape)[:n]
            if key == 'symmetric_ids':
                agg['instance_masks'] = s['inst'][:n]
        agg['pixel_counts'] = s['count'][:n]
        out = {'mask': s['class_mask'][:B], 'agg_data': agg}
        if depth_kind is not None:
            out['depth'] = s['depth'][:B]
        return out, done

    @staticmethod
    def check(batch_dict):
        """Synchronises.  ValueError when an instance of the batch has no pixel in its mask (the host path's n < k)."""
        empty = torch.nonzero(batch_dict['agg_data']['pixel_counts'] == 0).flatten().tolist()
        if empty:
            raise ValueError("instances without a pixel in their mask: rows %s" % empty)
