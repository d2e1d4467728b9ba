"""PNG decoding on the device (csrc/png_device.hip: k_png_inflate + k_png_unfilter behind fpc_png_decode_device, and the
uploaders' decode="device") against the host decoder fpc_png_decode, byte for byte.  Only well-formed deflate streams
reach a kernel here: truncated and structurally damaged ones run on the CPU build of the same inflate.hpp
(tests/test_png_inflate_host.py).  The one damaged file below has a wrong Adler-32 and nothing else."""
import ctypes
import os
import struct
import zlib

import numpy as np
import pytest
import torch

import _gt_cases as C
from oracle import png_oracle as po

pytestmark = pytest.mark.gpu

PNG_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "png")
CANARY = 0x5A
WIDTHS, HEIGHTS = (1, 5, 33, 64), (1, 3, 17)
SIZES = [(H, W) for H in HEIGHTS for W in WIDTHS] + [(130, 7)]      # 130 rows: three bands of the un-filter kernel, the last partial
FORMATS = ("grey8", "ga8", "rgb8", "rgba8", "pal8", "grey16", "rgb16")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def D(dev):
    from fastposecnn_amd import _native
    _native.lib()
    from fastposecnn_amd.tools import dataset as D
    return D


def chunk(typ, payload):
    return struct.pack(">I", len(payload)) + typ + payload + struct.pack(">I", zlib.crc32(typ + payload) & 0xffffffff)


def with_stream(png, z, split=None):
    """The same file around another zlib stream."""
    out = po.SIG
    for typ, body in po._chunks(png):
        if typ not in (b"IDAT", b"IEND"):
            out += chunk(typ, body)
    step = split or len(z)
    for o in range(0, len(z), step):
        out += chunk(b"IDAT", z[o:o + step])
    return out + chunk(b"IEND", b"")


def stream_of(png):
    return b"".join(body for typ, body in po._chunks(png) if typ == b"IDAT")


def z_fixed(png):
    c = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_FIXED)
    raw = zlib.decompress(stream_of(png))
    return with_stream(png, c.compress(raw) + c.flush())


def image(fmt, H, W, r):
    """-> (array, palette or None): low-entropy values with runs, so that level 6 emits matches as well as literals."""
    ch = {"grey8": 1, "ga8": 2, "rgb8": 3, "rgba8": 4, "pal8": 1, "grey16": 1, "rgb16": 3}[fmt]
    if fmt == "pal8":
        return r.integers(0, 7, (H, W), dtype=np.uint8), r.integers(0, 256, (7, 3), dtype=np.uint8)
    hi = 65536 if fmt.endswith("16") else 256
    a = r.integers(0, hi, (H, W, ch)).astype(np.uint16 if hi == 65536 else np.uint8)
    a[:, W // 2:] = a[:, :W - W // 2]
    return (a[:, :, 0] if ch == 1 else a), None


def host_decode(D, f, mode):
    a = D.imread_png(f, rgb8=(mode == 3))
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def device_decode(dev, files, H, W, mode, frame_bytes):
    """fpc_pack_batch -> copies -> fpc_png_decode_device with 64 canary bytes around out, workspace and status.
    -> (out uint8 [n, frame_bytes], status int32 [n])."""
    from fastposecnn_amd import _native as nat
    L, n = nat.lib(), len(files)
    staging = torch.empty(L.fpc_png_pack_bytes(n, H, W), dtype=torch.uint8).pin_memory()
    desc = torch.zeros((n, 8), dtype=torch.int64)
    bufs = [np.frombuffer(f, np.uint8) for f in files]
    ptrs = (ctypes.c_void_p * n)(*[b.ctypes.data for b in bufs])
    sizes = (ctypes.c_size_t * n)(*[b.size for b in bufs])
    used = ctypes.c_size_t(0)
    nat.check(L.fpc_png_pack_batch(ptrs, sizes, n, H, W, mode, staging.data_ptr(), staging.numel(), desc.data_ptr(),
                                   ctypes.byref(used)), "fpc_png_pack_batch")
    max_bpp = int((desc[:, 4] * desc[:, 6] // 8).max())
    wsb = L.fpc_png_decode_device_workspace_bytes(n, H, W, max_bpp)
    z_dev, desc_dev = staging[:used.value].to(dev), desc.to(dev)
    out = torch.full((64 + n * frame_bytes + 64,), CANARY, dtype=torch.uint8, device=dev)
    ws = torch.full((64 + wsb + 64,), CANARY, dtype=torch.uint8, device=dev)
    status = torch.full((16 + n + 16,), -77, dtype=torch.int32, device=dev)
    nat.check(L.fpc_png_decode_device(z_dev.data_ptr(), used.value, desc_dev.data_ptr(), n, H, W, mode, max_bpp, out.data_ptr() + 64,
                                      frame_bytes, status.data_ptr() + 64, ws.data_ptr() + 64, wsb, nat.stream()),
              "fpc_png_decode_device")
    torch.cuda.synchronize()
    out, ws, status = out.cpu().numpy(), ws.cpu().numpy(), status.cpu().numpy()
    assert (out[:64] == CANARY).all() and (out[-64:] == CANARY).all(), "out canary"
    assert (ws[:64] == CANARY).all() and (ws[-64:] == CANARY).all(), "workspace canary"
    assert (status[:16] == -77).all() and (status[-16:] == -77).all(), "status canary"
    return out[64:-64].reshape(n, frame_bytes), status[16:-16]


def check_batch(D, dev, files, H, W, mode):
    want = [host_decode(D, f, mode) for f in files]
    frame = want[0].size
    assert all(w.size == frame for w in want)
    got, status = device_decode(dev, files, H, W, mode, frame)
    assert not status.any(), status
    for i, w in enumerate(want):
        assert np.array_equal(got[i], w), (i, mode)
    return got


def mode0_groups(files):
    """Files of one (depth, mode-0 channels), as fpc_png_pack_batch wants them for mode 0."""
    groups = {}
    for f in files:
        a, info = po.decode(f)
        groups.setdefault((info["bit_depth"], info["channels"]), []).append(f)
    return list(groups.values())


def test_every_fixture_in_both_modes(D, dev):
    names = sorted(f for f in os.listdir(PNG_DIR) if f.endswith(".png"))
    assert len(names) >= 10
    for name in names:
        f = open(os.path.join(PNG_DIR, name), "rb").read()
        _, info = po.decode(f)
        for mode in (0, 3):
            check_batch(D, dev, [f], info["height"], info["width"], mode)


@pytest.fixture(scope="module")
def matrix():
    """(H, W) -> the files of that size: 7 formats x (5 forced filters + the cycling default) x (level 0, level 6, Z_FIXED,
    level 6 in 7-byte IDAT chunks)."""
    r = np.random.default_rng(77)
    out = {}
    for H, W in SIZES:
        files = []
        for fmt in FORMATS:
            a, pal = image(fmt, H, W, r)
            for filt in (0, 1, 2, 3, 4, None):
                filters = None if filt is None else [filt] * H
                f6 = po.encode(a, filters=filters, level=6, palette=pal)
                files += [po.encode(a, filters=filters, level=0, palette=pal), f6, z_fixed(f6),
                          po.encode(a, filters=filters, level=6, idat_split=7, palette=pal)]
        out[(H, W)] = files
    return out


@pytest.mark.parametrize("H, W", SIZES)
def test_synthetic_matrix(D, dev, matrix, H, W):
    files = matrix[(H, W)]
    assert len(files) == 7 * 6 * 4
    check_batch(D, dev, files, H, W, 3)
    for group in mode0_groups(files):
        check_batch(D, dev, group, H, W, 0)


def test_mixed_batch_of_12(D, dev, matrix):
    files = matrix[(17, 33)]
    r = np.random.default_rng(1)
    pick = [files[i] for i in r.choice(len(files), 12, replace=False)]
    assert len({po.decode(f)[1]["color_type"] for f in pick}) >= 3
    check_batch(D, dev, pick, 17, 33, 3)


@pytest.fixture(scope="module")
def full_frame():
    r = np.random.default_rng(9)
    y, x = np.mgrid[0:480, 0:640]
    ramp = np.stack([(x * 255 // 639), (y * 255 // 479), ((x + y) * 255 // 1118)], -1)
    a = ((ramp & ~7) | r.integers(0, 8, (480, 640, 3))).astype(np.uint8)
    return po.encode(a, level=6)


def test_full_frame_is_multi_block_and_repeatable(D, dev, full_frame):
    z = stream_of(full_frame)
    assert z[2] & 1 == 0                       # BFINAL of the first block: more blocks follow
    first = check_batch(D, dev, [full_frame], 480, 640, 3)
    again = check_batch(D, dev, [full_frame], 480, 640, 3)
    assert np.array_equal(first, again)


def wrong_adler(png):
    z = bytearray(stream_of(png))
    z[-1] ^= 0x40
    return with_stream(png, bytes(z))


def test_status_of_one_damaged_file_leaves_the_others(D, dev, matrix):
    good = [f for f in matrix[(17, 33)] if po.decode(f)[1]["color_type"] == 2][:3]
    files = [good[0], wrong_adler(good[1]), good[2]]
    with pytest.raises(RuntimeError):
        D.imread_png(files[1])                 # the host decoder refuses it too
    want = [host_decode(D, f, 3) for f in good]
    got, status = device_decode(dev, files, 17, 33, 3, want[0].size)
    assert status[0] == 0 and status[2] == 0 and status[1] == 12          # FPC_INF_EADLER
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
    assert (got[1] == CANARY).all()            # a file that does not decode leaves its frame alone


@pytest.fixture(scope="module")
def nocs(D):
    ds = C.dataset()
    items = [ds.gt_item(i % len(ds)) for i in range(4)]
    read = lambda path: open(path, "rb").read()
    return (items, [read(str(it["path"])) for it in items], [C.mask_bytes(it) for it in items],
            [read(it["mask_path"].replace("_mask.png", "_depth.png")) for it in items])


def test_frame_uploader_parity(D, dev, nocs):
    items, color, _, _ = nocs
    host, devp = D.FrameUploader(4, 48, 64, device=dev, slots=2), D.FrameUploader(4, 48, 64, device=dev, slots=2)
    for it in range(5):
        files = color[it % 4:] + color[:it % 4]
        a, ea = host.upload_png(files)
        b, eb = devp.upload_png(files, decode="device")
        ea.synchronize()
        eb.synchronize()
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), it
    devp.check_decoded()
    devp.upload_png(color[:3] + [wrong_adler(color[3])], decode="device")
    with pytest.raises(RuntimeError, match="file 3"):
        devp.check_decoded()
    devp.check_decoded()                        # reported once
    b, eb = devp.upload_png(color, decode="device")
    a, ea = host.upload_png(color)
    ea.synchronize()
    eb.synchronize()
    assert torch.equal(a, b)


def test_ground_truth_uploader_parity(D, dev, nocs):
    items, _, masks, depths = nocs
    mk = lambda: D.GroundTruthUploader(4, 48, 64, 4, device=dev, slots=2, max_instances=16, with_depth=True)
    host, devp = mk(), mk()
    for it in range(5):
        o = [(it + j) % 4 for j in range(4)]
        args = ([masks[j] for j in o], [items[j] for j in o])
        a, ea = host.upload_png(*args, depth_files=[depths[j] for j in o])
        b, eb = devp.upload_png(*args, depth_files=[depths[j] for j in o], decode="device")
        ea.synchronize()
        eb.synchronize()
        assert torch.equal(a["mask"], b["mask"]) and torch.equal(a["depth"], b["depth"]), it
        assert list(a["agg_data"]) == list(b["agg_data"])
        for key in a["agg_data"]:
            assert torch.equal(a["agg_data"][key], b["agg_data"][key]), (it, key)
    devp.check_decoded()
    devp.upload_png([masks[0], wrong_adler(masks[1])], items[:2], depth_files=depths[:2], decode="device")
    with pytest.raises(RuntimeError, match="file 1"):
        devp.upload_png(masks, items, depth_files=depths, decode="device")      # the slot comes round again: slots = 2
        devp.upload_png(masks, items, depth_files=depths, decode="device")
