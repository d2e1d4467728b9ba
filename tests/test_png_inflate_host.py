"""csrc/inflate.hpp on the host (fpc_inflate_host: the template the device kernel k_png_inflate instantiates) against
zlib.decompress, damaged streams with one status per failure class, and the host pre-pass fpc_png_pack_batch.  The
damaged streams run here only: no GPU test feeds them to a kernel."""
import ctypes
import os
import re
import struct
import zlib

import numpy as np
import pytest

from oracle import png_oracle as po

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PNG_DIR = os.path.join(REPO, "tests", "golden", "png")
CANARY = 0xA5


@pytest.fixture(scope="module")
def L():
    from fastposecnn_amd import build, _native
    build.build()
    return _native.lib()


@pytest.fixture(scope="module")
def codes():
    hdr = open(os.path.join(REPO, "include", "fpc.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (FPC_(?:INF|PNG)_E[A-Z_]+) (\d+)", hdr)}


def inflate(L, z, cap):
    """-> (status, bytes produced); 64 canary bytes on both sides of `out` must survive whatever the stream is."""
    zb = np.frombuffer(bytes(z), np.uint8) if len(z) else np.zeros(1, np.uint8)
    out = np.full(cap + 128, CANARY, np.uint8)
    n = ctypes.c_size_t(0)
    rc = L.fpc_inflate_host(zb.ctypes.data, len(z), out.ctypes.data + 64, cap, ctypes.byref(n))
    assert (out[:64] == CANARY).all() and (out[64 + cap:] == CANARY).all(), "wrote outside [out, out + cap)"
    assert n.value <= cap
    return rc, out[64:64 + n.value].tobytes()


def roundtrip(L, raw, z):
    assert zlib.decompress(z) == raw
    rc, got = inflate(L, z, len(raw))
    assert rc == 0 and got == raw, (rc, len(got), len(raw))


def deflate(raw, strategy, level=6, wbits=15):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, strategy)
    return c.compress(raw) + c.flush()


def first_block(z):
    """(BFINAL, BTYPE) of the first block of a zlib stream."""
    return z[2] & 1, (z[2] >> 1) & 3


def idat(png):
    return b"".join(body for typ, body in po._chunks(png) if typ == b"IDAT")


# ------------------------------------------------------------------------------------------------------ valid streams

def test_two_stored_blocks(L):
    z = zlib.compress(bytes(70000), 0)
    assert first_block(z) == (0, 0)
    roundtrip(L, bytes(70000), z)


def test_fixed_huffman_blocks(L):
    raw = np.tile(np.arange(97, dtype=np.uint8), 40).tobytes()
    z = deflate(raw, zlib.Z_FIXED)
    assert first_block(z)[1] == 1
    roundtrip(L, raw, z)
    z = zlib.compress(raw, 6)
    assert first_block(z)[1] == 1
    roundtrip(L, raw, z)


def test_dynamic_blocks_rle_and_literals_only(L):
    raw = np.repeat(np.arange(50, dtype=np.uint8), 60).tobytes()
    for strategy in (zlib.Z_RLE, zlib.Z_HUFFMAN_ONLY):
        z = deflate(raw, strategy)
        assert first_block(z)[1] == 2
        roundtrip(L, raw, z)


def test_every_fixture_idat_stream(L):
    names = sorted(f for f in os.listdir(PNG_DIR) if f.endswith(".png"))
    assert len(names) >= 10
    for name in names:
        z = idat(open(os.path.join(PNG_DIR, name), "rb").read())
        roundtrip(L, zlib.decompress(z), z)


def far_match_stream(head, tail_len, distance):
    """`head` as one stored block, then a fixed-Huffman block that copies tail_len bytes from `distance` back (zlib's own
    deflate never looks further back than 32 768 - 262, so the stream is written here)."""
    b = Bits().put(0, 1).put(0, 2).put(0, 5).put(len(head), 16).put(len(head) ^ 0xffff, 16)
    for v in head:
        b.put(v, 8)
    b.put(1, 1).put(1, 2)
    left = tail_len
    while left:
        n = 258 if left >= 258 + 3 or left == 258 else min(left - 3, 200) if left > 258 else left
        sym = max(i for i in range(29) if LBASE[i] <= n)
        code = 257 + sym
        b.code(code - 256, 7) if code < 280 else b.code(0xC0 + code - 280, 8)
        b.put(n - LBASE[sym], LEXT[sym])
        b.code(29, 5).put(distance - 24577, 13)
        left -= n
    b.code(0, 7)
    return bytes(b.out) + (bytes([b.acc]) if b.n else b"")


LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]


@pytest.mark.parametrize("rows_apart, width", [(17, 1921), (16, 2048)])
def test_distances_just_under_the_window(L, rows_apart, width):
    """Two identical rows 17 x 1921 = 32 657 bytes apart (and, 16 x 2048, exactly the window: 32 768)."""
    r = np.random.default_rng(5)
    rows = r.integers(0, 256, (rows_apart + 1, width), dtype=np.uint8)
    rows[rows_apart] = rows[0]
    raw = rows.tobytes()
    body = far_match_stream(raw[:rows_apart * width], width, rows_apart * width)
    assert zlib.decompressobj(-15).decompress(body) == raw
    with pytest.raises(zlib.error):                      # the distances are real: a 512-byte window does not reach them
        zlib.decompressobj(-9).decompress(body)
    z = b"\x78\xda" + body + struct.pack(">I", zlib.adler32(raw))
    roundtrip(L, raw, z)
    assert inflate(L, header(cinfo=6) + z[2:], len(raw))[0] != 0          # nor does a declared 16 KiB window


def test_seeded_random_mixtures(L):
    r = np.random.default_rng(20261019)
    for _ in range(50):
        parts = []
        for _ in range(int(r.integers(1, 7))):
            kind, n = int(r.integers(0, 4)), int(r.integers(1, 40000))
            if kind == 0:
                parts.append(r.integers(0, 256, n, dtype=np.uint8).tobytes())
            elif kind == 1:
                parts.append(bytes([int(r.integers(0, 256))]) * n)
            elif kind == 2:
                parts.append(r.integers(0, 4, n, dtype=np.uint8).tobytes())
            else:
                parts.append((b"".join(parts))[-n:] or b"x")          # a repeat of earlier output: long distances
        raw = b"".join(parts)
        strategy = [zlib.Z_DEFAULT_STRATEGY, zlib.Z_FILTERED, zlib.Z_RLE, zlib.Z_FIXED][int(r.integers(0, 4))]
        roundtrip(L, raw, deflate(raw, strategy, int(r.integers(0, 10))))


# ---------------------------------------------------------------------------------------------------- damaged streams

class Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, count):                          # LSB first (header fields, extra bits)
        for i in range(count):
            self.acc |= ((value >> i) & 1) << self.n
            self.n += 1
            if self.n == 8:
                self.out.append(self.acc)
                self.acc, self.n = 0, 0
        return self

    def code(self, value, count):                         # a Huffman code: most significant bit first
        for i in reversed(range(count)):
            self.put((value >> i) & 1, 1)
        return self

    def done(self, pad=4):
        if self.n:
            self.out.append(self.acc)
        return b"\x78\x9c" + bytes(self.out) + bytes(pad)


def fixed_literal(b, byte):
    return b.code(0x30 + byte, 8) if byte < 144 else b.code(0x190 + byte - 144, 9)


ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def dynamic_header(cl):
    """BFINAL = 1, BTYPE = 2, HLIT = 257, HDIST = 1 and the code-length code lengths `cl` (symbol -> length)."""
    b = Bits().put(1, 1).put(2, 2).put(0, 5).put(0, 5)
    last = max(i for i, s in enumerate(ORDER) if cl.get(s, 0)) + 1
    last = max(last, 4)
    b.put(last - 4, 4)
    for s in ORDER[:last]:
        b.put(cl.get(s, 0), 3)
    return b


def header(cm=8, cinfo=7, fdict=0):
    cmf, flg = (cinfo << 4) | cm, fdict << 5
    flg += (31 - ((cmf << 8) + flg) % 31) % 31
    return bytes([cmf, flg])


def test_damaged_streams_one_status_per_class(L, codes):
    good_raw = b"hello hello hello hello world" * 3
    good = zlib.compress(good_raw, 6)
    cases = {
        "FPC_INF_EBLOCK_TYPE": (Bits().put(1, 1).put(3, 2).done(), 16),
        "FPC_INF_ESTORED_LEN": (b"\x78\x01\x01\x05\x00\x00\x00hello" + bytes(4), 5),
        "FPC_INF_EOVERSUBSCRIBED": (dynamic_header({s: 1 for s in ORDER}).done(), 16),
        "FPC_INF_EINCOMPLETE": (dynamic_header({0: 1}).done(), 16),
        "FPC_INF_EREPEAT_FIRST": (dynamic_header({16: 1, 0: 1}).code(1, 1).put(0, 2).done(), 16),
        "FPC_INF_ELITLEN_SYMBOL": (fixed_literal(Bits().put(1, 1).put(1, 2), 65).code(0xC6, 8).done(), 16),
        "FPC_INF_EDIST_SYMBOL": (fixed_literal(Bits().put(1, 1).put(1, 2), 65).code(1, 7).code(30, 5).done(), 16),
        "FPC_INF_EDIST_TOO_FAR": (fixed_literal(Bits().put(1, 1).put(1, 2), 65).code(1, 7).code(1, 5).done(), 16),
        "FPC_INF_EOUT_OVERFLOW": (good, len(good_raw) - 1),
        "FPC_INF_EOUT_SHORT": (good, len(good_raw) + 1),
        "FPC_INF_EADLER": (good[:-1] + bytes([good[-1] ^ 1]), len(good_raw)),
        "FPC_INF_EFDICT": (header(fdict=1) + good[2:], len(good_raw)),
        "FPC_INF_EMETHOD": (header(cm=9) + good[2:], len(good_raw)),
        "FPC_INF_ETRUNCATED": (good[:len(good) // 2], len(good_raw)),
    }
    seen = {}
    for name, (z, cap) in cases.items():
        rc, _ = inflate(L, z, cap)
        assert rc == codes[name] != 0, (name, rc)
        seen[name] = rc
    assert len(set(seen.values())) == len(cases) == 14
    # the second literal/length and distance symbols of each pair, and a window the header declares smaller than the distance
    assert inflate(L, fixed_literal(Bits().put(1, 1).put(1, 2), 65).code(0xC7, 8).done(), 16)[0] == codes["FPC_INF_ELITLEN_SYMBOL"]
    assert inflate(L, fixed_literal(Bits().put(1, 1).put(1, 2), 65).code(1, 7).code(31, 5).done(), 16)[0] == codes["FPC_INF_EDIST_SYMBOL"]
    assert inflate(L, header(cinfo=8) + good[2:], len(good_raw))[0] == codes["FPC_INF_EMETHOD"]
    assert inflate(L, good, len(good_raw)) == (0, good_raw)


def test_truncation_at_every_byte(L, codes):
    r = np.random.default_rng(3)
    raws = [r.integers(0, 256, 200, dtype=np.uint8).tobytes(),                      # stored at level 0
            b"abcabcabcabd" * 9,                                                    # fixed
            bytes(r.integers(0, 6, 600, dtype=np.uint8))]                           # dynamic
    kinds = []
    for raw, level in zip(raws, (0, 6, 9)):
        z = zlib.compress(raw, level)
        assert len(z) <= 300
        kinds.append(first_block(z)[1])
        for k in range(len(z)):
            rc, got = inflate(L, z[:k], len(raw))
            assert rc != 0 and raw.startswith(got), (level, k, rc)
            if k < len(z) - 4:
                assert rc == codes["FPC_INF_ETRUNCATED"], (level, k, rc)
        assert inflate(L, z, len(raw)) == (0, raw)
    assert kinds == [0, 1, 2]


def test_flipped_bits_never_write_outside(L):
    """Any status is fine for a stream with a flipped bit (some still decode); the canaries and `cap` are what is checked."""
    r = np.random.default_rng(11)
    raw = bytes(r.integers(0, 5, 3000, dtype=np.uint8)) + bytes(500)
    z = bytearray(zlib.compress(raw, 9))
    for _ in range(400):
        bad = bytearray(z)
        bad[int(r.integers(2, len(z)))] ^= 1 << int(r.integers(0, 8))
        rc, got = inflate(L, bad, len(raw))
        assert rc != 0 or got == raw


def test_invalid_arguments(L):
    out = np.zeros(8, np.uint8)
    assert L.fpc_inflate_host(None, 4, out.ctypes.data, 8, None) == -1
    assert L.fpc_inflate_host(out.ctypes.data, 4, None, 8, None) == -1
    assert L.fpc_inflate_host(out.ctypes.data, 1 << 31, out.ctypes.data, 8, None) == -1
    assert L.fpc_inflate_host(out.ctypes.data, 4, out.ctypes.data, 1 << 31, None) == -1


# ---------------------------------------------------------------------------------------------------------- pre-pass

def pack(L, files, H, W, mode, staging_bytes=None):
    n = len(files)
    nbytes = L.fpc_png_pack_bytes(n, H, W) if staging_bytes is None else staging_bytes
    raw = np.full(nbytes + 16 + 64, CANARY, np.uint8)
    off = (-raw.ctypes.data) % 16
    staging = raw[off:off + nbytes]
    desc = np.full((n, 8), -7, np.int64)
    bufs = [np.frombuffer(f, np.uint8) for f in files]
    ptrs = (ctypes.c_void_p * n)(*[b.ctypes.data for b in bufs])
    sizes = (ctypes.c_size_t * n)(*[b.size for b in bufs])
    used = ctypes.c_size_t(0)
    rc = L.fpc_png_pack_batch(ptrs, sizes, n, H, W, mode, staging.ctypes.data, nbytes, desc.ctypes.data, ctypes.byref(used))
    assert (raw[off + nbytes:] == CANARY).all() and (raw[:off] == CANARY).all()
    return rc, staging, desc, used.value


@pytest.mark.parametrize("split", [1, 7, 100, None])
def test_pack_descriptors_and_payload(L, split):
    r = np.random.default_rng(2)
    imgs = [r.integers(0, 256, (9, 13, 3), dtype=np.uint8), r.integers(0, 3, (9, 13, 4), dtype=np.uint8),
            r.integers(0, 256, (9, 13), dtype=np.uint16)]
    files = [po.encode(a, idat_split=split) for a in imgs]
    rc, staging, desc, used = pack(L, files, 9, 13, 3)
    assert rc == 0
    o = 0
    for i, (a, f) in enumerate(zip(imgs, files)):
        z = idat(f)
        depth = 16 if a.dtype == np.uint16 else 8
        ch = 1 if a.ndim == 2 else a.shape[2]
        assert desc[i].tolist() == [o, len(z), 13, 9, depth, {1: 0, 3: 2, 4: 6}[ch], ch, 0]
        assert o % 16 == 0 and staging[o:o + len(z)].tobytes() == z
        pad = (-len(z)) % 16
        assert not staging[o + len(z):o + len(z) + pad].any()
        o += len(z) + pad
    assert used == o and (staging[o:] == CANARY).all()
    # mode 0 wants one (depth, channels) as well as one size
    assert pack(L, files, 9, 13, 0)[0] == -1
    assert pack(L, files[:1] * 2, 9, 13, 0)[0] == 0


def test_pack_carries_the_palette(L):
    r = np.random.default_rng(4)
    pal = r.integers(0, 256, (5, 3), dtype=np.uint8)
    f = po.encode(r.integers(0, 5, (6, 7), dtype=np.uint8), palette=pal)
    rc, staging, desc, used = pack(L, [f, f], 6, 7, 3)
    z = idat(f)
    assert rc == 0 and desc[0].tolist() == [0, len(z), 7, 6, 8, 3, 1, 5]
    p = (len(z) + 15) // 16 * 16
    assert staging[p:p + 15].tobytes() == pal.tobytes() and not staging[p + 15:p + 768].any()
    assert desc[1, 0] == p + 768 and used == 2 * (p + 768)


def test_pack_refuses_what_the_host_decoder_refuses(L):
    good = po.encode(np.arange(5 * 6 * 3, dtype=np.uint8).reshape(5, 6, 3))
    at = good.index(b"IDAT")
    bad_crc = bytearray(good)
    bad_crc[at + 6] ^= 1
    ihdr = bytearray(good[16:29])
    ihdr[12] = 1
    interlaced = good[:16] + bytes(ihdr) + struct.pack(">I", zlib.crc32(b"IHDR" + bytes(ihdr))) + good[33:]
    from fastposecnn_amd.tools import dataset as D
    for f in (bytes(bad_crc), b"\x88" + good[1:], interlaced, good[:at + 9]):
        rc, staging, desc, used = pack(L, [good, f], 5, 6, 3)
        assert rc == -5
        with pytest.raises(RuntimeError):
            D.imread_png(f)
    assert pack(L, [good, good], 5, 6, 3)[0] == 0


def test_pack_mixed_sizes_writes_nothing(L):
    a = po.encode(np.zeros((5, 6, 3), np.uint8))
    b = po.encode(np.zeros((5, 7, 3), np.uint8))
    rc, staging, desc, used = pack(L, [a, b], 5, 6, 3)
    assert rc == -1 and used == 0
    assert (staging == CANARY).all() and (desc == -7).all()
    rc, staging, desc, used = pack(L, [a, a], 5, 6, 3, staging_bytes=32)
    assert rc == -2                                       # FPC_EWORKSPACE: the payloads do not fit


def test_pack_bytes_covers_level_0(L):
    r = np.random.default_rng(6)
    a = r.integers(0, 65536, (40, 50, 4), dtype=np.uint16)          # 8 bytes a pixel, stored blocks
    f = po.encode(a, level=0)
    assert len(idat(f)) > a.nbytes
    assert pack(L, [f], 40, 50, 3, staging_bytes=L.fpc_png_pack_bytes(1, 40, 50))[0] == 0
    assert L.fpc_png_pack_bytes(0, 40, 50) == 0


def test_entries_are_declared_exported_and_bound(L):
    from fastposecnn_amd import _native
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "fpc.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_native.LIB_PATH)
    for name in ("fpc_inflate_host", "fpc_png_pack_bytes", "fpc_png_pack_batch", "fpc_png_decode_device",
                 "fpc_png_decode_device_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(raw, name) and name in _native.EXPORTED
    assert "#define FPC_ABI_VERSION 11" in hdr and L.fpc_abi_version() == 11


def test_device_entry_refuses_bad_arguments_before_any_launch(L):
    """No GPU is needed: every refusal comes before the first HIP call."""
    f = L.fpc_png_decode_device
    ok = dict(staging=4096, sbytes=1024, desc=8192, n=2, H=4, W=4, mode=3, bpp=4, out=16384, frame=48, status=32768, ws=65536,
              wsb=1 << 20)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["staging"], a["sbytes"], a["desc"], a["n"], a["H"], a["W"], a["mode"], a["bpp"], a["out"], a["frame"],
                 a["status"], a["ws"], a["wsb"], None)

    for key in ("staging", "desc", "out", "status", "ws"):
        assert call(**{key: None}) == -1, key
    for key, value in (("staging", 4100), ("desc", 8196), ("out", 16392), ("status", 32770), ("ws", 65544)):
        assert call(**{key: value}) == -1, key
    assert call(n=0) == -1 and call(mode=1) == -1 and call(bpp=9) == -1 and call(frame=47) == -1
    assert call(sbytes=1 << 31) == -1 and call(frame=1 << 30) == -1
    assert call(H=65535, W=4096, bpp=8) == -1             # n raw slices beyond 2^31
    assert call(W=8193, frame=3 * 4 * 8193) == -1         # W * bpp beyond the un-filter kernel's row buffer
    assert call(wsb=16) == -2
    assert L.fpc_png_decode_device_workspace_bytes(2, 4, 4, 4) == 2 * 80
