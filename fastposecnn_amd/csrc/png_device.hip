// png_device.hip — PNG decoding on the device (opt-in, `decode="device"` of the two uploaders): the host walks the
// container and copies the COMPRESSED bytes (fpc_png_pack_batch), the device inflates and un-filters them
// (fpc_png_decode_device: k_png_inflate, then k_png_unfilter).  The host decoder (png_decode.hip) is untouched and stays
// the default; both read the header with png_header.hpp and refuse the same containers.
//
// k_png_inflate: one wave (one 64-lane workgroup) per file runs inflate.hpp.  The decode state is wave-uniform and kept
// scalar (readfirstlane on everything read from LDS); the lanes share the refill of the input stage (64 x 16 bytes of
// the staged stream per fetch), the match copies, the table fills and the flush of the 32 KiB LDS window to the raw
// scanline buffer in 16-byte stores.  A match is always read from the LDS window, never from what the wave stored to
// global memory.  LDS per workgroup: 32768 (window) + 1024 (input stage) + 10304 (tables) = 44096 bytes: three
// workgroups per CU.  No atomics.
//
// k_png_unfilter: one wave per file, raw scanlines [H][1 + stride] -> `out` in the requested mode.  Diagonal schedule:
// in a band of 64 rows lane r works on row y0 + r, one pixel behind lane r - 1, so that the pixel above (and, one step
// later, above-left) arrives by a lane shuffle from lane r - 1; lane 0 reads the band's upper neighbour row from LDS,
// where lane 63 of the previous band left it.  LDS: 32768 (that row) + 768 (palette).  W * bpp <= 32768 (FPC_EINVAL
// otherwise).  A filter byte > 4 is reported in `status` and its row is read as filter 0.
//
// Every access of a file stays inside its own slices whatever its bytes are: the staged stream [offset, offset +
// align16(zbytes)) (+ 768 palette bytes), its raw slice of the workspace, its frame of `out`, its `status` word.
#include <zlib.h>          // crc32 of the chunk walk only (host); the inflater is inflate.hpp

#include <vector>

#include "common.hpp"
#include "inflate.hpp"
#include "png_header.hpp"

namespace {

using namespace fpc_inflate;

constexpr int kDescWords = FPC_PNG_DESC_WORDS;           // int64 per file: offset, zbytes, w, h, depth, ctype, channels, palette_n
constexpr int kMaxStride = 32768;                        // W * bpp of the device path
constexpr size_t kLimit = (size_t)1 << 31;

inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

// ---------------------------------------------------------------------------------------------------- host inflater

struct HostIO {
    static constexpr int kLanes = 1;
    uint8_t* ring;
    Tables* t;
    const uint8_t* in;
    uint8_t* out;
    int lane() const { return 0; }
    uint32_t uni(uint32_t v) const { return v; }
    uint32_t sum(uint32_t v) const { return v; }
    void sync() const {}
    uint32_t in32(uint32_t pos) const { uint32_t v; memcpy(&v, in + pos, 4); return v; }
    uint32_t in8(uint32_t pos) const { return in[pos]; }
    void store_piece(uint32_t pos, const uint8_t* src, uint32_t nb) const { memcpy(out + pos, src, nb); }
    struct Peek { const uint16_t* tab; uint64_t bb; uint32_t mask; };
    Peek peek_all(const uint16_t* tab, uint64_t bb, uint32_t mask) const { return Peek{tab, bb, mask}; }
    uint32_t peek_at(const Peek& h, uint32_t pos) const { return h.tab[(uint32_t)(h.bb >> pos) & h.mask]; }
    void lit_put(uint32_t op, uint32_t k, uint32_t byte) const { ring[(op + k) & (uint32_t)(kRing - 1)] = (uint8_t)byte; }
    void lit_commit(uint32_t, uint32_t) const {}
};

// ------------------------------------------------------------------------------------------------------ device side

struct Desc { uint32_t offset, zbytes, depth, ctype, channels, pn, bpp, expect; };

// the descriptor of `file`, checked against the launch's geometry: nothing below trusts a word it did not check here.
// (Inlined: out of line, `d` is handed over in private memory, whose loads count as lane-varying, and with them the whole
// decode state: every branch of the inflater then runs under an exec mask, at three times the instructions.)
__device__ __forceinline__ int load_desc(const int64_t* __restrict__ desc, int file, int H, int W, int mode, int max_bpp, size_t staging_bytes,
                         size_t frame_bytes, Desc& d) {
    const int64_t* q = desc + (size_t)file * kDescWords;
    const int64_t off = q[0], zb = q[1], w = q[2], h = q[3], depth = q[4], ctype = q[5], ch = q[6], pn = q[7];
    if (w != W || h != H || (depth != 8 && depth != 16)) return FPC_PNG_EDESC;
    const int want = ctype == 0 ? 1 : ctype == 2 ? 3 : ctype == 3 ? 1 : ctype == 4 ? 2 : ctype == 6 ? 4 : 0;
    if (want == 0 || ch != want || (ctype == 3 && (depth != 8 || pn < 1 || pn > 256))) return FPC_PNG_EDESC;
    const int bpp = (int)(ch * depth / 8);
    if (bpp > max_bpp) return FPC_PNG_EDESC;
    if (off < 0 || (off & 15) || zb < 1 || (uint64_t)off >= staging_bytes) return FPC_PNG_EDESC;
    const uint64_t need = (((uint64_t)zb + 15u) & ~(uint64_t)15u) + (ctype == 3 ? 768u : 0u);
    if (need > staging_bytes - (uint64_t)off) return FPC_PNG_EDESC;
    const uint64_t obpp = mode == 3 || ctype == 3 ? 3u : (uint64_t)bpp;
    if ((uint64_t)H * W * obpp > frame_bytes) return FPC_PNG_EDESC;
    d.offset = (uint32_t)off; d.zbytes = (uint32_t)zb; d.depth = (uint32_t)depth; d.ctype = (uint32_t)ctype;
    d.channels = (uint32_t)ch; d.pn = (uint32_t)pn; d.bpp = (uint32_t)bpp;
    d.expect = (uint32_t)H * (1u + (uint32_t)W * (uint32_t)bpp);
    return 0;
}

struct DevIO {
    static constexpr int kLanes = 64;
    uint8_t* ring;
    Tables* t;
    uint8_t* stage;              // LDS, 1024 bytes of the stream from `sb`
    const uint8_t* in;
    uint32_t n16;                // the staged stream's bytes, rounded up to 16 (its slice)
    uint8_t* out;
    uint32_t sb;
    int lits;                    // the literals of the current run, the k-th in lane k

    __device__ int lane() const { return (int)threadIdx.x; }
    __device__ uint32_t uni(uint32_t v) const { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
    __device__ uint32_t sum(uint32_t v) const {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
        return uni(v);
    }
    __device__ void sync() const { __syncthreads(); }
    __device__ void fetch(uint32_t pos) {
        const uint32_t base = pos & ~1023u;
        if (base == sb) return;
        __syncthreads();
        const uint32_t off = base + 16u * threadIdx.x;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (off < n16) v = *reinterpret_cast<const uint4*>(in + off);
        *reinterpret_cast<uint4*>(stage + 16u * threadIdx.x) = v;
        sb = base;
        __syncthreads();
    }
    __device__ uint32_t in32(uint32_t pos) {
        fetch(pos);
        return uni(*reinterpret_cast<const uint32_t*>(stage + (pos & 1023u)));      // pos % 4 == 0 (inflate.hpp: refill)
    }
    __device__ uint32_t in8(uint32_t pos) {
        fetch(pos);
        return uni(stage[pos & 1023u]);
    }
    __device__ int peek_all(const uint16_t* tab, uint64_t bb, uint32_t mask) const { return tab[(uint32_t)(bb >> threadIdx.x) & mask]; }
    __device__ uint32_t peek_at(int h, uint32_t pos) const { return (uint32_t)__builtin_amdgcn_readlane(h, (int)pos); }
    __device__ void lit_put(uint32_t, uint32_t k, uint32_t byte) { lits = threadIdx.x == k ? (int)byte : lits; }
    __device__ void lit_commit(uint32_t op, uint32_t k) const {
        if (threadIdx.x < k) ring[(op + threadIdx.x) & (uint32_t)(kRing - 1)] = (uint8_t)lits;
    }
    // the raw slice is padded to 16 bytes: the last piece is stored whole, zero beyond its nb bytes
    __device__ void store_piece(uint32_t pos, const uint8_t* src, uint32_t nb) const {
        uint4 v = *reinterpret_cast<const uint4*>(src);
        uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t keep = nb > 4 * k ? nb - 4 * k : 0;
            if (keep < 4) w[k] &= keep ? (1u << (8 * keep)) - 1u : 0u;
        }
        *reinterpret_cast<uint4*>(out + pos) = make_uint4(w[0], w[1], w[2], w[3]);
    }
};

__global__ __launch_bounds__(64) void k_png_inflate(const uint8_t* __restrict__ staging, size_t staging_bytes,
                                                    const int64_t* __restrict__ desc, int H, int W, int mode, int max_bpp,
                                                    size_t frame_bytes, uint8_t* __restrict__ raw, size_t raw_slice,
                                                    int32_t* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) uint8_t ring[kRing];
    __shared__ __attribute__((aligned(16))) uint8_t stage[1024];
    __shared__ Tables tables;
    const int file = blockIdx.x;
    Desc d;
    int st = load_desc(desc, file, H, W, mode, max_bpp, staging_bytes, frame_bytes, d);
    if (st == 0 && (size_t)d.expect > raw_slice) st = FPC_PNG_EDESC;
    if (st == 0) {
        DevIO io{ring, &tables, stage, staging + d.offset, (d.zbytes + 15u) & ~15u, raw + (size_t)file * raw_slice, 0xffffffffu, 0};
        Inflater<DevIO> inf(io);
        uint32_t produced = 0;
        st = inf.run(d.zbytes, d.expect, &produced);
    }
    if (threadIdx.x == 0) status[file] = st;
}

__device__ __forceinline__ int paeth_dev(int a, int b, int c) {
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ __forceinline__ uint64_t shfl_up1(uint64_t v) {
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, 1, 64), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), 1, 64);
    return ((uint64_t)hi << 32) | lo;
}

__global__ __launch_bounds__(64) void k_png_unfilter(const uint8_t* __restrict__ staging, size_t staging_bytes,
                                                     const int64_t* __restrict__ desc, int H, int W, int mode, int max_bpp,
                                                     uint8_t* __restrict__ out, size_t frame_bytes,
                                                     const uint8_t* __restrict__ raw_all, size_t raw_slice,
                                                     int32_t* __restrict__ status) {
    __shared__ uint8_t above[kMaxStride];        // the row over the current band (the previous band's last row)
    __shared__ uint8_t pal[768];
    const int file = blockIdx.x, lane = threadIdx.x;
    if (status[file] != 0) return;               // k_png_inflate's verdict; the frame of `out` is left as it was
    Desc d;
    if (load_desc(desc, file, H, W, mode, max_bpp, staging_bytes, frame_bytes, d) != 0) return;      // (it passed there)
    const int bpp = (int)d.bpp, sb = (int)d.depth / 8;
    const size_t stride = (size_t)W * bpp;
    if (stride > (size_t)kMaxStride) return;     // refused on the host before the launch
    const uint8_t* raw = raw_all + (size_t)file * raw_slice;
    uint8_t* o = out + (size_t)file * frame_bytes;
    if (d.ctype == 3) {
        const uint8_t* p = staging + d.offset + ((d.zbytes + 15u) & ~15u);
        for (int i = lane; i < 768; i += 64) pal[i] = p[i];
    }
    __syncthreads();
    const bool to_rgb = mode == 3 || d.ctype == 3;
    bool bad = false;
    for (int y0 = 0; y0 < H; y0 += 64) {
        const int y = y0 + lane, rows = H - y0 < 64 ? H - y0 : 64;
        const bool active = y < H;
        const uint8_t* line = raw + (size_t)(active ? y : 0) * (stride + 1);
        int ft = active ? line[0] : 0;
        if (ft > 4) { bad = true; ft = 0; }
        uint64_t a = 0, c = 0, mine = 0;          // left, above-left, this lane's last pixel: bpp bytes each, byte k at bits 8k
        const int steps = W + rows - 1;
        for (int t0 = 0; t0 < steps; t0 += 4) {
            uint64_t f[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {         // the four steps' raw bytes are asked for before the first is used
                const int x = t0 + j - lane;
                f[j] = 0;
                if (active && x >= 0 && x < W)
                    for (int k = 0; k < bpp; ++k) f[j] |= (uint64_t)line[1 + (size_t)x * bpp + k] << (8 * k);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int x = t0 + j - lane;
                uint64_t b = shfl_up1(mine);      // lane r - 1 finished pixel x of the row above one step ago
                const bool valid = active && x >= 0 && x < W;
                if (!valid) continue;
                if (lane == 0) {
                    b = 0;
                    if (y > 0)
                        for (int k = 0; k < bpp; ++k) b |= (uint64_t)above[(size_t)x * bpp + k] << (8 * k);
                }
                uint64_t r = 0;
                for (int k = 0; k < bpp; ++k) {
                    const int fk = (int)(f[j] >> (8 * k)) & 255, ak = (int)(a >> (8 * k)) & 255, bk = (int)(b >> (8 * k)) & 255,
                              ck = (int)(c >> (8 * k)) & 255;
                    const int pred = ft == 0 ? 0 : ft == 1 ? ak : ft == 2 ? bk : ft == 3 ? (ak + bk) >> 1 : paeth_dev(ak, bk, ck);
                    r |= (uint64_t)((fk + pred) & 255) << (8 * k);
                }
                a = r; c = b; mine = r;
                if (lane == 63)
                    for (int k = 0; k < bpp; ++k) above[(size_t)x * bpp + k] = (uint8_t)(r >> (8 * k));
                const size_t px = (size_t)y * W + x;
                if (to_rgb) {
                    uint8_t* q = o + px * 3;
                    if (d.ctype == 3) {
                        const int i = (int)(r & 255) < (int)d.pn ? (int)(r & 255) : 0;
                        q[0] = pal[3 * i]; q[1] = pal[3 * i + 1]; q[2] = pal[3 * i + 2];
                    } else if (d.channels <= 2) {
                        q[0] = q[1] = q[2] = (uint8_t)r;
                    } else {
                        q[0] = (uint8_t)r; q[1] = (uint8_t)(r >> (8 * sb)); q[2] = (uint8_t)(r >> (16 * sb));
                    }
                } else if (sb == 1) {
                    uint8_t* q = o + px * bpp;
                    for (int k = 0; k < bpp; ++k) q[k] = (uint8_t)(r >> (8 * k));
                } else {                          // big-endian samples -> u16 little-endian
                    uint8_t* q = o + px * bpp;
                    for (int k = 0; k < bpp; ++k) q[k ^ 1] = (uint8_t)(r >> (8 * k));
                }
            }
        }
        __syncthreads();                          // lane 63's row is complete before lane 0 of the next band reads it
    }
    const bool any_bad = __ballot(bad) != 0;
    if (lane == 0 && any_bad) status[file] = FPC_PNG_EFILTER;
}

}  // namespace

extern "C" int fpc_inflate_host(const uint8_t* in, size_t zbytes, uint8_t* out, size_t cap, size_t* out_len) {
    if (!in || (!out && cap) || zbytes >= kLimit || cap >= kLimit) return FPC_EINVAL;
    try {
        std::vector<uint8_t> ring(kRing);
        std::vector<Tables> tables(1);
        HostIO io{ring.data(), tables.data(), in, out};
        Inflater<HostIO> inf(io);
        uint32_t produced = 0;
        const int st = inf.run((uint32_t)zbytes, (uint32_t)cap, &produced);
        if (out_len) *out_len = produced;
        return st;
    } catch (...) {
        return FPC_EINVAL;
    }
}

extern "C" size_t fpc_png_pack_bytes(int n, int H, int W) {
    if (n < 1 || H < 1 || W < 1 || H > 65535 || W > 65535) return 0;
    const size_t raw = (size_t)H * (1 + (size_t)W * 8);
    return (size_t)n * (align16(raw + raw / 8 + 1024) + 768);
}

extern "C" int fpc_png_pack_batch(const uint8_t* const* datas, const size_t* sizes, int n, int H, int W, int mode,
                                  uint8_t* staging, size_t staging_bytes, int64_t* desc, size_t* used) {
    if (n < 1 || H < 1 || W < 1 || !datas || !sizes || !staging || !desc || !used) return FPC_EINVAL;
    if ((mode != 0 && mode != 3) || ((uintptr_t)staging & 15) || staging_bytes >= kLimit) return FPC_EINVAL;
    std::vector<PngHeader> hs((size_t)n);
    for (int i = 0; i < n; ++i) {                     // every file is checked before a byte is written, as fpc_png_decode_batch
        if (!datas[i]) return FPC_EINVAL;
        const int rc = parse_header(datas[i], sizes[i], hs[i]);
        if (rc != FPC_OK) return rc;
        if ((int)hs[i].w != W || (int)hs[i].h != H) return FPC_EINVAL;
        const int c0 = hs[0].ctype == 3 ? 3 : hs[0].channels, ci = hs[i].ctype == 3 ? 3 : hs[i].channels;
        if (mode == 0 && (hs[i].depth != hs[0].depth || ci != c0)) return FPC_EINVAL;
        if ((size_t)H * ((size_t)W * hs[i].bpp + 1) > ((size_t)1 << 30)) return FPC_EFORMAT;      // png_decode.hip's limit
    }
    size_t o = 0;
    for (int i = 0; i < n; ++i) {
        const uint8_t* d = datas[i];
        const size_t nb = sizes[i], start = o;
        const PngHeader& h = hs[i];
        uint8_t palette[768];
        memset(palette, 0, sizeof(palette));
        int pn = 0;
        size_t c = 8;
        bool end = false;
        while (c + 12 <= nb && !end) {
            const uint32_t len = be32(d + c);
            const uint8_t* typ = d + c + 4;
            if ((size_t)len > nb - c - 12) return FPC_EFORMAT;
            const uint8_t* body = d + c + 8;
            if ((uint32_t)crc32(crc32(0L, Z_NULL, 0), typ, 4 + len) != be32(body + len)) return FPC_EFORMAT;
            if (memcmp(typ, "IDAT", 4) == 0) {
                if (len > staging_bytes || o > staging_bytes - len) return FPC_EWORKSPACE;
                memcpy(staging + o, body, len);
                o += len;
            } else if (memcmp(typ, "PLTE", 4) == 0) {
                if (len % 3 != 0 || len > 768) return FPC_EFORMAT;
                memcpy(palette, body, len);
                pn = (int)(len / 3);
            } else if (memcmp(typ, "IEND", 4) == 0) {
                end = true;
            }
            c += 12 + (size_t)len;
        }
        const size_t zbytes = o - start;
        if (zbytes == 0 || (h.ctype == 3 && pn == 0)) return FPC_EFORMAT;
        const size_t padded = align16(o) + (h.ctype == 3 ? 768 : 0);
        if (padded > staging_bytes) return FPC_EWORKSPACE;
        memset(staging + o, 0, align16(o) - o);
        if (h.ctype == 3) memcpy(staging + align16(o), palette, 768);
        o = padded;
        int64_t* q = desc + (size_t)i * kDescWords;
        q[0] = (int64_t)start; q[1] = (int64_t)zbytes; q[2] = h.w; q[3] = h.h; q[4] = h.depth; q[5] = h.ctype; q[6] = h.channels;
        q[7] = pn;
    }
    *used = o;
    return FPC_OK;
}

extern "C" size_t fpc_png_decode_device_workspace_bytes(int n, int H, int W, int max_bpp) {
    if (n < 1 || H < 1 || W < 1 || max_bpp < 1 || max_bpp > 8) return 0;
    return (size_t)n * align16((size_t)H * (1 + (size_t)W * max_bpp));
}

extern "C" int fpc_png_decode_device(const uint8_t* staging, size_t staging_bytes, const int64_t* desc, int n, int H, int W,
                                     int mode, int max_bpp, void* out, size_t frame_bytes, int32_t* status, void* workspace,
                                     size_t workspace_bytes, fpc_stream_t stream) {
    if (!staging || !desc || !out || !status || !workspace) return FPC_EINVAL;
    if (n < 1 || H < 1 || W < 1 || H > 65535 || W > 65535 || (mode != 0 && mode != 3) || max_bpp < 1 || max_bpp > 8) return FPC_EINVAL;
    if (((uintptr_t)staging & 15) || ((uintptr_t)desc & 7) || ((uintptr_t)out & 15) || ((uintptr_t)status & 3) ||
        ((uintptr_t)workspace & 15))
        return FPC_EINVAL;
    if ((size_t)W * max_bpp > (size_t)kMaxStride) return FPC_EINVAL;
    const size_t raw_slice = align16((size_t)H * (1 + (size_t)W * max_bpp));
    if (staging_bytes >= kLimit || raw_slice >= kLimit / (size_t)n || frame_bytes >= kLimit / (size_t)n) return FPC_EINVAL;
    if (mode == 3 && frame_bytes < (size_t)H * W * 3) return FPC_EINVAL;
    if (workspace_bytes < (size_t)n * raw_slice) return FPC_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    k_png_inflate<<<n, 64, 0, s>>>(staging, staging_bytes, desc, H, W, mode, max_bpp, frame_bytes, (uint8_t*)workspace, raw_slice,
                                   status);
    k_png_unfilter<<<n, 64, 0, s>>>(staging, staging_bytes, desc, H, W, mode, max_bpp, (uint8_t*)out, frame_bytes,
                                    (const uint8_t*)workspace, raw_slice, status);
    return fpc::check_launch();
}
