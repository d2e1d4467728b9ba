// conv_igemm.hip — the implicit-GEMM convolution of the backbone engine, its split-K epilogue and its weight packers.
//
//   k_conv_igemm        implicit-GEMM convolution on the f32 matrix cores
//                       (v_mfma_f32_32x32x2_f32: exact f32 FMA chains, no reduced precision).
//                       M = output pixels of one image, N = output channels, K = (kh, kw, ci).
//                       Activations are NHWC so a K-step of 32 channels is one 128-byte row per
//                       output pixel; weights are pre-packed OHWI [Npad][Kpad].  256 threads =
//                       2x2 wave64, each wave owns a (BM/2)x(BN/2) block of 32x32 MFMA tiles.
//                       Global -> registers -> LDS (double buffered, rows padded to 36 floats:
//                       conflict-free ds_read_b128 fragments), one barrier per K-step; the next
//                       K-step's global loads are in flight under the current step's MFMAs.
//                       Epilogue: folded BatchNorm / bias, residual, FPN nearest-x2 add, ReLU,
//                       GroupNorm partial sums.  Split-K writes raw partials instead.
//                       Split forms (MODE 0): BF3, three bf16 planes per operand and six products per 16-deep k group
//                       (fpc_conv2d's 1000 + split); H3, two fp16 planes and three products (6000 + split, 6100 + split with
//                       the second-launch split-K sum) on k_pack_weight_h3's power-of-two-scaled weights — activations keep
//                       3 * 2^-23 relative for 2^-2 <= |x| < 2^16, 2^-24 absolute below, lose precision above (2^-12 of the
//                       value at 131 008) and saturate (finite) beyond 131 008 (common.hpp: split_h2).
//   k_conv_splitk_epilogue  fixed-order sum of the split-K partials + the same epilogue.
//   k_pack_weight, k_pack_weight_bf3, k_pack_weight_h3: OIHW weights -> the kernel's [Npad][Kpad] images (once per plan).
#include "conv_device.hpp"

namespace fpc {

// ------------------------------------------------------------------------------------------
// implicit-GEMM convolution
// (FPC_IGEMM_DMA_B: net_kernels.hpp — fpc_conv2d's packing depends on it)
#ifndef FPC_IGEMM_PRIO
#define FPC_IGEMM_PRIO 1
#endif
#ifndef FPC_IGEMM_INTERLEAVE
#define FPC_IGEMM_INTERLEAVE 1
#endif

// One K-step of operands, global -> registers.  Thread (sr, sq) owns rows sr + 32*i and the float4 at
// column 4*sq of the 32-wide K-step.  (Macros, not functions: hipcc keeps by-reference register
// arrays in scratch.)
//
// Every load is a buffer_load (descriptor + 32-bit lane offset + scalar offset): beside a SIMD partner that
// issues MFMAs back to back a global_load with a 64-bit VGPR address waits like a vector-ALU instruction — one
// slot per MFMA, starved by a pure MFMA loop — while the buffer form issues in 9 cycles
// (tools_dev/dma_vs_mfma.hip).  MODE 0 (Cin % 32 == 0: a K-step is 32 channels of ONE tap) keeps the whole
// address generation on the scalar unit: per row a constant lane offset and an inverted validity mask over the
// taps (bit t = 1: tap t of this row is padding), so the zero fill is  offset | ((mask >> tap) << 31)  — two
// vector instructions per row and K-step; the tap walk (c0, kw, kh) advances with scalar compares.  MODE 0
// loads must be issued in K-step order (they are: ks0, ks0+1, ...).
#define FPC_CONV_LOAD(KS, ra, rb)                                                                                     \
    do {                                                                                                      \
        const int ks_ = (KS);                                                                                 \
        if (!DMAB) { _Pragma("unroll") for (int i = 0; i < BR; ++i) rb[i] = buf_load4(rs_w, wvo[i], ks_ * (kConvBK * 4)); } \
        if (MODE == 0) {                                                                                      \
            _Pragma("unroll") for (int i = 0; i < AR; ++i)                                                    \
                ra[i] = buf_load4(rs_in, ((anm[i] >> ld_tap) << 31) | avo[i], ld_soff);                       \
            ld_c0 += kConvBK; ld_soff += kConvBK * 4;                                                         \
            if (ld_c0 >= Cin) {                                                                               \
                ld_c0 = 0; ++ld_tap; ++ld_kw;                                                                 \
                if (ld_kw == Kw) { ld_kw = 0; ++ld_kh; }                                                      \
                ld_soff = (ld_kh * ish + ld_kw * isw) * 4;                                                    \
            }                                                                                                 \
        } else if (MODE == 2) {                                                                               \
            /* Cin % 4 == 0, channel-last: this lane's float4 is 4 channels of ONE tap (the 7x7 stem on */   \
            /* the NHWC4 image: 8 taps per K-step)                                                       */   \
            int kq = ks_ * kConvBK + 4 * sq;                                                                  \
            bool kv = kq < K;                                                                                 \
            int tap = kq / Cin, c0 = kq - tap * Cin;                                                          \
            int kh = tap / Kw, kw = tap - kh * Kw;                                                            \
            long long koff = (long long)kh * in_sh + (long long)kw * in_sw + c0;                              \
            _Pragma("unroll") for (int i = 0; i < AR; ++i) {                                                  \
                int hi = a_hi0[i] + kh, wi = a_wi0[i] + kw;                                                   \
                bool ok = kv && hi >= 0 && hi < Hi && wi >= 0 && wi < Wi;                                     \
                ra[i] = ok ? *reinterpret_cast<const f32x4*>(P.in + a_off[i] + koff)                          \
                           : f32x4{0.f, 0.f, 0.f, 0.f};                                                       \
            }                                                                                                 \
        } else {                                                                                              \
            /* any Cin / any input strides */                                                                 \
            _Pragma("unroll") for (int i = 0; i < AR; ++i) ra[i] = f32x4{0.f, 0.f, 0.f, 0.f};           \
            _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                                   \
                int k = ks_ * kConvBK + 4 * sq + e;                                                           \
                bool kv = k < K;                                                                              \
                int tap = k / Cin, ci = k - tap * Cin;                                                        \
                int kh = tap / Kw, kw = tap - kh * Kw;                                                        \
                long long koff = (long long)kh * in_sh + (long long)kw * in_sw + (long long)ci * in_sc;       \
                _Pragma("unroll") for (int i = 0; i < AR; ++i) {                                              \
                    int hi = a_hi0[i] + kh, wi = a_wi0[i] + kw;                                               \
                    bool ok = kv && hi >= 0 && hi < Hi && wi >= 0 && wi < Wi;                                 \
                    float v = ok ? P.in[a_off[i] + koff] : 0.f;                                               \
                    if (e == 0) ra[i].x = v;                                                                  \
                    if (e == 1) ra[i].y = v;                                                                  \
                    if (e == 2) ra[i].z = v;                                                                  \
                    if (e == 3) ra[i].w = v;                                                                  \
                }                                                                                             \
            }                                                                                                 \
        }                                                                                                     \
    } while (0)

#define FPC_CONV_STORE(BUF, ra, rb)                                                                           \
    do {                                                                                                      \
        float* As_ = lds + (BUF) * (BM + BN) * kLdsRow;                                                       \
        float* Bs_ = As_ + BM * kLdsRow;                                                                      \
        _Pragma("unroll") for (int i = 0; i < AR; ++i)                                                        \
            *reinterpret_cast<f32x4*>(As_ + (sr + 32 * i) * kLdsRow + swz_w) = ra[i];                        \
        _Pragma("unroll") for (int i = 0; i < BR; ++i)                                                        \
            *reinterpret_cast<f32x4*>(Bs_ + (sr + 32 * i) * kLdsRow + swz_w) = rb[i];                        \
    } while (0)

// Split-precision staging: three bf16 planes per operand in LDS.  Plane rows are 32 bf16 = 64 bytes = four 16-byte chunks
// (one MFMA operand each); chunk c of row r sits in slot c ^ ((r >> 2) & 1) so that the eight rows a ds_read_b128 group
// touches hit eight different 16-byte positions of the bank window.  The ACTIVATION rows are split here, on the way from
// the f32 registers of one K-step; the WEIGHT rows arrive already split (k_pack_weight_bf3: three bf16 planes behind the
// f32 image) and go global -> LDS by LDS-DMA, FPC_CONV_DMA_B — no registers, no vector instructions, no ds_write.
#define FPC_CONV_STORE_BF3(BUF, ra, rb)                                                                       \
    do {                                                                                                      \
        char* st_ = reinterpret_cast<char*>(lds) + (BUF) * (BM + BN) * 192;                                   \
        _Pragma("unroll") for (int i = 0; i < AR + (DMAB ? 0 : BR); ++i) {                                    \
            const int row_ = (i < AR ? 0 : BM) + sr + 32 * (i < AR ? i : i - AR);                             \
            u32x2 p1_, p2_, p3_;                                                                              \
            split_bf3(i < AR ? ra[i < AR ? i : 0] : rb[i < AR ? 0 : i - AR], p1_, p2_, p3_);                  \
            char* d_ = st_ + row_ * 64 + bf3_w;                                                               \
            *reinterpret_cast<u32x2*>(d_) = p1_;                                                              \
            *reinterpret_cast<u32x2*>(d_ + (BM + BN) * 64) = p2_;                                             \
            *reinterpret_cast<u32x2*>(d_ + 2 * (BM + BN) * 64) = p3_;                                         \
        }                                                                                                     \
    } while (0)

// Epilogue of one lane's 4 rows (p0 + 8k) x 4 channels (n .. n+3) of a 32-row tile: folded BatchNorm / bias, residual,
// FPN nearest-x2 add, ReLU, store, and the GroupNorm partial sums of the tile's 32 rows per channel.
struct EpiGeom { int b, HoWo, Wo, Cout, Hu, Wu, P32, relu, lane; };
// The epilogue's own global reads of one lane's 4 rows x 4 channels (Cout % 4 == 0): scale / shift, residual, top-down addend.
// k_conv_igemm requests them BEFORE a tile's LDS transpose (round 5): issued inside conv_epilogue they sat behind the transpose's
// s_waitcnt (a memory clobber the compiler cannot move loads across), one exposed L2 round trip per 32 x 32 tile.  Absent
// operands come back as 1 / 0, so the epilogue uses them unconditionally.
struct EpiPre { f32x4 sc, sh, res[4], up[4]; };
__device__ __forceinline__ void conv_epilogue_prefetch(EpiPre& e, const ConvPtrs& P, const EpiGeom& g, int p0, int n) {
    e.sc = f32x4{1.f, 1.f, 1.f, 1.f}; e.sh = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k) { e.res[k] = f32x4{0.f, 0.f, 0.f, 0.f}; e.up[k] = e.res[k]; }
    if ((g.Cout & 3) != 0 || n >= g.Cout) return;
    if (P.scale) e.sc = *reinterpret_cast<const f32x4*>(P.scale + n);
    if (P.shift) e.sh = *reinterpret_cast<const f32x4*>(P.shift + n);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int p = p0 + 8 * k;
        if (p >= g.HoWo) continue;
        if (P.res) e.res[k] = *reinterpret_cast<const f32x4*>(P.res + ((size_t)g.b * g.HoWo + p) * g.Cout + n);
        if (P.up) {
            const int ho = p / g.Wo, wo = p - ho * g.Wo;
            e.up[k] = *reinterpret_cast<const f32x4*>(P.up + (((size_t)g.b * g.Hu + (ho >> 1)) * g.Wu + (wo >> 1)) * g.Cout + n);
        }
    }
}
__device__ __forceinline__ void conv_epilogue(const ConvPtrs& P, const EpiGeom& g, f32x4 v0, f32x4 v1, f32x4 v2, f32x4 v3, int p0, int n,
                                              const EpiPre& pre) {
    const int b = g.b, HoWo = g.HoWo, Wo = g.Wo, Cout = g.Cout, Hu = g.Hu, Wu = g.Wu;
    const f32x4 v[4] = {v0, v1, v2, v3};
    f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
    if ((Cout & 3) == 0) {
        const bool nv = n < Cout;
        const f32x4 sc = pre.sc, sh = pre.sh;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int p = p0 + 8 * k;
            if (!(nv && p < HoWo)) continue;
            f32x4 x = v[k];
            if (P.scale) x = x * sc;
            x = x + sh;
            size_t o = ((size_t)b * HoWo + p) * Cout + n;
            if (P.res) x += pre.res[k];
            if (P.up) x += pre.up[k];
            if (g.relu) { x[0] = fmaxf(x[0], 0.f); x[1] = fmaxf(x[1], 0.f); x[2] = fmaxf(x[2], 0.f); x[3] = fmaxf(x[3], 0.f); }
            *reinterpret_cast<f32x4*>(P.out + o) = x;
            s1 += x;
            s2 += x * x;
        }
    } else {                                           // any Cout: scalar accesses
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int p = p0 + 8 * k;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                int ne = n + e;
                if (!(ne < Cout && p < HoWo)) continue;
                float x = v[k][e];
                if (P.scale) x = x * P.scale[ne];
                if (P.shift) x = x + P.shift[ne];
                size_t o = ((size_t)b * HoWo + p) * Cout + ne;
                if (P.res) x += P.res[o];
                if (P.up) {
                    int ho = p / Wo, wo = p - ho * Wo;
                    x += P.up[(((size_t)b * Hu + (ho >> 1)) * Wu + (wo >> 1)) * Cout + ne];
                }
                if (g.relu) x = fmaxf(x, 0.f);
                P.out[o] = x;
                s1[e] += x;
                s2[e] += x * x;
            }
        }
    }
    if (P.gn_part) {
        // column sums over the tile's 32 rows: lanes with equal (lane & 7) hold the same channels
#pragma unroll
        for (int o = 8; o < 64; o <<= 1) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                s1[e] += __shfl_xor(s1[e], o, 64);
                s2[e] += __shfl_xor(s2[e], o, 64);
            }
        }
        if (g.lane < 8) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (n + e < Cout) {
                    float* gp = P.gn_part + (((size_t)b * g.P32 + p0 / 32) * Cout + n + e) * 2;
                    gp[0] = s1[e]; gp[1] = s2[e];
                }
        }
    }
}

// (the 128x128 tiling keeps 64 accumulator + 64 staging registers per lane: one workgroup per CU, no spills)
// H3 (ConvArgs::h3): the three-product form on two fp16 pieces per operand (split_h2; weights: k_pack_weight_h3's planes)
template <int BM, int BN, int MODE, bool BF3 = false, bool H3 = false>
__global__ __launch_bounds__(256, (BM * BN >= 128 * 128) ? 1 : 2) void k_conv_igemm(const ConvArgs a) {
    constexpr int TM = BM / 64, TN = BN / 64;     // 32x32 tiles per wave
    constexpr int AR = BM / 32, BR = BN / 32;     // float4 rows staged per thread
    constexpr bool SPL = BF3 || H3;               // split operands in LDS planes
    constexpr int NPL = H3 ? 2 : 3;               // planes per operand
    constexpr int kPlB = NPL * 64;                // bytes of one operand row over its planes (one stage)
    constexpr bool DMAB = SPL && FPC_IGEMM_DMA_B; // split precision: weight planes pre-split, staged by LDS-DMA
    // f32 operands: 2 stages x (BM + BN) rows x 128 B;  split precision: 2 stages x NPL planes x (BM + BN) rows x 64 B
    __shared__ __attribute__((aligned(16))) float lds[SPL ? 2 * (BM + BN) * (NPL * 16) : 2 * (BM + BN) * kLdsRow];
    __shared__ int s_last;
    static_assert(!SPL || MODE == 0, "split precision rides on the fast loader");
    static_assert(!(BF3 && H3) && (!H3 || DMAB), "one product form; H3 weights come by LDS-DMA only");
#ifdef FPC_STAMP_IGEMM      // diagnostic build (tools_dev/igemm_stamps.py): phase stamps per wave into a.dbg
    const long long st0 = clock64();
#endif

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int li = lane & 31, lh = lane >> 5;
    const int Cin = a.Cin, Kw = a.Kw, K = a.K, Hi = a.Hi, Wi = a.Wi, Wo = a.Wo, Cout = a.Cout, Npad = a.Npad;
    const int Kpad = a.Kpad, stride = a.stride, pad = a.pad, mtiles = a.mtiles, ntiles = a.ntiles, nB = a.B;
    const int nsplit = a.nsplit, ksteps = a.ksteps;
    const long long in_sb = a.in_sb, in_sh = a.in_sh, in_sw = a.in_sw, in_sc = a.in_sc;

    // Block order: the WEIGHT SLICE (group, n tile, k split) varies fastest, then the m tile.  Workgroups
    // are dealt round-robin over the 8 XCDs, so blockIdx % 8 — hence the weight slice, whenever the slice
    // count is 1, 2, 4 or a multiple of 8 — is fixed per XCD: an XCD's private L2 then holds ~1 MB of
    // weights that every one of its workgroups re-reads, instead of all slices thrashing all L2s
    // (measured before: 45-55 % L2 misses, ~5 TB/s of fabric reads for 85 MB of unique operands).
    int bid = blockIdx.x;
    const int sp = bid % nsplit; bid /= nsplit;
    const int nt = bid % ntiles; bid /= ntiles;
    const int grp = bid % a.groups; bid /= a.groups;
    const int mt = bid % mtiles;
    const int b = bid / mtiles;
    ConvPtrs P = a.p[0];
    if (grp == 1) P = a.p[1];
    if (grp == 2) P = a.p[2];
    if (grp == 3) P = a.p[3];
    const int HoWo = a.Ho * Wo;
    const int m0 = mt * BM, n0 = nt * BN;
    int ks0 = 0, ks1 = ksteps;
    if (nsplit > 1) {
        int per = (ksteps + nsplit - 1) / nsplit;
        ks0 = sp * per;
        ks1 = min(ksteps, ks0 + per);
    }

    const int sr = t >> 3, sq = t & 7;
    // swizzled 16-byte slot (in floats) of this thread's staging writes, and of its fragment reads per k-group:
    // lanes 0-31 carry k = kk*8 + e (chunk 2kk), lanes 32-63 k = kk*8 + 4 + e (chunk 2kk + 1); rows sr + 32i / li + 32i
    const int swz_w = 4 * (sq ^ (sr & 7));
    // split precision: byte offset inside a 64-byte plane row of this thread's four k (write) and of this lane's
    // eight k per 16-deep MFMA (read): chunk = k / 8, slot = chunk ^ ((row >> 2) & 1); rows sr + 32i / li + 32i
    const int bf3_w = (((sq >> 1) ^ ((sr >> 2) & 1)) << 4) + ((sq & 1) << 3);
    const int bf3_r[2] = {((0 + lh) ^ ((li >> 2) & 1)) << 4, ((2 + lh) ^ ((li >> 2) & 1)) << 4};
    const int swz_r[4] = {4 * ((0 + lh) ^ (li & 7)), 4 * ((2 + lh) ^ (li & 7)), 4 * ((4 + lh) ^ (li & 7)), 4 * ((6 + lh) ^ (li & 7))};
    long long a_off[AR];     // MODE 1, 2: element offset of (b, hi0, wi0, 0)
    int a_hi0[AR], a_wi0[AR];
    unsigned avo[AR], anm[AR];   // MODE 0: byte offset of (ho*stride, wo*stride, 4*sq) from the shifted base; padding mask
    const int ish = (int)in_sh, isw = (int)in_sw;
#pragma unroll
    for (int i = 0; i < AR; ++i) {
        int p = m0 + sr + 32 * i;
        bool ok = p < HoWo;
        int ho = ok ? p / Wo : 0, wo = ok ? p - ho * Wo : 0;
        a_hi0[i] = ok ? ho * stride - pad : -0x40000000;   // rows past the image: always out of bounds
        a_wi0[i] = wo * stride - pad;
        a_off[i] = (long long)b * in_sb + (long long)a_hi0[i] * in_sh + (long long)a_wi0[i] * in_sw;
        if (MODE == 0) {
            avo[i] = (unsigned)((ho * stride * ish + wo * stride * isw + 4 * sq) * 4);
            unsigned vw = 0, m = 0;                        // valid columns (bit kw), valid taps (bit kh*Kw + kw)
            const int lpx = a.lanepx ? sq : 0;             // lane-pixel layout: this lane's 16 bytes are pixel wi0 + sq
            for (int kw = 0; kw < Kw; ++kw) vw |= (unsigned)(a_wi0[i] + kw + lpx >= 0 && a_wi0[i] + kw + lpx < Wi) << kw;
            for (int kh = 0; kh < a.Kh; ++kh)
                if (ok && a_hi0[i] + kh >= 0 && a_hi0[i] + kh < Hi) m |= vw << (kh * Kw);
            anm[i] = ~m;
        }
    }
    // MODE 0: the descriptor starts `pad` rows and columns before the image (valid taps never reach below P.in)
    const __amdgpu_buffer_rsrc_t rs_in = make_rsrc(P.in + (long long)b * in_sb - ((long long)pad * in_sh + (long long)pad * in_sw));
    const __amdgpu_buffer_rsrc_t rs_w = make_rsrc(P.w);
    unsigned wvo[BR];
#pragma unroll
    for (int i = 0; i < BR; ++i) wvo[i] = (unsigned)(((n0 + sr + 32 * i) * Kpad + 4 * sq) * 4);
    // split precision: this wave's LDS-DMA pieces of a K-step's weight planes.  A piece = 16 rows x 64 B of one plane (1 KB,
    // lane l -> row l >> 2, slot l & 3); 3 * BN / 16 pieces per K-step, piece q = wave + 4 i is plane q / (BN / 16), row
    // group q % (BN / 16).  The swizzle is the choice of the chunk each lane fetches.  SGPR base + 32-bit lane offset, the
    // base advances 64 B per K-step (see the Winograd kernel for why not a 64-bit lane address).
    // (H3: the two fp16 planes start at P.w and 1 / s follows them)
    constexpr int kRG = BN / 16, kNPB = NPL * kRG / 4;
    const int swave = __builtin_amdgcn_readfirstlane(wave);
    unsigned bvo[kNPB];
    const char* w3b = nullptr;
    if constexpr (DMAB) {
#pragma unroll
        for (int i = 0; i < kNPB; ++i) {
            const int q = swave + 4 * i, pl = q / kRG, rg = q - pl * kRG;
            const int r = rg * 16 + (lane >> 2), c = (lane & 3) ^ ((r >> 2) & 1);
            bvo[i] = (unsigned)((((size_t)pl * Npad + n0 + r) * Kpad + c * 8) * 2);
        }
        w3b = reinterpret_cast<const char*>(P.w + (H3 ? 0 : (size_t)Npad * Kpad)) + (size_t)ks0 * (kConvBK * 2);
    }
    const float h3_inv = H3 ? P.w[(size_t)Npad * Kpad] : 1.f;
    float m1 = -1.f;
    if constexpr (H3) asm volatile("s_mov_b32 %0, 0xbf800000" : "=s"(m1));      // -1.0f, opaque: x - h1 as one v_fma_mix_f32
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
#define FPC_CONV_DMA_B(BUF)                                                                                   \
    do {                                                                                                      \
        _Pragma("unroll") for (int i = 0; i < kNPB; ++i) {                                                    \
            const int q_ = swave + 4 * i, pl_ = q_ / kRG, rg_ = q_ - pl_ * kRG;                               \
            asm volatile("s_mov_b32 m0, %0\n s_nop 0\n global_load_lds_dwordx4 %1, %2\n"                      \
                         :: "s"((unsigned)(size_t)(__attribute__((address_space(3))) void*)(reinterpret_cast<char*>(lds) + \
                                 (BUF) * (BM + BN) * kPlB + pl_ * (BM + BN) * 64 + (BM + rg_ * 16) * 64)),      \
                            "v"(bvo[i]), "s"(w3b) : "memory", "m0");                                          \
        }                                                                                                     \
        w3b += kConvBK * 2;                                                                                   \
    } while (0)
    // the pieces above have landed; the NYOUNG vector-memory operations issued after them may stay in flight
#define FPC_CONV_DMA_WAIT(YOUNGER)                                                                            \
    do {                                                                                                      \
        if (YOUNGER) { if constexpr (AR == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); } \
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                 \
    } while (0)
    static_assert(AR == 2 || AR == 4, "FPC_CONV_DMA_WAIT counts AR activation loads");
    // tap walk of the NEXT K-step to load (scalar): channel offset, tap index and coordinates, byte offset of the tap
    int ld_c0, ld_tap, ld_kh, ld_kw, ld_soff;
    {
        int k0 = ks0 * kConvBK;
        ld_tap = k0 / Cin; ld_c0 = k0 - ld_tap * Cin;
        ld_kh = ld_tap / Kw; ld_kw = ld_tap - ld_kh * Kw;
        ld_soff = (ld_kh * ish + ld_kw * isw + ld_c0) * 4;
    }

    // two register sets: the loads of K-step k+2 are issued while step k is computed and step k+1
    // waits in registers, so every global load has two compute phases to land (HBM / L2 latency
    // under load exceeds one phase of 16..64 MFMAs)
    f32x4 ra0[AR], rb0[BR], ra1[AR], rb1[BR];
    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // Fragments of the next 8-deep k group are read from LDS BEFORE the current group's MFMAs are issued
    // (sched_barrier keeps hipcc from sinking the reads to their first use): the ~128-cycle LDS latency
    // is then hidden behind 8..32 MFMAs instead of stalling the wave four times per K-step.
#define FPC_CONV_FRAG(KK, FA, FB)                                                                             \
    do {                                                                                                      \
        _Pragma("unroll") for (int i = 0; i < TM; ++i) FA[i] =                                                \
            *reinterpret_cast<const f32x4*>(As + i * 32 * kLdsRow + swz_r[KK]);                               \
        _Pragma("unroll") for (int j = 0; j < TN; ++j) FB[j] =                                                \
            *reinterpret_cast<const f32x4*>(Bs + j * 32 * kLdsRow + swz_r[KK]);                               \
    } while (0)
    /* lanes 0-31 carry k = kk*8 + e, lanes 32-63 carry k = kk*8 + 4 + e: each MFMA sums two k */
#define FPC_CONV_MFMA(FA, FB)                                                                                 \
    do {                                                                                                      \
        _Pragma("unroll") for (int e = 0; e < 4; ++e)                                                         \
            _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                    \
                _Pragma("unroll") for (int j = 0; j < TN; ++j)                                                \
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(FA[i][e], FB[j][e], acc[i][j], 0, 0, 0); \
    } while (0)
#define FPC_CONV_COMPUTE(BUF)                                                                                  \
    do {                                                                                                      \
        const float* As = lds + (BUF) * (BM + BN) * kLdsRow + (wm * (BM / 2) + li) * kLdsRow;                 \
        const float* Bs = lds + (BUF) * (BM + BN) * kLdsRow + BM * kLdsRow + (wn * (BN / 2) + li) * kLdsRow;  \
        f32x4 fa0[TM], fb0[TN], fa1[TM], fb1[TN];                                                             \
        FPC_CONV_FRAG(0, fa0, fb0);                                                                           \
        FPC_CONV_FRAG(1, fa1, fb1);                                                                           \
        __builtin_amdgcn_sched_barrier(0);                                                                    \
        __builtin_amdgcn_s_setprio(1);                                                                        \
        FPC_CONV_MFMA(fa0, fb0);                                                                              \
        __builtin_amdgcn_sched_barrier(0);                                                                    \
        FPC_CONV_FRAG(2, fa0, fb0);                                                                           \
        __builtin_amdgcn_sched_barrier(0);                                                                    \
        FPC_CONV_MFMA(fa1, fb1);                                                                              \
        __builtin_amdgcn_sched_barrier(0);                                                                    \
        FPC_CONV_FRAG(3, fa1, fb1);                                                                           \
        __builtin_amdgcn_sched_barrier(0);                                                                    \
        FPC_CONV_MFMA(fa0, fb0);                                                                              \
        FPC_CONV_MFMA(fa1, fb1);                                                                              \
        __builtin_amdgcn_s_setprio(0);                                                                        \
    } while (0)

    // split precision: per 16-deep k group three planes per operand, six MFMAs per 32x32 tile
#define FPC_BF3_FRAG(KK, FA, FB)                                                                              \
    do {                                                                                                      \
        _Pragma("unroll") for (int p_ = 0; p_ < 3; ++p_) {                                                    \
            _Pragma("unroll") for (int i = 0; i < TM; ++i) FA[p_][i] = __builtin_bit_cast(bf16x8,             \
                *reinterpret_cast<const u32x4*>(Ab + p_ * (BM + BN) * 64 + i * 32 * 64 + bf3_r[KK]));         \
            _Pragma("unroll") for (int j = 0; j < TN; ++j) FB[p_][j] = __builtin_bit_cast(bf16x8,             \
                *reinterpret_cast<const u32x4*>(Bb + p_ * (BM + BN) * 64 + j * 32 * 64 + bf3_r[KK]));         \
        }                                                                                                     \
    } while (0)
#define FPC_BF3_MFMA(FA, FB)                                                                                  \
    do {                                                                                                      \
        _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                        \
            _Pragma("unroll") for (int j = 0; j < TN; ++j) {                                                  \
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(FA[2][i], FB[0][j], acc[i][j], 0, 0, 0);  \
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(FA[0][i], FB[2][j], acc[i][j], 0, 0, 0);  \
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(FA[1][i], FB[1][j], acc[i][j], 0, 0, 0);  \
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(FA[1][i], FB[0][j], acc[i][j], 0, 0, 0);  \
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(FA[0][i], FB[1][j], acc[i][j], 0, 0, 0);  \
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(FA[0][i], FB[0][j], acc[i][j], 0, 0, 0);  \
            }                                                                                                 \
    } while (0)
#define FPC_CONV_COMPUTE_BF3(BUF)                                                                             \
    do {                                                                                                      \
        const char* Ab = reinterpret_cast<const char*>(lds) + (BUF) * (BM + BN) * 192 + (wm * (BM / 2) + li) * 64;        \
        const char* Bb = reinterpret_cast<const char*>(lds) + (BUF) * (BM + BN) * 192 + (BM + wn * (BN / 2) + li) * 64;   \
        bf16x8 ga0[3][TM], gb0[3][TN], ga1[3][TM], gb1[3][TN];                                                \
        FPC_BF3_FRAG(0, ga0, gb0);                                                                            \
        FPC_BF3_FRAG(1, ga1, gb1);                                                                            \
        __builtin_amdgcn_sched_barrier(0);                                                                    \
        __builtin_amdgcn_s_setprio(FPC_IGEMM_PRIO);                                                                        \
        FPC_BF3_MFMA(ga0, gb0);                                                                               \
        FPC_BF3_MFMA(ga1, gb1);                                                                               \
        __builtin_amdgcn_s_setprio(0);                                                                        \
    } while (0)
    // Split precision with DMA-staged weights: the matrix block of LDS buffer BUF with the split of the NEXT step's
    // activation registers (ra -> the three planes of buffer BUF ^ 1) cut into 6 micro-steps per row — and, and-subtract,
    // and, subtract, pack, three 8-byte LDS stores — that are issued one after each MFMA (or every second one), in the matrix
    // instructions' shadow instead of as a block of 44 vector instructions + 6 ds_write_b64 behind them.  Runs unconditionally:
    // past the last step it splits stale registers into a buffer nobody reads (the epilogue's patches come after a barrier).
    // Not for the 128 x 128 tile: fully unrolled there the block needs more than 512 registers.
#define FPC_CONV_COMPUTE_STORE_BF3(BUF, ra)                                                                   \
    do {                                                                                                      \
        const char* Ab = reinterpret_cast<const char*>(lds) + (BUF) * (BM + BN) * 192 + (wm * (BM / 2) + li) * 64;        \
        const char* Bb = reinterpret_cast<const char*>(lds) + (BUF) * (BM + BN) * 192 + (BM + wn * (BN / 2) + li) * 64;   \
        char* st_ = reinterpret_cast<char*>(lds) + ((BUF) ^ 1) * (BM + BN) * 192;                             \
        bf16x8 ga[2][3][TM], gb[2][3][TN];                                                                    \
        FPC_BF3_FRAG(0, ga[0], gb[0]);                                                                        \
        FPC_BF3_FRAG(1, ga[1], gb[1]);                                                                        \
        __builtin_amdgcn_sched_barrier(0);                                                                    \
        __builtin_amdgcn_s_setprio(FPC_IGEMM_PRIO);                                                                        \
        constexpr int kNM = 12 * TM * TN, kNS = 6 * AR;      /* MFMAs, split micro-steps */                    \
        constexpr int kPa[6] = {2, 0, 1, 1, 0, 0}, kPb[6] = {0, 2, 1, 0, 1, 0};                               \
        unsigned sb1_[AR][4], sb2_[AR][4];                                                                    \
        float sr_[AR][4], sq_[AR][4];                                                                         \
        u32x2 sp1_[AR], sp2_[AR], sp3_[AR];                                                                   \
        _Pragma("unroll") for (int m_ = 0; m_ < kNM; ++m_) {                                                  \
            const int kk_ = m_ / (6 * TM * TN), t_ = (m_ / 6) % (TM * TN), c_ = m_ % 6;                       \
            const int i_ = t_ / TN, j_ = t_ % TN;                                                             \
            acc[i_][j_] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ga[kk_][kPa[c_]][i_], gb[kk_][kPb[c_]][j_], acc[i_][j_], 0, 0, 0); \
            _Pragma("unroll") for (int ns_ = m_ * kNS / kNM; ns_ < (m_ + 1) * kNS / kNM; ++ns_) {             \
                const int r_ = ns_ / 6, ph_ = ns_ % 6;                                                        \
                if (ph_ == 0) { _Pragma("unroll") for (int e = 0; e < 4; ++e) { const float x_ = ra[r_][e]; sb1_[r_][e] = __builtin_bit_cast(unsigned, x_) & 0xFFFF0000u; } } \
                if (ph_ == 1) { _Pragma("unroll") for (int e = 0; e < 4; ++e) { const float x_ = ra[r_][e]; sr_[r_][e] = x_ - __builtin_bit_cast(float, sb1_[r_][e]); } } \
                if (ph_ == 2) { _Pragma("unroll") for (int e = 0; e < 4; ++e) sb2_[r_][e] = __builtin_bit_cast(unsigned, sr_[r_][e]) & 0xFFFF0000u; } \
                if (ph_ == 3) { _Pragma("unroll") for (int e = 0; e < 4; ++e) sq_[r_][e] = sr_[r_][e] - __builtin_bit_cast(float, sb2_[r_][e]); } \
                if (ph_ == 4) {                                                                               \
                    const float x0_ = ra[r_][0], x1_ = ra[r_][1], x2_ = ra[r_][2], x3_ = ra[r_][3];           \
                    sp1_[r_] = u32x2{pack_hi16(x0_, x1_), pack_hi16(x2_, x3_)};                               \
                    sp2_[r_] = u32x2{pack_hi16(sr_[r_][0], sr_[r_][1]), pack_hi16(sr_[r_][2], sr_[r_][3])};   \
                    sp3_[r_] = u32x2{pack_hi16(sq_[r_][0], sq_[r_][1]), pack_hi16(sq_[r_][2], sq_[r_][3])};   \
                }                                                                                             \
                if (ph_ == 5) {                                                                               \
                    char* d_ = st_ + (sr + 32 * r_) * 64 + bf3_w;                                             \
                    *reinterpret_cast<u32x2*>(d_) = sp1_[r_];                                                 \
                    *reinterpret_cast<u32x2*>(d_ + (BM + BN) * 64) = sp2_[r_];                                \
                    *reinterpret_cast<u32x2*>(d_ + 2 * (BM + BN) * 64) = sp3_[r_];                            \
                }                                                                                             \
            }                                                                                                 \
            __builtin_amdgcn_sched_barrier(0);                                                                \
        }                                                                                                     \
        __builtin_amdgcn_s_setprio(0);                                                                        \
    } while (0)
    // Three-product form (H3): per 16-deep k group two fp16 planes per operand, acc += A2 B1 + A1 B2 + A1 B1 — three MFMAs per
    // 32x32 tile instead of six.  The activation rows are split on the way into LDS (split_h2), the weight planes come by LDS-DMA.
#define FPC_H3_FRAG(KK, FA, FB)                                                                               \
    do {                                                                                                      \
        _Pragma("unroll") for (int p_ = 0; p_ < 2; ++p_) {                                                    \
            _Pragma("unroll") for (int i = 0; i < TM; ++i) FA[p_][i] = __builtin_bit_cast(f16x8,              \
                *reinterpret_cast<const u32x4*>(Ab + p_ * (BM + BN) * 64 + i * 32 * 64 + bf3_r[KK]));         \
            _Pragma("unroll") for (int j = 0; j < TN; ++j) FB[p_][j] = __builtin_bit_cast(f16x8,              \
                *reinterpret_cast<const u32x4*>(Bb + p_ * (BM + BN) * 64 + j * 32 * 64 + bf3_r[KK]));         \
        }                                                                                                     \
    } while (0)
#define FPC_H3_MFMA(FA, FB)                                                                                   \
    do {                                                                                                      \
        _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                        \
            _Pragma("unroll") for (int j = 0; j < TN; ++j) {                                                  \
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(FA[1][i], FB[0][j], acc[i][j], 0, 0, 0);   \
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(FA[0][i], FB[1][j], acc[i][j], 0, 0, 0);   \
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(FA[0][i], FB[0][j], acc[i][j], 0, 0, 0);   \
            }                                                                                                 \
    } while (0)
#define FPC_CONV_COMPUTE_H3(BUF)                                                                              \
    do {                                                                                                      \
        const char* Ab = reinterpret_cast<const char*>(lds) + (BUF) * (BM + BN) * kPlB + (wm * (BM / 2) + li) * 64;        \
        const char* Bb = reinterpret_cast<const char*>(lds) + (BUF) * (BM + BN) * kPlB + (BM + wn * (BN / 2) + li) * 64;   \
        f16x8 ha0[2][TM], hb0[2][TN], ha1[2][TM], hb1[2][TN];                                                 \
        FPC_H3_FRAG(0, ha0, hb0);                                                                             \
        FPC_H3_FRAG(1, ha1, hb1);                                                                             \
        __builtin_amdgcn_sched_barrier(0);                                                                    \
        __builtin_amdgcn_s_setprio(FPC_IGEMM_PRIO);                                                           \
        FPC_H3_MFMA(ha0, hb0);                                                                                \
        FPC_H3_MFMA(ha1, hb1);                                                                                \
        __builtin_amdgcn_s_setprio(0);                                                                        \
    } while (0)
    // ... with the split of the NEXT step's activation registers (ra -> the two planes of buffer BUF ^ 1) cut into 4 micro-steps
    // per row (two truncating conversions, four v_fma_mix residuals, two conversions, two 8-byte LDS stores) issued one after each
    // MFMA, as FPC_CONV_COMPUTE_STORE_BF3.  Not for the 128 x 128 tile.
#define FPC_CONV_COMPUTE_STORE_H3(BUF, ra)                                                                    \
    do {                                                                                                      \
        const char* Ab = reinterpret_cast<const char*>(lds) + (BUF) * (BM + BN) * kPlB + (wm * (BM / 2) + li) * 64;        \
        const char* Bb = reinterpret_cast<const char*>(lds) + (BUF) * (BM + BN) * kPlB + (BM + wn * (BN / 2) + li) * 64;   \
        char* st_ = reinterpret_cast<char*>(lds) + ((BUF) ^ 1) * (BM + BN) * kPlB;                            \
        f16x8 ha[2][2][TM], hb[2][2][TN];                                                                     \
        FPC_H3_FRAG(0, ha[0], hb[0]);                                                                         \
        FPC_H3_FRAG(1, ha[1], hb[1]);                                                                         \
        __builtin_amdgcn_sched_barrier(0);                                                                    \
        __builtin_amdgcn_s_setprio(FPC_IGEMM_PRIO);                                                           \
        constexpr int kNM = 6 * TM * TN, kNS = 4 * AR;      /* MFMAs, split micro-steps */                     \
        constexpr int kPa[3] = {1, 0, 0}, kPb[3] = {0, 1, 0};                                                 \
        fp16x2 sh1_[AR][2];                                                                                   \
        float sr_[AR][4];                                                                                     \
        u32x2 sp1_[AR], sp2_[AR];                                                                             \
        _Pragma("unroll") for (int m_ = 0; m_ < kNM; ++m_) {                                                  \
            const int kk_ = m_ / (3 * TM * TN), t_ = (m_ / 3) % (TM * TN), c_ = m_ % 3;                       \
            const int i_ = t_ / TN, j_ = t_ % TN;                                                             \
            acc[i_][j_] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ha[kk_][kPa[c_]][i_], hb[kk_][kPb[c_]][j_], acc[i_][j_], 0, 0, 0); \
            _Pragma("unroll") for (int ns_ = m_ * kNS / kNM; ns_ < (m_ + 1) * kNS / kNM; ++ns_) {             \
                const int r_ = ns_ / 4, ph_ = ns_ % 4;                                                        \
                if (ph_ == 0) {                                                                               \
                    const float x0_ = ra[r_][0], x1_ = ra[r_][1], x2_ = ra[r_][2], x3_ = ra[r_][3];           \
                    sh1_[r_][0] = __builtin_amdgcn_cvt_pkrtz(x0_, x1_);                                       \
                    sh1_[r_][1] = __builtin_amdgcn_cvt_pkrtz(x2_, x3_);                                       \
                }                                                                                             \
                if (ph_ == 1) { _Pragma("unroll") for (int e = 0; e < 4; ++e) { const float x_ = ra[r_][e]; sr_[r_][e] = __builtin_fmaf((float)sh1_[r_][e >> 1][e & 1], m1, x_); } } \
                if (ph_ == 2) {                                                                               \
                    sp1_[r_] = u32x2{__builtin_bit_cast(unsigned, sh1_[r_][0]), __builtin_bit_cast(unsigned, sh1_[r_][1])};           \
                    sp2_[r_] = u32x2{__builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(sr_[r_][0], sr_[r_][1])),                 \
                                     __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(sr_[r_][2], sr_[r_][3]))};                \
                }                                                                                             \
                if (ph_ == 3) {                                                                               \
                    char* d_ = st_ + (sr + 32 * r_) * 64 + bf3_w;                                             \
                    *reinterpret_cast<u32x2*>(d_) = sp1_[r_];                                                 \
                    *reinterpret_cast<u32x2*>(d_ + (BM + BN) * 64) = sp2_[r_];                                \
                }                                                                                             \
            }                                                                                                 \
            __builtin_amdgcn_sched_barrier(0);                                                                \
        }                                                                                                     \
        __builtin_amdgcn_s_setprio(0);                                                                        \
    } while (0)
#define FPC_CONV_STORE_H3(BUF, ra)                                                                            \
    do {                                                                                                      \
        char* st_ = reinterpret_cast<char*>(lds) + (BUF) * (BM + BN) * kPlB;                                  \
        _Pragma("unroll") for (int i = 0; i < AR; ++i) {                                                      \
            u32x2 p1_, p2_;                                                                                   \
            split_h2(ra[i], m1, p1_, p2_);                                                                    \
            char* d_ = st_ + (sr + 32 * i) * 64 + bf3_w;                                                      \
            *reinterpret_cast<u32x2*>(d_) = p1_;                                                              \
            *reinterpret_cast<u32x2*>(d_ + (BM + BN) * 64) = p2_;                                             \
        }                                                                                                     \
    } while (0)
#define FPC_STORE_ANY(BUF, ra, rb) do { if (H3) FPC_CONV_STORE_H3(BUF, ra); else if (BF3) FPC_CONV_STORE_BF3(BUF, ra, rb); else FPC_CONV_STORE(BUF, ra, rb); } while (0)
#define FPC_COMPUTE_ANY(BUF) do { if (H3) FPC_CONV_COMPUTE_H3(BUF); else if (BF3) FPC_CONV_COMPUTE_BF3(BUF); else FPC_CONV_COMPUTE(BUF); } while (0)
    // the interleaved split-and-compute block of the split forms (the 128 x 128 tile computes, then stores)
#define FPC_COMPUTE_STORE_SPLIT(BUF, ra) do { if constexpr (H3) FPC_CONV_COMPUTE_STORE_H3(BUF, ra); else FPC_CONV_COMPUTE_STORE_BF3(BUF, ra); } while (0)

    // Split precision: the weight planes of step k + 1 are DMA'd into the other LDS buffer at the start of step k (that buffer
    // was last read in step k - 1) and must have landed at the barrier that ends step k; the activation loads issued after
    // them (step k + 2) stay in flight across the barrier (counted vmcnt).
    if (ks0 < ks1) {
        if constexpr (DMAB) FPC_CONV_DMA_B(0);
        FPC_CONV_LOAD(ks0, ra0, rb0);
        FPC_STORE_ANY(0, ra0, rb0);
    }
    if (ks0 + 1 < ks1) FPC_CONV_LOAD(ks0 + 1, ra0, rb0);
    if constexpr (DMAB) FPC_CONV_DMA_WAIT(ks0 + 1 < ks1);
    __syncthreads();
#ifdef FPC_STAMP_IGEMM
    const long long st1 = clock64();
#endif
    for (int ks = ks0; ks < ks1; ks += 2) {
        // even phase: LDS buffer 0 holds step ks, set 0 holds ks+1
        if constexpr (DMAB) { if (ks + 1 < ks1) FPC_CONV_DMA_B(1); }
        if (ks + 2 < ks1) FPC_CONV_LOAD(ks + 2, ra1, rb1);
        if constexpr (DMAB && FPC_IGEMM_INTERLEAVE && BM * BN < 128 * 128) FPC_COMPUTE_STORE_SPLIT(0, ra0);
        else {
            FPC_COMPUTE_ANY(0);
            if (ks + 1 < ks1) FPC_STORE_ANY(1, ra0, rb0);
        }
        if constexpr (DMAB) FPC_CONV_DMA_WAIT(ks + 2 < ks1);
        __syncthreads();
        if (ks + 1 >= ks1) break;
        // odd phase: LDS buffer 1 holds step ks+1, set 1 holds ks+2
        if constexpr (DMAB) { if (ks + 2 < ks1) FPC_CONV_DMA_B(0); }
        if (ks + 3 < ks1) FPC_CONV_LOAD(ks + 3, ra0, rb0);
        if constexpr (DMAB && FPC_IGEMM_INTERLEAVE && BM * BN < 128 * 128) FPC_COMPUTE_STORE_SPLIT(1, ra1);
        else {
            FPC_COMPUTE_ANY(1);
            if (ks + 2 < ks1) FPC_STORE_ANY(0, ra1, rb1);
        }
        if constexpr (DMAB) FPC_CONV_DMA_WAIT(ks + 3 < ks1);
        __syncthreads();
    }
#pragma clang diagnostic pop
    // H3: the sums are of weights scaled by s = 2^k; 1 / s is a power of two, so this is exact — the epilogue and the split-K
    // partials (k_conv_splitk_epilogue, the fused last-arriver sum) see unscaled sums
    if constexpr (H3) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] *= h3_inv;
    }

#ifdef FPC_STAMP_IGEMM
    const long long st2 = clock64();
#endif
    // C/D layout of the 32x32 tile: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5),
    // i.e. a lane holds 16 rows of ONE channel.  Each wave transposes its tile through a private LDS
    // patch (the operand buffers are free after the last barrier) so that a lane owns 4 consecutive
    // channels of 4 rows: every global access of the epilogue is then 16 bytes per lane and a row's
    // 32 channels are one 128-byte segment (scalar 4-byte stores made the 1x1 laterals store-issue bound).
    constexpr int kTS = 36;                                   // floats per transposed row
    float* tp = lds + wave * 32 * kTS;
    const int trow = lane >> 3, tc4 = (lane & 7) * 4;         // rows trow + 8k (k < 4), channels tc4 .. tc4+3
    const int Wu = Wo >> 1, Hu = a.Ho >> 1;
    // split-K: partials of split s at ws0 + s * ws_split; padded rows / columns exist
    const size_t ws_split = (size_t)nB * mtiles * BM * Npad;
    float* ws0 = nsplit > 1 ? a.splitk_ws + (((size_t)grp * nsplit * nB + b) * ((size_t)mtiles * BM)) * Npad : nullptr;
    float* ws = ws0 ? ws0 + sp * ws_split : nullptr;
    const bool fused = a.fused != 0;
    const EpiGeom eg{b, HoWo, Wo, Cout, Hu, Wu, mtiles * (BM / 32), a.relu, lane};
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            // (this tile's epilogue operands are requested first: they land while the tile goes through the LDS patch)
            EpiPre pre;
            if (!ws) conv_epilogue_prefetch(pre, P, eg, m0 + wm * (BM / 2) + i * 32 + trow, n0 + wn * (BN / 2) + j * 32 + tc4);
#pragma unroll
            for (int r = 0; r < 16; ++r) tp[((r & 3) + 8 * (r >> 2) + 4 * lh) * kTS + li] = acc[i][j][r];
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // same wave: LDS ops complete in order
            f32x4 v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = *reinterpret_cast<const f32x4*>(tp + (trow + 8 * k) * kTS + tc4);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // reads done before the next tile overwrites the patch
            const int prow = m0 + wm * (BM / 2) + i * 32;
            const int n = n0 + wn * (BN / 2) + j * 32 + tc4;
            if (ws) {                                          // split-K: raw partial sums
                if (fused) {                                   // read by another workgroup of this launch: write-through
#pragma unroll
                    for (int k = 0; k < 4; ++k) store_wt128(ws + (size_t)(prow + trow + 8 * k) * Npad + n, v[k]);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        *reinterpret_cast<f32x4*>(ws + (size_t)(prow + trow + 8 * k) * Npad + n) = v[k];
                }
                continue;
            }
            conv_epilogue(P, eg, v[0], v[1], v[2], v[3], prow + trow, n, pre);
        }
    // Fused split-K: every workgroup has written its raw partial tile through to memory; it drains, and takes a ticket
    // of its output tile.  The one that draws the last ticket sums ALL partials in split order (its own included: the
    // sum does not depend on who arrives last; the same order as k_conv_splitk_epilogue) and applies the epilogue.
    if (ws && fused) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (t == 0) {
            int* tk = a.tickets + (((size_t)grp * nB + b) * mtiles + mt) * ntiles + nt;
            const int got = __hip_atomic_fetch_add(tk, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (got == nsplit - 1) __hip_atomic_store(tk, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // for the next launch
            s_last = got == nsplit - 1;
        }
        __syncthreads();
        if (s_last) {
#pragma unroll 1
            for (int ij = 0; ij < TM * TN; ++ij) {
                const int i = ij / TN, j = ij - i * TN;
                const int prow = m0 + wm * (BM / 2) + i * 32;
                const int n = n0 + wn * (BN / 2) + j * 32 + tc4;
                const float* src = ws0 + (size_t)(prow + trow) * Npad + n;
                EpiPre pre;
                conv_epilogue_prefetch(pre, P, eg, prow + trow, n);      // beside the partial sums' loads
                f32x4 v[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = load_wt128(src + (size_t)(8 * k) * Npad);
#pragma unroll 2
                for (int q = 1; q < nsplit; ++q) {
                    f32x4 u[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) u[k] = load_wt128(src + q * ws_split + (size_t)(8 * k) * Npad);
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] += u[k];
                }
                conv_epilogue(P, eg, v[0], v[1], v[2], v[3], prow + trow, n, pre);
            }
        }
    }
#ifdef FPC_STAMP_IGEMM
    if (a.dbg && lane == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        long long* o = (long long*)a.dbg + ((size_t)blockIdx.x * 4 + wave) * 4;
        o[0] = st1 - st0; o[1] = st2 - st1; o[2] = clock64() - st2; o[3] = ks1 - ks0;
    }
#endif
}

// Sums the split-K partials in split order and applies the epilogue.
// grid (P32 * nchunk, B, G): one workgroup = 32 rows x 128 channels; thread = 4 rows x 4 channels, so a
// split costs every thread four independent 16-byte loads (unrolled over splits for more in flight).
__global__ __launch_bounds__(256) void k_conv_splitk_epilogue(const ConvArgs a) {
    __shared__ float s_sum[8][128][2];
    ConvPtrs P = a.p[0];
    if (blockIdx.z == 1) P = a.p[1];
    if (blockIdx.z == 2) P = a.p[2];
    if (blockIdx.z == 3) P = a.p[3];
    const int t = threadIdx.x, rg = t >> 5, cq = t & 31;
    const int nchunk = (a.Cout + 127) >> 7;
    const int b = blockIdx.y, tile = blockIdx.x / nchunk, nc = (blockIdx.x - tile * nchunk) * 128;
    const int HoWo = a.Ho * a.Wo, Mp = a.mtiles * a.bm, nsplit = a.nsplit, Npad = a.Npad, Cout = a.Cout;
    const int Wu = a.Wo >> 1, Hu = a.Ho >> 1;
    const int P32 = a.mtiles * a.bm / 32;
    const int n = nc + 4 * cq;
    const bool nv = n < Cout;     // Cout % 4 == 0 on this path
    f32x4 v[4];
    bool rv[4];
    const float* src[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int p = tile * 32 + rg + 8 * j;
        rv[j] = nv && p < HoWo;
        v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        src[j] = a.splitk_ws + (((size_t)blockIdx.z * nsplit * a.B + b) * (size_t)Mp + (rv[j] ? p : 0)) * Npad + (nv ? n : 0);
    }
    const size_t sstride = (size_t)a.B * Mp * Npad;
#pragma unroll 4
    for (int sp = 0; sp < nsplit; ++sp) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] += *reinterpret_cast<const f32x4*>(src[j] + sp * sstride);
    }
    f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
    if (nv && P.scale) sc = *reinterpret_cast<const f32x4*>(P.scale + n);
    if (nv && P.shift) sh = *reinterpret_cast<const f32x4*>(P.shift + n);
    f32x4 cs1 = {0.f, 0.f, 0.f, 0.f}, cs2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (!rv[j]) continue;
        int p = tile * 32 + rg + 8 * j;
        f32x4 x = v[j];
        if (P.scale) x = x * sc;
        x = x + sh;
        size_t o = ((size_t)b * HoWo + p) * Cout + n;
        if (P.res) x += *reinterpret_cast<const f32x4*>(P.res + o);
        if (P.up) {
            int ho = p / a.Wo, wo = p - ho * a.Wo;
            x += *reinterpret_cast<const f32x4*>(P.up + (((size_t)b * Hu + (ho >> 1)) * Wu + (wo >> 1)) * Cout + n);
        }
        if (a.relu) { x[0] = fmaxf(x[0], 0.f); x[1] = fmaxf(x[1], 0.f); x[2] = fmaxf(x[2], 0.f); x[3] = fmaxf(x[3], 0.f); }
        *reinterpret_cast<f32x4*>(P.out + o) = x;
        cs1 += x;
        cs2 += x * x;
    }
    if (P.gn_part) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { s_sum[rg][4 * cq + e][0] = cs1[e]; s_sum[rg][4 * cq + e][1] = cs2[e]; }
        __syncthreads();
        if (t < 128 && nc + t < Cout) {
            float u = 0.f, w = 0.f;
#pragma unroll
            for (int g = 0; g < 8; ++g) { u += s_sum[g][t][0]; w += s_sum[g][t][1]; }
            float* gp = P.gn_part + (((size_t)b * P32 + tile) * Cout + nc + t) * 2;
            gp[0] = u; gp[1] = w;
        }
    }
}

// ------------------------------------------------------------------------------------------
// parameter repacking (once per plan)

// OIHW [Cout][Cin][Kh][Kw] -> OHWI rows [Npad][Kpad], k = (kh*Kwp + kw)*Cinp + ci, zero padded.  Cinp >= Cin: channel
// padding of the input layout (4 for the RGB stem); Kwp >= Kw: taps per kernel row in the layout (8 for the stem,
// whose K-step is one kernel row = 8 consecutive 4-channel pixels)
__global__ __launch_bounds__(256) void k_pack_weight(const float* __restrict__ w, float* __restrict__ out, int Cout,
                                                     int Cin, int Cinp, int Kh, int Kw, int Kwp, int Npad, int Kpad) {
    long long total = (long long)Npad * Kpad;
    int K = Cinp * Kh * Kwp;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long long)gridDim.x * blockDim.x) {
        int k = (int)(g % Kpad), n = (int)(g / Kpad);
        float v = 0.f;
        if (n < Cout && k < K) {
            int tap = k / Cinp, ci = k - tap * Cinp;
            int kh = tap / Kwp, kw = tap - kh * Kwp;
            if (ci < Cin && kw < Kw) v = w[(((size_t)n * Cin + ci) * Kh + kh) * Kw + kw];
        }
        out[g] = v;
    }
}

// The same [Npad][Kpad] image split EXACTLY into three bf16 planes (x = b1 + b2 + b3 by truncation, as split_bf3):
// out[(plane * Npad + n) * Kpad + k] — the weight operand of the split-precision direct convolution, staged by LDS-DMA.
__global__ __launch_bounds__(256) void k_pack_weight_bf3(const float* __restrict__ w, unsigned short* __restrict__ out, int Cout,
                                                       int Cin, int Cinp, int Kh, int Kw, int Kwp, int Npad, int Kpad) {
    const int K = Cinp * Kh * Kwp;
    long long total = (long long)Npad * Kpad;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long long)gridDim.x * blockDim.x) {
        int n = (int)(g / Kpad), k = (int)(g - (long long)n * Kpad);
        float v = 0.f;
        if (n < Cout && k < K) {
            int tap = k / Cinp, ci = k - tap * Cinp;
            int kh = tap / Kwp, kw = tap - kh * Kwp;
            if (ci < Cin && kw < Kw) v = w[(((size_t)n * Cin + ci) * Kh + kh) * Kw + kw];
        }
        const unsigned b1 = __builtin_bit_cast(unsigned, v) & 0xFFFF0000u;
        const float r = v - __builtin_bit_cast(float, b1);
        const unsigned b2 = __builtin_bit_cast(unsigned, r) & 0xFFFF0000u;
        const float q = r - __builtin_bit_cast(float, b2);
        out[g] = (unsigned short)(b1 >> 16);
        out[total + g] = (unsigned short)(b2 >> 16);
        out[2 * total + g] = (unsigned short)(__builtin_bit_cast(unsigned, q) >> 16);
    }
}

// The same [Npad][Kpad] image as TWO fp16 planes for k_conv_igemm's three-product form: scaled by s = 2^k, the largest power of
// two with max |w| s < 2^13 (k_wino_pack_fp16's rule without the transform's 2.25; max |w| from k_absmax_bits in tail[1]), and split
// by truncation, w s = g1 + g2 + rest with |rest| <= 3 * 2^-23 |w s| (< 2^-24 where |w s| < 2^-2): out[(plane * Npad + n) * Kpad + k], tail[0] = 1 / s.
__global__ __launch_bounds__(256) void k_pack_weight_h3(const float* __restrict__ w, unsigned short* __restrict__ out, float* __restrict__ tail,
                                                        int Cout, int Cin, int Cinp, int Kh, int Kw, int Kwp, int Npad, int Kpad) {
    const float wmax = __builtin_bit_cast(float, reinterpret_cast<const unsigned*>(tail)[1]);
    int ex = 0;
    if (wmax > 0.f && wmax < 3.0e38f) { (void)frexpf(wmax, &ex); ex = 13 - ex; }      // wmax = m 2^e, m in [0.5, 1): wmax 2^(13 - e) < 2^13
    ex = max(-100, min(100, ex));
    const float sc = ldexpf(1.0f, ex);
    if (blockIdx.x == 0 && threadIdx.x == 0) tail[0] = ldexpf(1.0f, -ex);
    const int K = Cinp * Kh * Kwp;
    const long long total = (long long)Npad * Kpad;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long long)gridDim.x * blockDim.x) {
        int n = (int)(g / Kpad), k = (int)(g - (long long)n * Kpad);
        float v = 0.f;
        if (n < Cout && k < K) {
            int tap = k / Cinp, ci = k - tap * Cinp;
            int kh = tap / Kwp, kw = tap - kh * Kwp;
            if (ci < Cin && kw < Kw) v = w[(((size_t)n * Cin + ci) * Kh + kh) * Kw + kw] * sc;      // (a power of two: exact)
        }
        const fp16x2 h = __builtin_amdgcn_cvt_pkrtz(v, 0.f);
        const float r = v - (float)h[0];
        const fp16x2 h2 = __builtin_amdgcn_cvt_pkrtz(r, 0.f);
        out[g] = (unsigned short)(__builtin_bit_cast(unsigned, h) & 0xFFFFu);
        out[total + g] = (unsigned short)(__builtin_bit_cast(unsigned, h2) & 0xFFFFu);
    }
}

// ------------------------------------------------------------------------------------------
// launch wrappers

template <int BM, int BN>
static void launch_conv_t(const ConvArgs& a, int groups, hipStream_t s) {
    dim3 grid(a.mtiles * a.B * a.ntiles * a.nsplit * groups);
    if (a.generic == 0 && a.h3)
        hipLaunchKernelGGL((k_conv_igemm<BM, BN, 0, false, true>), grid, dim3(256), 0, s, a);
    else if (a.generic == 0 && a.bf3)
        hipLaunchKernelGGL((k_conv_igemm<BM, BN, 0, true>), grid, dim3(256), 0, s, a);
    else if (a.generic == 0)
        hipLaunchKernelGGL((k_conv_igemm<BM, BN, 0>), grid, dim3(256), 0, s, a);
    else if (a.generic == 2)
        hipLaunchKernelGGL((k_conv_igemm<BM, BN, 2>), grid, dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((k_conv_igemm<BM, BN, 1>), grid, dim3(256), 0, s, a);
}

// a.generic: 0 = Cin % 32 == 0 channel-last (fast path), 2 = Cin % 4 == 0 channel-last (per-lane tap decode),
//            1 = anything (scalar gathers)
int launch_conv(const ConvArgs& a, int groups, hipStream_t s) {
    if (groups < 1 || groups > kMaxGroup || a.Npad % a.bn != 0 || a.Kpad % kConvBK != 0) return FPC_EINVAL;
#ifndef FPC_STAMP_IGEMM
    if (a.dbg) return FPC_EINVAL;      // a stamp buffer needs the diagnostic build
#endif
    if (a.generic == 0 && (a.Cin % kConvBK != 0 || a.in_sc != 1 || a.Kh * a.Kw > 32 ||
                           ((long long)a.Hi + 2 * a.pad) * a.in_sh * 4 >= (1LL << 31)))
        return FPC_EINVAL;      // tap mask is 32 bits, lane offsets are 31 bits
    if ((long long)a.Npad * a.Kpad * 4 >= (1LL << 31)) return FPC_EINVAL;
    if (a.h3 && (a.generic != 0 || a.bf3 || a.lanepx)) return FPC_EINVAL;      // the three-product form rides on the fast loader alone
    if (a.nsplit > 1 && a.fused && (!a.tickets || (long long)groups * a.B * a.mtiles * a.ntiles > kConvTickets || a.Cout % 4 != 0))
        return FPC_EINVAL;
    if (a.generic == 2 && (a.Cin % 4 != 0 || a.in_sc != 1 || a.in_sw % 4 != 0 || a.in_sh % 4 != 0 || a.in_sb % 4 != 0))
        return FPC_EINVAL;
    if (a.bm == 128 && a.bn == 128) launch_conv_t<128, 128>(a, groups, s);
    else if (a.bm == 128 && a.bn == 64) launch_conv_t<128, 64>(a, groups, s);
    else if (a.bm == 64 && a.bn == 128) launch_conv_t<64, 128>(a, groups, s);
    else if (a.bm == 64 && a.bn == 64) launch_conv_t<64, 64>(a, groups, s);
    else return FPC_EINVAL;
    return check_launch();
}

int launch_conv_splitk_epilogue(const ConvArgs& a, int groups, hipStream_t s) {
    if (a.Cout % 4 != 0) return FPC_EINVAL;
    hipLaunchKernelGGL(k_conv_splitk_epilogue, dim3((a.mtiles * a.bm / 32) * cdiv(a.Cout, 128), a.B, groups), dim3(256), 0, s,
                       a);
    return check_launch();
}

int launch_pack_weight(const float* w, float* packed, int Cout, int Cin, int Cinp, int Kh, int Kw, int Kwp, int Npad,
                       int Kpad, hipStream_t s) {
    if (Kwp < Kw || Cinp < Cin) return FPC_EINVAL;
    hipLaunchKernelGGL(k_pack_weight, dim3(stream_grid((long long)Npad * Kpad)), dim3(256), 0, s, w, packed, Cout, Cin,
                       Cinp, Kh, Kw, Kwp, Npad, Kpad);
    return check_launch();
}

int launch_pack_weight_bf3(const float* w, float* packed, int Cout, int Cin, int Cinp, int Kh, int Kw, int Kwp, int Npad,
                           int Kpad, hipStream_t s) {
    if (Kwp < Kw || Cinp < Cin) return FPC_EINVAL;
    hipLaunchKernelGGL(k_pack_weight_bf3, dim3(stream_grid((long long)Npad * Kpad)), dim3(256), 0, s, w,
                       reinterpret_cast<unsigned short*>(packed + (size_t)Npad * Kpad), Cout, Cin, Cinp, Kh, Kw, Kwp, Npad, Kpad);
    return check_launch();
}

int launch_pack_weight_h3(const float* w, float* packed, int Cout, int Cin, int Cinp, int Kh, int Kw, int Kwp, int Npad,
                          int Kpad, hipStream_t s) {
    if (Kwp < Kw || Cinp < Cin || ((uintptr_t)w & 15)) return FPC_EINVAL;
    float* tail = packed + (size_t)Npad * Kpad;
    if (hipMemsetAsync(tail, 0, 2 * sizeof(float), s) != hipSuccess) return FPC_ELAUNCH;
    const int rc = launch_absmax_bits(w, (long long)Cout * Cin * Kh * Kw, reinterpret_cast<unsigned*>(tail) + 1, s);
    if (rc) return rc;
    hipLaunchKernelGGL(k_pack_weight_h3, dim3(stream_grid((long long)Npad * Kpad)), dim3(256), 0, s, w,
                       reinterpret_cast<unsigned short*>(packed), tail, Cout, Cin, Cinp, Kh, Kw, Kwp, Npad, Kpad);
    return check_launch();
}

}  // namespace fpc
