// inflate.hpp — RFC 1950 (zlib wrapper) and RFC 1951 (DEFLATE) written once, for the host and for one wave of the device.
// No zlib in here: png_device.hip's k_png_inflate and the host entry fpc_inflate_host instantiate the SAME template, so the
// CPU suite (tests/test_png_inflate_host.py) exercises the code the kernel runs, ring, flush and table build included.
//
// Shape of the decoder.  The decode state (bit buffer, positions, block state) is the same in every lane of the wave
// ("wave-uniform"); an IO policy says what a lane is:
//     IO::kLanes                       1 on the host, 64 on the device
//     io.lane()                        this lane's index
//     io.uni(v)                        a value every lane holds alike (readfirstlane on the device: keeps the state scalar)
//     io.sum(v)                        the sum of v over the lanes
//     io.sync()                        stores of any lane to the ring / tables / stage are visible to every lane afterwards
//     io.in32(pos) / io.in8(pos)       input bytes; the core only asks for pos (+4) <= zbytes
//     io.store_piece(pos, src, nb)     16 output bytes (the last piece: nb < 16) from the ring to out + pos, pos % 16 == 0
//     io.ring, io.t                    the 32 KiB window and the tables of the current block (LDS on the device)
//     io.peek_all(tab, bb, mask)       h: the table entry of the code starting at bit i of bb, for every i a lane stands for
//     io.peek_at(h, i)                 that entry (i < 64)
//     io.lit_put(op, k, byte), io.lit_commit(op, k)    the k-th literal of a run; the run's k bytes to ring[op ..]
// The lanes share three jobs: copying a match (out[op + j] = out[op - D + j % D], no dependency between the j), filling the
// decode tables, and flushing the ring to the output in 16-byte pieces while summing Adler-32 over the flushed bytes.
//
// TERMINATION BY CONSTRUCTION.  Every iteration of every data-dependent loop either consumes at least one input bit
// (header fields, code lengths, Huffman symbols, stored bytes, trailer) or emits at least one output byte (a match), and
// both positions are checked before the step: the bit reader never moves past `zbytes`, the writer never past `expect`
// (= H (1 + W bpp) for a PNG).  A block costs, beyond its bits, a constant (table build: <= 320 symbols, <= 4608 table
// entries) and consumes at least 3 bits.  Total work is therefore bounded by  C * (8 * zbytes + expect)  whatever the
// bytes are, with C a constant of the code, not of the data.
//
// NO ACCESS OUTSIDE [in, in + zbytes) AND [out, out + cap): the IO policies keep that (the device policy reads and writes
// whole 16-byte pieces of slices that are padded to 16 bytes by their owner); table indices are masked or range-checked.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FPC_INF_HD __host__ __device__ __attribute__((always_inline))      // out of line, the state lives in memory: 15 x slower on the device
#else
#define FPC_INF_HD __attribute__((always_inline))
#endif

namespace fpc_inflate {

// one status per failure class (include/fpc.h: FPC_INF_*)
enum : int {
    OK = 0,
    E_TRUNCATED = 1,        // the stream ends inside a field
    E_BLOCK_TYPE = 2,       // BTYPE 3
    E_STORED_LEN = 3,       // LEN != ~NLEN
    E_OVERSUBSCRIBED = 4,   // a set of code lengths claims more codes than exist
    E_INCOMPLETE = 5,       // a set of code lengths leaves codes unused (other than a single 1-bit code)
    E_REPEAT_FIRST = 6,     // code-length symbol 16 with no previous length
    E_LITLEN_SYMBOL = 7,    // literal/length symbol 286 or 287
    E_DIST_SYMBOL = 8,      // distance symbol 30 or 31
    E_DIST_TOO_FAR = 9,     // a distance before the start of the output (or beyond the declared window)
    E_OUT_OVERFLOW = 10,    // more output than `expect`
    E_OUT_SHORT = 11,       // the stream ends with less output than `expect`
    E_ADLER = 12,           // Adler-32 trailer mismatch
    E_FDICT = 13,           // a preset dictionary is asked for
    E_METHOD = 14,          // CM != 8 or a window beyond 32 KiB
    E_FCHECK = 15,          // the header's check bits
    E_LENGTHS_OVERRUN = 16, // a code-length repeat runs past HLIT + HDIST
    E_NO_END_CODE = 17,     // the literal/length code has no end-of-block symbol
    E_BAD_CODE = 18         // bits that no code of an (allowed) incomplete set matches
};

constexpr int kRing = 32768;          // the window, a ring: byte p of the output lives at ring[p & (kRing - 1)]
constexpr int kFlushAt = 16384;       // un-flushed bytes that trigger a flush; kFlushAt + 258 + 15 <= kRing
constexpr int kLitBits = 12, kDistBits = 9;       // 12: a photograph's literal code has 11- and 12-bit members in every block

struct Tables {                       // 10304 bytes
    uint16_t lit[1 << kLitBits];      // (symbol << 4) | length for codes of <= kLitBits bits, 0: take the canonical walk
    uint16_t dist[1 << kDistBits];
    uint16_t lsorted[288], dsorted[32];               // symbols in canonical order
    uint16_t lcnt[16], dcnt[16];                      // codes per length
    uint16_t offs[16], first[16];                     // build scratch: first sorted index / first code of each length
    uint8_t lens[320];                                // the code lengths as read
};

struct Bits {
    uint64_t bb = 0;                  // bits not yet consumed, LSB first; zero above bc
    int bc = 0;
    uint32_t ip = 0, n = 0;           // next input byte, input size
};

template <class IO>
FPC_INF_HD inline void refill(IO& io, Bits& b) {
    if (b.bc > 32) return;
    if (b.ip + 4 <= b.n && (b.ip & 3) == 0) {
        b.bb |= (uint64_t)io.in32(b.ip) << b.bc;
        b.ip += 4;
        b.bc += 32;
    } else {
        while (b.bc <= 56 && b.ip < b.n) {
            b.bb |= (uint64_t)io.in8(b.ip) << b.bc;
            b.ip += 1;
            b.bc += 8;
        }
    }
}

// k <= 16 bits, or E_TRUNCATED
template <class IO>
FPC_INF_HD inline int getbits(IO& io, Bits& b, int k, uint32_t& v) {
    refill(io, b);
    if (b.bc < k) return E_TRUNCATED;
    v = (uint32_t)b.bb & ((1u << k) - 1u);
    b.bb >>= k;
    b.bc -= k;
    return OK;
}

FPC_INF_HD inline uint32_t bitrev(uint32_t code, int len) {
    uint32_t r = 0;
    for (int i = 0; i < len; ++i) r |= ((code >> i) & 1u) << (len - 1 - i);
    return r;
}

// kind 0: the code-length code (must be complete), 1: literal/length, 2: distance
template <class IO>
FPC_INF_HD inline int build(IO& io, const uint8_t* lens, int n, uint16_t* tab, int tb, uint16_t* sorted, uint16_t* cnt, Tables& t,
                        int kind) {
    int st = OK, nsym = 0;
    if (io.lane() == 0) {
        for (int l = 0; l < 16; ++l) cnt[l] = 0;
        for (int s = 0; s < n; ++s) cnt[lens[s] & 15] += 1;
        int left = 1, maxl = 0;
        for (int l = 1; l < 16 && st == OK; ++l) {
            left = (left << 1) - (int)cnt[l];
            if (left < 0) st = E_OVERSUBSCRIBED;
            if (cnt[l]) maxl = l;
        }
        if (st == OK && left > 0 && (kind == 0 || maxl > 1)) st = E_INCOMPLETE;
        if (st == OK) {
            uint16_t next[16];
            uint32_t code = 0, o = 0;
            for (int l = 1; l < 16; ++l) {
                code = (code + (l > 1 ? cnt[l - 1] : 0)) << 1;
                t.first[l] = (uint16_t)code;
                t.offs[l] = next[l] = (uint16_t)o;
                o += cnt[l];
            }
            nsym = (int)o;
            for (int s = 0; s < n; ++s)
                if (lens[s] & 15) sorted[next[lens[s] & 15]++] = (uint16_t)s;
        }
    }
    st = (int)io.uni((uint32_t)st);
    if (st != OK) return st;
    nsym = (int)io.uni((uint32_t)nsym);
    for (int j = io.lane(); j < (1 << tb); j += IO::kLanes) tab[j] = 0;
    io.sync();
    for (int k = io.lane(); k < nsym; k += IO::kLanes) {
        const int s = sorted[k], l = lens[s] & 15;
        if (l <= tb) {
            const uint32_t r = bitrev((uint32_t)t.first[l] + (uint32_t)(k - (int)t.offs[l]), l);
            for (uint32_t j = r; j < (1u << tb); j += 1u << l) tab[j] = (uint16_t)((s << 4) | l);
        }
    }
    io.sync();
    return OK;
}

// one Huffman symbol: consumes its 1 .. 15 bits
template <class IO>
FPC_INF_HD inline int decode(IO& io, Bits& b, const uint16_t* tab, int tb, const uint16_t* cnt, const uint16_t* sorted, int nsorted,
                         int& sym) {
    refill(io, b);
    const uint32_t v = (uint32_t)b.bb;
    const uint32_t e = io.uni(tab[v & ((1u << tb) - 1u)]);
    int l;
    if (e) {
        l = (int)(e & 15u);
        sym = (int)(e >> 4);
    } else {                                      // canonical walk, one bit a step (codes longer than the table, or none)
        int code = 0, first = 0, index = 0;
        sym = -1;
        for (l = 1; l <= 15; ++l) {
            code |= (int)((v >> (l - 1)) & 1u);
            const int c = (int)io.uni(cnt[l]);
            if (code - c < first) {
                const int k = index + (code - first);
                if (k >= 0 && k < nsorted) sym = (int)io.uni(sorted[k]);
                break;
            }
            index += c;
            first = (first + c) << 1;
            code <<= 1;
        }
        if (sym < 0) return b.bc < 15 ? E_TRUNCATED : E_BAD_CODE;
    }
    if (l > b.bc) return E_TRUNCATED;
    b.bb >>= l;
    b.bc -= l;
    return OK;
}

template <class IO>
struct Inflater {
    IO& io;
    Bits b;
    uint32_t op = 0, fp = 0, expect = 0;          // bytes produced, bytes flushed (multiple of 16 until the end), bytes wanted
    uint32_t s1 = 1, s2 = 0;                      // Adler-32 of out[0, fp)

    FPC_INF_HD explicit Inflater(IO& io_) : io(io_) {}

    // ring[fp, end) -> out, Adler-32 carried over it; end = op at the end of the stream, else op rounded down to 16
    FPC_INF_HD void flush(bool last) {
        io.sync();
        const uint32_t end = last ? op : (op & ~15u);
        const uint32_t n = end - fp, pieces = (n + 15u) >> 4;
        uint64_t sd = 0, sw = 0;                  // sum d[i], sum (n - i) d[i] over this lane's bytes, i counted from fp
        for (uint32_t q = (uint32_t)io.lane(); q < pieces; q += (uint32_t)IO::kLanes) {
            const uint32_t i0 = q << 4, nb = n - i0 < 16u ? n - i0 : 16u;
            const uint8_t* src = io.ring + ((fp + i0) & (uint32_t)(kRing - 1));
            uint32_t d = 0, kd = 0;
            for (uint32_t k = 0; k < nb; ++k) {
                d += src[k];
                kd += k * src[k];
            }
            sd += d;
            sw += (uint64_t)(n - i0) * d - kd;
            io.store_piece(fp + i0, src, nb);
        }
        const uint32_t S = io.sum((uint32_t)(sd % 65521u)) % 65521u, Wt = io.sum((uint32_t)(sw % 65521u)) % 65521u;
        s2 = (uint32_t)((s2 + (uint64_t)(n % 65521u) * s1 + Wt) % 65521u);
        s1 = (s1 + S) % 65521u;
        fp = end;
    }

    FPC_INF_HD int literal(uint32_t byte) {
        if (op >= expect) return E_OUT_OVERFLOW;
        if (op - fp >= (uint32_t)kFlushAt) flush(false);
        if (io.lane() == 0) io.ring[op & (uint32_t)(kRing - 1)] = (uint8_t)byte;
        op += 1;
        return OK;
    }

    // L in 3 .. 258, D in 1 .. 32768
    FPC_INF_HD int match(uint32_t L, uint32_t D, uint32_t window) {
        if (D > op || D > window) return E_DIST_TOO_FAR;
        if (L > expect - op) return E_OUT_OVERFLOW;
        if (op - fp >= (uint32_t)kFlushAt) flush(false);
        io.sync();                                // the literals lane 0 wrote, the bytes of the match before this one
        const uint32_t from = op - D;
        for (uint32_t j = (uint32_t)io.lane(); j < L; j += (uint32_t)IO::kLanes) {
            const uint32_t o = j < D ? j : j % D;                 // an overlapping match repeats its first D bytes
            const uint8_t v = io.ring[(from + o) & (uint32_t)(kRing - 1)];
            io.ring[(op + j) & (uint32_t)(kRing - 1)] = v;        // D <= kRing: a slot is read no later than it is rewritten
        }
        op += L;
        return OK;
    }

    FPC_INF_HD int stored() {
        uint32_t v, len, nlen;
        int st;
        if ((st = getbits(io, b, b.bc & 7, v)) != OK) return st;  // to the byte boundary
        if ((st = getbits(io, b, 16, len)) != OK) return st;
        if ((st = getbits(io, b, 16, nlen)) != OK) return st;
        if (len != (~nlen & 0xffffu)) return E_STORED_LEN;
        for (uint32_t i = 0; i < len; ++i) {
            if ((st = getbits(io, b, 8, v)) != OK) return st;
            if ((st = literal(v)) != OK) return st;
        }
        return OK;
    }

    FPC_INF_HD int fixed_tables() {
        Tables& t = *io.t;
        if (io.lane() == 0) {
            for (int s = 0; s < 288; ++s) t.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
            for (int s = 0; s < 32; ++s) t.lens[288 + s] = 5;
        }
        io.sync();
        int st = build(io, t.lens, 288, t.lit, kLitBits, t.lsorted, t.lcnt, t, 1);
        if (st != OK) return st;
        return build(io, t.lens + 288, 32, t.dist, kDistBits, t.dsorted, t.dcnt, t, 2);      // 30 and 31 decode, then fail
    }

    FPC_INF_HD int dynamic_tables(int& nlit, int& ndist) {
        Tables& t = *io.t;
        uint32_t v;
        int st;
        if ((st = getbits(io, b, 14, v)) != OK) return st;
        nlit = (int)(v & 31u) + 257;
        ndist = (int)((v >> 5) & 31u) + 1;
        const int ncode = (int)(v >> 10) + 4;
        if (nlit > 286) return E_LITLEN_SYMBOL;
        if (ndist > 30) return E_DIST_SYMBOL;
        const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        uint32_t cl[19];
        for (int i = 0; i < 19; ++i) cl[i] = 0;
        for (int i = 0; i < ncode; ++i) {
            if ((st = getbits(io, b, 3, v)) != OK) return st;
            cl[i] = v;
        }
        io.sync();                                // the previous block's readers of lens / tables are done
        if (io.lane() == 0)
            for (int i = 0; i < 19; ++i) t.lens[order[i]] = (uint8_t)cl[i];
        io.sync();
        if ((st = build(io, t.lens, 19, t.lit, 7, t.lsorted, t.lcnt, t, 0)) != OK) return st;
        const int total = nlit + ndist;           // <= 288 + 32
        int i = 0;
        uint32_t prev = 0;
        uint8_t* lens = t.lens;
        // the lengths overwrite the 19 code-length-code lengths they are decoded with: those live on in lit / lsorted / lcnt only
        while (i < total) {
            int sym;
            if ((st = decode(io, b, t.lit, 7, t.lcnt, t.lsorted, 19, sym)) != OK) return st;
            uint32_t rep = 1, val = (uint32_t)sym;
            if (sym == 16) {
                if (i == 0) return E_REPEAT_FIRST;
                if ((st = getbits(io, b, 2, v)) != OK) return st;
                rep = 3 + v;
                val = prev;
            } else if (sym == 17) {
                if ((st = getbits(io, b, 3, v)) != OK) return st;
                rep = 3 + v;
                val = 0;
            } else if (sym == 18) {
                if ((st = getbits(io, b, 7, v)) != OK) return st;
                rep = 11 + v;
                val = 0;
            } else if (sym > 18) {
                return E_BAD_CODE;
            }
            if ((uint32_t)i + rep > (uint32_t)total) return E_LENGTHS_OVERRUN;
            if (io.lane() == 0)
                for (uint32_t k = 0; k < rep; ++k) lens[i + (int)k] = (uint8_t)val;
            i += (int)rep;
            prev = val;
        }
        io.sync();
        if (io.uni(lens[256]) == 0) return E_NO_END_CODE;
        // build() of the literal/length code rewrites t.lit, lsorted, lcnt: the code-length code is no longer needed
        if ((st = build(io, lens, nlit, t.lit, kLitBits, t.lsorted, t.lcnt, t, 1)) != OK) return st;
        return build(io, lens + nlit, ndist, t.dist, kDistBits, t.dsorted, t.dcnt, t, 2);
    }

    FPC_INF_HD int coded(int nlit, int ndist, uint32_t window) {
        const uint16_t lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
        const uint8_t lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
        const uint16_t dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
        const uint8_t dext[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
        Tables& t = *io.t;
        const int nls = nlit < 288 ? nlit : 288, nds = ndist < 32 ? ndist : 32;
        for (;;) {
            int sym, st;
            uint32_t v;
            // A run of literals out of ONE table look-up: lane i looks up the code that would start at bit i of the bit buffer,
            // the chain bit 0 -> + its length -> ... then costs a lane read a symbol.  The run ends at anything that is not a
            // literal of a table-length code lying wholly inside the buffered bits; the general path below takes that symbol
            // (and reports what is wrong with it, if anything is).  A run consumes at least one bit or is empty.
            refill(io, b);
            if (op - fp >= (uint32_t)kFlushAt) flush(false);
            {
                const auto h = io.peek_all(t.lit, b.bb, (1u << kLitBits) - 1u);
                const uint32_t room = expect - op < 32u ? expect - op : 32u, bc = (uint32_t)b.bc;
                uint32_t pos = 0, k = 0;
                for (;;) {                        // one exit test a literal: branches, not arithmetic, set this loop's pace
                    const uint32_t e = io.peek_at(h, pos & 63u), next = pos + (e & 15u);      // (pos == bc == 64: any entry, next > bc)
                    // a table entry (e != 0, so its length is >= 1) of a literal (e < 256 << 4), inside the buffered bits, with room
                    if (!((e - 1u < 4095u) & (next <= bc) & (k < room))) break;
                    io.lit_put(op, k, e >> 4);
                    pos = next;
                    k += 1;
                }
                if (k) {
                    io.lit_commit(op, k);
                    op += k;
                    b.bb = pos >= 64u ? 0 : b.bb >> pos;
                    b.bc -= (int)pos;
                    continue;
                }
            }
            if ((st = decode(io, b, t.lit, kLitBits, t.lcnt, t.lsorted, nls, sym)) != OK) return st;
            if (sym < 256) {
                if ((st = literal((uint32_t)sym)) != OK) return st;
                continue;
            }
            if (sym == 256) return OK;
            if (sym > 285) return E_LITLEN_SYMBOL;
            sym -= 257;
            if ((st = getbits(io, b, lext[sym], v)) != OK) return st;
            const uint32_t L = lbase[sym] + v;
            if ((st = decode(io, b, t.dist, kDistBits, t.dcnt, t.dsorted, nds, sym)) != OK) return st;
            if (sym > 29) return E_DIST_SYMBOL;
            if ((st = getbits(io, b, dext[sym], v)) != OK) return st;
            if ((st = match(L, dbase[sym] + v, window)) != OK) return st;
        }
    }

    // the whole zlib stream; *produced = bytes written to out (all of them flushed, also on failure)
    FPC_INF_HD int run(uint32_t zbytes, uint32_t expect_, uint32_t* produced) {
        b.n = zbytes;
        expect = expect_;
        const int st = body();
        if (st != OK) flush(true);                // what was decoded is in `out`: op <= expect
        *produced = op;
        return st;
    }

    FPC_INF_HD int body() {
        uint32_t cmf, flg, v;
        int st;
        if ((st = getbits(io, b, 8, cmf)) != OK) return st;
        if ((st = getbits(io, b, 8, flg)) != OK) return st;
        if ((cmf & 15u) != 8u || (cmf >> 4) > 7u) return E_METHOD;
        if (((cmf << 8) | flg) % 31u) return E_FCHECK;
        if (flg & 0x20u) return E_FDICT;
        const uint32_t window = 1u << ((cmf >> 4) + 8);
        uint32_t last;
        do {
            if ((st = getbits(io, b, 3, v)) != OK) return st;
            last = v & 1u;
            const uint32_t type = v >> 1;
            if (type == 0) {
                st = stored();
            } else if (type == 1) {
                if ((st = fixed_tables()) == OK) st = coded(288, 32, window);
            } else if (type == 2) {
                int nlit = 0, ndist = 0;
                if ((st = dynamic_tables(nlit, ndist)) == OK) st = coded(nlit, ndist, window);
            } else {
                st = E_BLOCK_TYPE;
            }
            if (st != OK) return st;
        } while (!last);
        flush(true);
        if (op != expect) return E_OUT_SHORT;
        if ((st = getbits(io, b, b.bc & 7, v)) != OK) return st;
        uint32_t want = 0;
        for (int i = 0; i < 4; ++i) {
            if ((st = getbits(io, b, 8, v)) != OK) return st;
            want = (want << 8) | v;
        }
        return want == ((s2 << 16) | s1) ? OK : E_ADLER;
    }
};

}  // namespace fpc_inflate
