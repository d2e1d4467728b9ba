// png_header.hpp — the PNG signature and IHDR, read once for png_decode.hip (host decode) and png_device.hip (host pre-pass
// of the device decode): both refuse the same files.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/fpc.h"

namespace {

struct PngHeader { uint32_t w, h; int depth, ctype, channels, bpp; };

inline uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

const uint8_t kSig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};

// IHDR of a PNG in memory; FPC_OK, or FPC_EFORMAT for anything this decoder does not read
inline int parse_header(const uint8_t* d, size_t n, PngHeader& h) {
    if (n < 8 + 25 || memcmp(d, kSig, 8) != 0) return FPC_EFORMAT;
    if (be32(d + 8) != 13 || memcmp(d + 12, "IHDR", 4) != 0) return FPC_EFORMAT;
    const uint8_t* p = d + 16;
    h.w = be32(p); h.h = be32(p + 4); h.depth = p[8]; h.ctype = p[9];
    const int compression = p[10], filter = p[11], interlace = p[12];
    if (h.w == 0 || h.h == 0 || h.w > 65535 || h.h > 65535) return FPC_EFORMAT;
    if (compression != 0 || filter != 0 || interlace != 0) return FPC_EFORMAT;      // Adam7 files are not produced by the dataset tools
    if (h.depth != 8 && h.depth != 16) return FPC_EFORMAT;
    switch (h.ctype) {
        case 0: h.channels = 1; break;
        case 2: h.channels = 3; break;
        case 3: h.channels = 1; if (h.depth != 8) return FPC_EFORMAT; break;
        case 4: h.channels = 2; break;
        case 6: h.channels = 4; break;
        default: return FPC_EFORMAT;
    }
    h.bpp = h.channels * h.depth / 8;
    return FPC_OK;
}

}  // namespace
