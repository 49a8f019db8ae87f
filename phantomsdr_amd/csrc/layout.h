// layout.h - where a frame's tiled pyramid records (RecMap) and its spectrum bins (SpecLayout) sit in device memory: the two
// index maps every producer, every consumer and the create-time planner (createplan.h) share.  Host code and device code
// alike, no HIP include: quantize.h brings them to the kernels, tests/create_plan_table.cpp builds them with the host compiler.
#pragma once
#include <stddef.h>

#ifndef PSDR_HOST_DEVICE
#if defined(__HIPCC__)
#define PSDR_HOST_DEVICE __host__ __device__
#else
#define PSDR_HOST_DEVICE
#endif
#endif
#ifndef PSDR_FORCEINLINE
#if defined(__HIPCC__)
#define PSDR_FORCEINLINE __forceinline__
#else
#define PSDR_FORCEINLINE inline
#endif
#endif

namespace psdr {

inline int ilog2(size_t v) {
    int l = 0;
    while (((size_t)1 << l) < v) l++;
    return l;
}

// Record ORDER of the tiled pyramid records (quantize.h): tile-major.  The pass-2 work-group that owns rows
// c1base..c1base+T-1 writes the records of all its L output rows back to back (one contiguous stream of full lines
// instead of one 32-byte piece per 2 KiB: the piecewise order cost 16 % of pass 2).  Group
// g = c / CH of client-order bin c sits in record
//   pos(g) = tl * (rows * gpt) + row * gpt + k,  row = g / tpr, tl = (g % tpr) / gpt, k = g % gpt
// (tpr = M1/CH groups per output row, gpt = T/CH groups per tile and row, rows = M2).
struct RecMap {
    int l2tpr, l2gpt, l2rows;
    int pair;    // mode 2, quartets (2048-point rows): a column's LOW and HIGH quartet records are adjacent,
                 // pos = ((g * rows) + c2) * 2 + side - one 16-byte store writes both (round 5: [tile][side][column] like the
                 // octets, 8-byte record stores and 4-byte sum stores: +48 % store instructions against the IQ pass)
    int mapped;  // 0: identity (level-major producers: the three-pass real-input path)
                 // 1: IQ tile-major (above)
                 // 2: fused real-input pass 2 (k_fft_pass2_real): octet (or quartet: CH = the couples of a tile) o = k / CH
                 //    of bin k lives in row c2 = o / tpr (tpr = M1/CH groups per row); the lower half of a row's octets
                 //    belongs to tile g = o % tpr as its LOW octet, the upper half to tile
                 //    g = tpr - 1 - o % tpr as its HIGH octet: pos = (g * 2 + side) * rows + c2 (a tile's low octets,
                 //    then its high octets: a wave of the octet loop stores 64 adjacent records of ONE side)
    PSDR_HOST_DEVICE PSDR_FORCEINLINE size_t pos(size_t g) const {
        if (!mapped) return g;
        const size_t row = g >> l2tpr, gc = g & (((size_t)1 << l2tpr) - 1);
        if (mapped == 2) {
            const size_t tpr = (size_t)1 << l2tpr;
            const size_t side = gc >= (tpr >> 1) ? 1 : 0;
            const size_t tl = side ? tpr - 1 - gc : gc;
            if (pair) return (((tl << l2rows) + row) << 1) + side;
            return (((tl << 1) + side) << l2rows) + row;
        }
        const size_t tl = gc >> l2gpt, k = gc & (((size_t)1 << l2gpt) - 1);
        return (((tl << l2rows) + row) << l2gpt) + k;
    }
};

// Device layout of the spectrum of one frame: where bin c (IQ: client order, real: k order) sits.
// The passes whose row transform has 1024 points keep the spectrum in 128-byte LINES of 16 bins,
// TILE-MAJOR: a pass-2 work-group owns 16 rows c1 of the (c1, c2) output grid (bin = c1 + M1*c2) and
// writes the 1024 lines of its tile as one contiguous 128 KiB block (a wave's store instruction
// covers 8 adjacent lines).  In the natural order the same lines are 8 KiB apart and their
// neighbours belong to tiles written by other work-groups at other times; measured on the fused
// real path that cost twice the whole rest of the tile.
//   mode 0  natural order
//   mode 1  IQ, tiles of 16 adjacent rows: line (tl, c2) = tl * L + c2 = rows 16tl..16tl+15 of column c2
//   mode 2  fused real input (k_fft_pass2_real, fft_pass.h): line (g, c) = g * L + c =
//           [ rows 8g..8g+7 of column c | the mirror octet of tile g of column L-1-c ]; the mirror
//           octet of tile g is rows M1-8g-7..M1-8g ascending (g = 0: its last element is row M1/2
//           instead of "row M1").  The halves of a line are the two real-signal bins a
//           (row, mirror row) couple produces together.  With 2048-point rows (2^22-point real frames
//           split 1024 x 2048) a tile holds CP = 4 couples: lines of 8 bins, [ rows 4g..4g+3 | mirror
//           quartet ] (l2cp = 2; 3 for the octets above).
//   mode 3  IQ, BANDED (band sharding, psdr_set_band_layout): the columns are split into 2^(l2L - l2Lb) bands of
//           Lb = 2^l2Lb columns; band b owns one region of the buffer (band_stride bins apart) that holds ALL frames of
//           the batch, each frame as tiles of Lw = Lb + halo lines: line (tl, c2) of mode 1 is line tl * Lw + (c2 & (Lb-1))
//           of the frame's slot in region c2 >> l2Lb; lines Lb .. Lw-1 of a tile repeat the first columns of the NEXT
//           band (k_band_halo), so that a window that starts in a band can be read from that band's region alone.
//           One region is what one peer receives: no pack pass.
//   mode 4  one band region as received (psdr_demod_batch_from_band_region): columns c2_0 .. c2_0 + Lw - 1
// Consumers index through pos() (demodulation slices) or ask for k order (psdr_read_spectrum).
struct SpecLayout {
    int mode, m1, l2m1, L, l2L;
    int k0;  // mode 0 only: the buffer starts at bin k0 (a band of the spectrum, psdr_demod_batch_from_band)
    int l2Lb, Lw, c2_0;  // modes 3, 4
    size_t band_stride;  // mode 3
    int l2cp;            // mode 2: log2 of the couples per tile (3: lines of 16 bins; 2: lines of 8)
    PSDR_HOST_DEVICE PSDR_FORCEINLINE size_t pos(int k) const {
        if (!mode) return (size_t)(k - k0);
        const int c1 = k & (m1 - 1), c2 = k >> l2m1;
        if (mode == 1) return ((((size_t)(c1 >> 4) << l2L) + c2) << 4) + (c1 & 15);
        if (mode == 3)
            return (size_t)(c2 >> l2Lb) * band_stride + ((((size_t)(c1 >> 4) * Lw) + (c2 & ((1 << l2Lb) - 1))) << 4) + (c1 & 15);
        if (mode == 4) {
            int cl = c2 - c2_0;
            if (cl < 0) cl += L;  // the last band's halo is the spectrum's first column
            return ((((size_t)(c1 >> 4) * Lw) + cl) << 4) + (c1 & 15);
        }
        const int cp = 1 << l2cp;
        if (c1 < (m1 >> 1)) return ((((size_t)(c1 >> l2cp) << l2L) + c2) << (l2cp + 1)) + (c1 & (cp - 1));
        const int hp = c1 == (m1 >> 1) ? m1 - 1 : c1 - 1;  // rows above M1/2 shift down, M1/2 goes last
        const int g = (m1 - 1 - hp) >> l2cp;
        return ((((size_t)g << l2L) + (L - 1 - c2)) << (l2cp + 1)) + cp + (hp & (cp - 1));
    }
};

}  // namespace psdr
