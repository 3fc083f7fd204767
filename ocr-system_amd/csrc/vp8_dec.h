// Lossy WebP (VP8 key frame) decoding: every function the kernels of vp8dec.hip run, __host__ __device__, shared with a host build
// (tests/vp8_main.cpp) as webp_dec.h is.  The arithmetic is libwebp's, which Pillow calls; where RFC 6386's decoder differs, libwebp's
// rule stands: the inner edges of a macroblock are filtered when it is in 4x4 mode, or is not skipped and has a block with a non-zero
// coefficient (an unskipped 16x16-mode macroblock whose blocks are all zero is not filtered inside); Y2's AC step is step * 101581 >> 16.
//
// The boolean decoder: range in 128..255, `bits` bits of `value` not yet consumed below the 8 that the next decision compares.  A byte
// is loaded only when a decision needs bits the window does not hold, so "a read past the end of a partition" is exact: the decision
// needed a byte that the partition does not have.  Such a read sets `over`, feeds zeros, and the file ends with -1.  (libwebp pads a
// truncated token partition with zeros and returns a picture; a strict reader need not.)  Every intact stream of libwebp's encoder,
// which flushes whole bytes, stays inside.
// A partition that begins with the byte 0xFF is refused as well: the code value then lies outside the coder's interval (value >= range),
// which no encoder writes, and the excess sits in bits that libwebp's 64-bit window keeps and its 32-bit window (BITS = 24, as on 32-bit
// ARM) shifts out, so the two builds of libwebp decode such a partition differently.  With a first byte below 0xFF, value < range << bits
// holds from then on, and the 32-bit window here loses nothing.
//
// The coefficient bound.  libwebp's C transforms compute in int, its SSE2 / NEON ones in 16-bit lanes, so a stream that drives an
// intermediate of a transform out of 16 bits decodes differently per host CPU and is refused (-1).  With S the sum of |c| over the 16
// dequantised coefficients of a block (for a 16x16-mode macroblock the DC is the one the inverse WHT produced):
//   inverse DCT: a pass maps column sums of |.| at most to  k * sum + 2, k = 1 + 20091 / 65536 = 1.30657  (every partial sum of either
//   implementation is bounded by the same figure), so any value of either pass stays within  k^2 * S + 8 k + 6 = 1.70713 S + 16.5;
//   S <= VP8_MAX_BLOCK_SUM = 19000 keeps it below 32454.
//   inverse WHT: every partial sum is at most the sum S2 of |c| over the 16 Y2 values plus the rounder 3; S2 <= VP8_MAX_Y2_SUM = 32764
//   keeps it inside 16 bits, and its outputs (S2 + 3) >> 3 <= 4095 enter the block sums above.
// Each product level * step is formed in int and counted before it is stored, so the bound also keeps every stored value inside 16 bits.
#pragma once
#include <cstddef>
#include <cstdint>

#include "vp8_tables.h"

#if defined(__HIPCC__)
#define VP8_UNROLL _Pragma("unroll")
#else
#define VP8_UNROLL
#endif

constexpr int VP8_MAX_BLOCK_SUM = 19000;
constexpr int VP8_MAX_Y2_SUM = 32764;
constexpr int VP8_ERR_CORRUPT = -1;

// intra modes: the four 16x16 / chroma modes are the first four 4x4 modes
enum { VP8_DC = 0, VP8_TM = 1, VP8_VE = 2, VP8_HE = 3, VP8_RD = 4, VP8_VR = 5, VP8_LD = 6, VP8_VL = 7, VP8_HD_ = 8, VP8_HU = 9 };

struct Vp8Bool { uint32_t pos, end, value; int range, bits, over; };
struct Vp8Strength { uint8_t limit, ilevel, hev, pad; };   // limit 0: not filtered
struct Vp8Frame {
    int width, height, mbw, mbh;
    int update_map, use_skip, filter_type, parts;   // filter_type 0: none, 1: simple, 2: normal
    uint8_t seg_p[3], skip_p;
    uint32_t part_off[8], part_len[8];   // token partitions, byte offsets in the VP8 payload
    int16_t dq[4][6];                    // per segment: y1 dc, y1 ac, y2 dc, y2 ac, uv dc, uv ac
    Vp8Strength fs[4][2];                // per segment, 16x16 / 4x4 macroblock
    Vp8Bool modes;                       // the first partition's decoder after the frame header
    uint8_t coef_p[1056];                // [4 types][8 bands][3 contexts][11]
};
// one macroblock: flags = segment | skip << 2 | is 4x4 << 3; inner: the inner edges are filtered; nz: bit k = block k (16 Y, 4 U, 4 V)
// has a non-zero coefficient
struct Vp8Mb { uint8_t flags, ymode, uvmode, inner, sub[16]; uint32_t nz; };
constexpr int VP8_MB_COEFS = 24 * 16;

VP8_HD int vp8_clz(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __clz((int)v);
#else
    return __builtin_clz(v);
#endif
}

VP8_HD void vp8_bool_init(Vp8Bool& b, const uint8_t* s, uint32_t start, uint32_t end) {
    b.pos = start; b.end = end; b.value = 0; b.range = 255; b.bits = -8;
    b.over = (start < end && s[start] == 0xFF) ? 2 : 0;   // a code value outside the coder's interval, see above
}
VP8_HD int vp8_bit(Vp8Bool& b, const uint8_t* s, int prob) {
    if (b.bits < 0) {
        if (b.pos + 3 <= b.end) {
            b.value = (b.value << 24) | ((uint32_t)s[b.pos] << 16) | ((uint32_t)s[b.pos + 1] << 8) | s[b.pos + 2];
            b.pos += 3; b.bits += 24;
        } else if (b.pos < b.end) {
            b.value = (b.value << 8) | s[b.pos++]; b.bits += 8;
        } else {
            b.over |= 1; b.value <<= 8; b.bits += 8;
        }
    }
    const uint32_t split = ((uint32_t)(b.range - 1) * (uint32_t)prob) >> 8;
    const int bit = (b.value >> b.bits) > split;
    if (bit) { b.range -= (int)split + 1; b.value -= (split + 1) << b.bits; }
    else b.range = (int)split + 1;
    const int shift = 7 ^ (31 - vp8_clz((uint32_t)b.range));
    b.range <<= shift; b.bits -= shift;
    return bit;
}
VP8_HD uint32_t vp8_get(Vp8Bool& b, const uint8_t* s, int n) {
    uint32_t v = 0;
    while (n-- > 0) v |= (uint32_t)vp8_bit(b, s, 128) << n;
    return v;
}
VP8_HD int vp8_get_signed(Vp8Bool& b, const uint8_t* s, int n) {
    const int v = (int)vp8_get(b, s, n);
    return vp8_get(b, s, 1) ? -v : v;
}

// ---- stage 1: the mode walk over the first partition.  top: 4 * mbw bytes of scratch.  -> 0 or -1
VP8_HD int vp8_mode_walk(const Vp8Frame& F, const uint8_t* s, Vp8Mb* mbs, uint8_t* top) {
    Vp8Bool b = F.modes;
    for (int i = 0; i < 4 * F.mbw; ++i) top[i] = VP8_DC;
    for (int y = 0; y < F.mbh; ++y) {
        uint32_t left = 0;   // four modes, a byte each
        for (int x = 0; x < F.mbw; ++x) {
            Vp8Mb* m = mbs + (size_t)y * F.mbw + x;
            int seg = 0;
            if (F.update_map) seg = !vp8_bit(b, s, F.seg_p[0]) ? vp8_bit(b, s, F.seg_p[1]) : vp8_bit(b, s, F.seg_p[2]) + 2;
            const int skip = F.use_skip ? vp8_bit(b, s, F.skip_p) : 0;
            const int i4 = !vp8_bit(b, s, 145);
            m->flags = (uint8_t)(seg | (skip << 2) | (i4 << 3));
            if (!i4) {
                const int ym = vp8_bit(b, s, 156) ? (vp8_bit(b, s, 128) ? VP8_TM : VP8_HE) : (vp8_bit(b, s, 163) ? VP8_VE : VP8_DC);
                m->ymode = (uint8_t)ym;
                for (int k = 0; k < 16; ++k) m->sub[k] = (uint8_t)ym;
                for (int k = 0; k < 4; ++k) top[4 * x + k] = (uint8_t)ym;
                left = 0x01010101u * (uint32_t)ym;
            } else {
                m->ymode = 0;
                for (int by = 0; by < 4; ++by) {
                    int l = (int)((left >> (8 * by)) & 255u);
                    for (int bx = 0; bx < 4; ++bx) {
                        const int pr = (top[4 * x + bx] * 10 + l) * 9;
                        int i = vp8_bmode_tree(vp8_bit(b, s, vp8_bmode_proba(pr)));
                        while (i > 0) i = vp8_bmode_tree(2 * i + vp8_bit(b, s, vp8_bmode_proba(pr + i)));
                        l = -i;
                        top[4 * x + bx] = (uint8_t)l;
                        m->sub[4 * by + bx] = (uint8_t)l;
                    }
                    left = (left & ~(255u << (8 * by))) | ((uint32_t)l << (8 * by));
                }
            }
            m->uvmode = (uint8_t)(!vp8_bit(b, s, 142) ? VP8_DC : !vp8_bit(b, s, 114) ? VP8_VE : vp8_bit(b, s, 183) ? VP8_TM : VP8_HE);
            m->inner = 0; m->nz = 0;
        }
        if (b.over) return VP8_ERR_CORRUPT;
    }
    return 0;
}

// ---- stage 2: the token walk
VP8_HD int vp8_cat(int cat, int i) { return cat == 0 ? vp8_cat3(i) : cat == 1 ? vp8_cat4(i) : cat == 2 ? vp8_cat5(i) : vp8_cat6(i); }

// one block's tokens from position n on -> the position after the last non-zero coefficient; dequantised values to out (zig-zag undone),
// *sum += their absolute values.  p: the type's probabilities [8 bands][3][11]
VP8_HD int vp8_coeffs(Vp8Bool& b, const uint8_t* s, const uint8_t* type_p, int ctx, int dc_q, int ac_q, int n, int16_t* out, int* sum) {
    const uint8_t* p = type_p + (vp8_bands(n) * 3 + ctx) * 11;
    for (; n < 16; ++n) {
        if (!vp8_bit(b, s, p[0])) return n;
        while (!vp8_bit(b, s, p[1])) {
            p = type_p + vp8_bands(++n) * 33;
            if (n == 16) return 16;
        }
        const uint8_t* next = type_p + vp8_bands(n + 1) * 33;
        int v;
        if (!vp8_bit(b, s, p[2])) { v = 1; p = next + 11; }
        else {
            if (!vp8_bit(b, s, p[3])) v = !vp8_bit(b, s, p[4]) ? 2 : 3 + vp8_bit(b, s, p[5]);
            else if (!vp8_bit(b, s, p[6])) {
                if (!vp8_bit(b, s, p[7])) v = 5 + vp8_bit(b, s, 159);
                else { v = 7 + 2 * vp8_bit(b, s, 165); v += vp8_bit(b, s, 145); }
            } else {
                const int bit1 = vp8_bit(b, s, p[8]), bit0 = vp8_bit(b, s, p[9 + bit1]), cat = 2 * bit1 + bit0;
                v = 0;
                for (int k = 0; vp8_cat(cat, k); ++k) v += v + vp8_bit(b, s, vp8_cat(cat, k));
                v += 3 + (8 << cat);
            }
            p = next + 22;
        }
        const int c = v * (n > 0 ? ac_q : dc_q);
        *sum += c;
        out[vp8_zigzag(n)] = (int16_t)(vp8_bit(b, s, 128) ? -c : c);
    }
    return 16;
}

// the inverse WHT of y2[16] into the DC of the 16 luma blocks of c
VP8_HD void vp8_wht(const int16_t* y2, int16_t* c) {
    int t[16];
    VP8_UNROLL
    for (int i = 0; i < 4; ++i) {
        const int a0 = y2[i] + y2[12 + i], a1 = y2[4 + i] + y2[8 + i], a2 = y2[4 + i] - y2[8 + i], a3 = y2[i] - y2[12 + i];
        t[i] = a0 + a1; t[8 + i] = a0 - a1; t[4 + i] = a3 + a2; t[12 + i] = a3 - a2;
    }
    VP8_UNROLL
    for (int i = 0; i < 4; ++i) {
        const int dc = t[4 * i] + 3, a0 = dc + t[4 * i + 3], a1 = t[4 * i + 1] + t[4 * i + 2], a2 = t[4 * i + 1] - t[4 * i + 2], a3 = dc - t[4 * i + 3];
        c[(4 * i) * 16] = (int16_t)((a0 + a1) >> 3); c[(4 * i + 1) * 16] = (int16_t)((a3 + a2) >> 3);
        c[(4 * i + 2) * 16] = (int16_t)((a0 - a1) >> 3); c[(4 * i + 3) * 16] = (int16_t)((a3 - a2) >> 3);
    }
}

// The token partitions of a file, macroblock row r from partition r & (parts - 1).  coefs: [mb][24][16], cleared before; tnz, tdc: mbw
// bytes of scratch each; pb: parts decoder states of scratch; y2: 16 values of scratch.  -> 0 or -1
VP8_HD int vp8_token_walk(const Vp8Frame& F, const uint8_t* s, Vp8Mb* mbs, int16_t* coefs, uint8_t* tnz, uint8_t* tdc, Vp8Bool* pb, int16_t* y2) {
    for (int k = 0; k < F.parts; ++k) vp8_bool_init(pb[k], s, F.part_off[k], F.part_off[k] + F.part_len[k]);
    for (int x = 0; x < F.mbw; ++x) tnz[x] = tdc[x] = 0;
    int bad = 0;
    for (int k = 0; k < F.parts && k < F.mbh; ++k) bad |= pb[k].over;   // (a partition no row reads is not judged)
    if (bad) return VP8_ERR_CORRUPT;
    for (int y = 0; y < F.mbh; ++y) {
        Vp8Bool b = pb[y & (F.parts - 1)];
        int lnz = 0, ldc = 0;
        for (int x = 0; x < F.mbw; ++x) {
            Vp8Mb* m = mbs + (size_t)y * F.mbw + x;
            const int flags = m->flags, i4 = (flags >> 3) & 1, skip = F.use_skip ? (flags >> 2) & 1 : 0;
            m->inner = (uint8_t)i4;   // (libwebp: 4x4 mode, or a macroblock that is not skipped and has a non-zero block)
            if (skip) {
                tnz[x] = 0; lnz = 0;
                if (!i4) { tdc[x] = 0; ldc = 0; }
                continue;
            }
            const int16_t* q = F.dq[flags & 3];
            int16_t* c = coefs + ((size_t)y * F.mbw + x) * VP8_MB_COEFS;
            uint32_t nzmask = 0;
            int first = 0;
            const uint8_t* yp = F.coef_p + 3 * 264;
            if (!i4) {
                for (int k = 0; k < 16; ++k) y2[k] = 0;
                int s2 = 0;
                const int nz = vp8_coeffs(b, s, F.coef_p + 264, tdc[x] + ldc, q[2], q[3], 0, y2, &s2);
                tdc[x] = (uint8_t)(nz > 0); ldc = nz > 0;
                bad |= s2 > VP8_MAX_Y2_SUM;
                if (nz > 0) vp8_wht(y2, c);   // (with the DC alone this is libwebp's (dc + 3) >> 3 in every block)
                first = 1; yp = F.coef_p;
            }
            int t = tnz[x] & 15, l = lnz & 15;
            for (int by = 0; by < 4; ++by) {
                int lb = l & 1;
                for (int bx = 0; bx < 4; ++bx) {
                    int16_t* blk = c + (4 * by + bx) * 16;
                    const int dc = blk[0];
                    int sum = dc < 0 ? -dc : dc;
                    const int nz = vp8_coeffs(b, s, yp, lb + (t & 1), q[0], q[1], first, blk, &sum);
                    bad |= sum > VP8_MAX_BLOCK_SUM;
                    lb = nz > first;
                    t = (t >> 1) | (lb << 7);
                    if (nz > 1 || blk[0] != 0) nzmask |= 1u << (4 * by + bx);   // (libwebp's non-zero code of the block)
                }
                t >>= 4;
                l = (l >> 1) | (lb << 7);
            }
            int out_t = t, out_l = l >> 4;
            for (int ch = 0; ch < 4; ch += 2) {
                t = tnz[x] >> (4 + ch); l = lnz >> (4 + ch);
                for (int by = 0; by < 2; ++by) {
                    int lb = l & 1;
                    for (int bx = 0; bx < 2; ++bx) {
                        const int k = 16 + 2 * ch + 2 * by + bx;
                        int sum = 0;
                        const int nz = vp8_coeffs(b, s, F.coef_p + 2 * 264, lb + (t & 1), q[4], q[5], 0, c + k * 16, &sum);
                        bad |= sum > VP8_MAX_BLOCK_SUM;
                        lb = nz > 0;
                        t = (t >> 1) | (lb << 3);
                        if (nz > 1 || c[k * 16] != 0) nzmask |= 1u << k;
                    }
                    t >>= 2;
                    l = (l >> 1) | (lb << 5);
                }
                out_t |= (t << 4) << ch;
                out_l |= (l & 0xf0) << ch;
            }
            tnz[x] = (uint8_t)out_t; lnz = out_l;
            m->nz = nzmask;
            m->inner = (uint8_t)(i4 | (nzmask != 0));
        }
        if (b.over || bad) return VP8_ERR_CORRUPT;
        pb[y & (F.parts - 1)] = b;
    }
    return 0;
}

// ---- stage 3: reconstruction into the unfiltered frame (planes padded to whole macroblocks)
VP8_HD int vp8_clip8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
// the frame with its borders: 127 above, 129 to the left (and above-left below row 0)
VP8_HD int vp8_px(const uint8_t* P, int stride, int x, int y) { return y < 0 ? 127 : x < 0 ? 129 : P[(size_t)y * stride + x]; }
VP8_HD int vp8_avg3(int a, int b, int c) { return (a + 2 * b + c + 2) >> 2; }
VP8_HD int vp8_avg2(int a, int b) { return (a + b + 1) >> 1; }
VP8_HD int vp8_mul1(int a) { return ((a * 20091) >> 16) + a; }
VP8_HD int vp8_mul2(int a) { return (a * 35468) >> 16; }

// p[16] (row-major prediction) + the inverse DCT of c (or nothing) -> the 4x4 block at (x0, y0)
VP8_HD void vp8_add_store(uint8_t* P, int stride, int x0, int y0, const int* p, const int16_t* c) {
    int r[16];
    if (c) {
        int t[16];
    VP8_UNROLL
        for (int i = 0; i < 4; ++i) {
            const int a = c[i] + c[8 + i], bb = c[i] - c[8 + i];
            const int cc = vp8_mul2(c[4 + i]) - vp8_mul1(c[12 + i]), d = vp8_mul1(c[4 + i]) + vp8_mul2(c[12 + i]);
            t[4 * i] = a + d; t[4 * i + 1] = bb + cc; t[4 * i + 2] = bb - cc; t[4 * i + 3] = a - d;
        }
    VP8_UNROLL
        for (int i = 0; i < 4; ++i) {
            const int dc = t[i] + 4, a = dc + t[8 + i], bb = dc - t[8 + i];
            const int cc = vp8_mul2(t[4 + i]) - vp8_mul1(t[12 + i]), d = vp8_mul1(t[4 + i]) + vp8_mul2(t[12 + i]);
            r[4 * i] = (a + d) >> 3; r[4 * i + 1] = (bb + cc) >> 3; r[4 * i + 2] = (bb - cc) >> 3; r[4 * i + 3] = (a - d) >> 3;
        }
    } else {
    VP8_UNROLL
        for (int i = 0; i < 16; ++i) r[i] = 0;
    }
    VP8_UNROLL
    for (int j = 0; j < 4; ++j) {
        const uint32_t w = (uint32_t)vp8_clip8(p[4 * j] + r[4 * j]) | ((uint32_t)vp8_clip8(p[4 * j + 1] + r[4 * j + 1]) << 8) |
                           ((uint32_t)vp8_clip8(p[4 * j + 2] + r[4 * j + 2]) << 16) | ((uint32_t)vp8_clip8(p[4 * j + 3] + r[4 * j + 3]) << 24);
        *(uint32_t*)(P + (size_t)(y0 + j) * stride + x0) = w;   // (x0 and the stride are multiples of 4)
    }
}

// a whole-macroblock mode (16x16 luma: n = 16, chroma: n = 8) for the 4x4 block at (bx, by) of the macroblock at (mx, my) pixels
VP8_HD void vp8_predict_mb(const uint8_t* P, int stride, int mx, int my, int n, int mode, int bx, int by, int* p) {
    const int x0 = mx + 4 * bx, y0 = my + 4 * by;
    if (mode == VP8_DC) {
        int dc = 128;
        const int sh = n == 16 ? 4 : 3;
        if (mx > 0 || my > 0) {
            int sum = 0;
            if (my > 0) for (int i = 0; i < n; ++i) sum += P[(size_t)(my - 1) * stride + mx + i];
            if (mx > 0) for (int i = 0; i < n; ++i) sum += P[(size_t)(my + i) * stride + mx - 1];
            dc = (mx > 0 && my > 0) ? (sum + n) >> (sh + 1) : (sum + (n >> 1)) >> sh;
        }
    VP8_UNROLL
        for (int i = 0; i < 16; ++i) p[i] = dc;
    } else if (mode == VP8_VE) {
    VP8_UNROLL
        for (int i = 0; i < 16; ++i) p[i] = vp8_px(P, stride, x0 + (i & 3), my - 1);
    } else if (mode == VP8_HE) {
    VP8_UNROLL
        for (int i = 0; i < 16; ++i) p[i] = vp8_px(P, stride, mx - 1, y0 + (i >> 2));
    } else {
        const int tl = vp8_px(P, stride, mx - 1, my - 1);
    VP8_UNROLL
        for (int i = 0; i < 16; ++i) p[i] = vp8_clip8(vp8_px(P, stride, x0 + (i & 3), my - 1) + vp8_px(P, stride, mx - 1, y0 + (i >> 2)) - tl);
    }
}

// a 4x4 sub-mode for the luma block (bx, by) of the macroblock at (mx, my) pixels; last: the macroblock is its row's last
VP8_HD void vp8_predict_sub(const uint8_t* P, int stride, int mx, int my, int last, int mode, int bx, int by, int* p) {
    const int x0 = mx + 4 * bx, y0 = my + 4 * by;
    // e: the edge from bottom-left over the corner to top-right: L K J I X A B C D E F G H
    int e[13];
    VP8_UNROLL
    for (int i = 0; i < 4; ++i) e[3 - i] = vp8_px(P, stride, x0 - 1, y0 + i);
    e[4] = vp8_px(P, stride, x0 - 1, y0 - 1);
    VP8_UNROLL
    for (int i = 0; i < 4; ++i) e[5 + i] = vp8_px(P, stride, x0 + i, y0 - 1);
    {   // above-right: inside the macroblock for the left three columns below row 0, else the macroblock row above
        const int ty = (by == 0 || bx == 3) ? my - 1 : y0 - 1;
    VP8_UNROLL
        for (int i = 0; i < 4; ++i) {
            const int tx = (bx == 3 && last) ? mx + 15 : x0 + 4 + i;
            e[9 + i] = vp8_px(P, stride, tx, ty);
        }
    }
    const int L = e[0], K = e[1], J = e[2], I = e[3], X = e[4], A = e[5], B = e[6], C = e[7], D = e[8], E = e[9], F = e[10], G = e[11], H = e[12];
#define VP8_DST(x, y) p[(y) * 4 + (x)]
    switch (mode) {
        case VP8_DC: {
            const int dc = (A + B + C + D + I + J + K + L + 4) >> 3;
    VP8_UNROLL
            for (int i = 0; i < 16; ++i) p[i] = dc;
        } break;
        case VP8_TM:
    VP8_UNROLL
            for (int i = 0; i < 16; ++i) p[i] = vp8_clip8(e[5 + (i & 3)] + e[3 - (i >> 2)] - X);
            break;
        case VP8_VE: {
            const int v0 = vp8_avg3(X, A, B), v1 = vp8_avg3(A, B, C), v2 = vp8_avg3(B, C, D), v3 = vp8_avg3(C, D, E);
    VP8_UNROLL
            for (int j = 0; j < 4; ++j) { p[4 * j] = v0; p[4 * j + 1] = v1; p[4 * j + 2] = v2; p[4 * j + 3] = v3; }
        } break;
        case VP8_HE: {
            const int h0 = vp8_avg3(X, I, J), h1 = vp8_avg3(I, J, K), h2 = vp8_avg3(J, K, L), h3 = vp8_avg3(K, L, L);
    VP8_UNROLL
            for (int i = 0; i < 4; ++i) { p[i] = h0; p[4 + i] = h1; p[8 + i] = h2; p[12 + i] = h3; }
        } break;
        case VP8_RD:
    VP8_UNROLL
            for (int i = 0; i < 16; ++i) { const int k = 3 - (i >> 2) + (i & 3); p[i] = vp8_avg3(e[k], e[k + 1], e[k + 2]); }
            break;
        case VP8_LD:
    VP8_UNROLL
            for (int i = 0; i < 16; ++i) { const int k = (i >> 2) + (i & 3); p[i] = vp8_avg3(e[5 + k], e[6 + k], e[k + 7 > 12 ? 12 : k + 7]); }
            break;
        case VP8_VR:
            VP8_DST(0, 0) = VP8_DST(1, 2) = vp8_avg2(X, A); VP8_DST(1, 0) = VP8_DST(2, 2) = vp8_avg2(A, B);
            VP8_DST(2, 0) = VP8_DST(3, 2) = vp8_avg2(B, C); VP8_DST(3, 0) = vp8_avg2(C, D);
            VP8_DST(0, 3) = vp8_avg3(K, J, I); VP8_DST(0, 2) = vp8_avg3(J, I, X);
            VP8_DST(0, 1) = VP8_DST(1, 3) = vp8_avg3(I, X, A); VP8_DST(1, 1) = VP8_DST(2, 3) = vp8_avg3(X, A, B);
            VP8_DST(2, 1) = VP8_DST(3, 3) = vp8_avg3(A, B, C); VP8_DST(3, 1) = vp8_avg3(B, C, D);
            break;
        case VP8_VL:
            VP8_DST(0, 0) = vp8_avg2(A, B); VP8_DST(1, 0) = VP8_DST(0, 2) = vp8_avg2(B, C);
            VP8_DST(2, 0) = VP8_DST(1, 2) = vp8_avg2(C, D); VP8_DST(3, 0) = VP8_DST(2, 2) = vp8_avg2(D, E);
            VP8_DST(0, 1) = vp8_avg3(A, B, C); VP8_DST(1, 1) = VP8_DST(0, 3) = vp8_avg3(B, C, D);
            VP8_DST(2, 1) = VP8_DST(1, 3) = vp8_avg3(C, D, E); VP8_DST(3, 1) = VP8_DST(2, 3) = vp8_avg3(D, E, F);
            VP8_DST(3, 2) = vp8_avg3(E, F, G); VP8_DST(3, 3) = vp8_avg3(F, G, H);
            break;
        case VP8_HU:
            VP8_DST(0, 0) = vp8_avg2(I, J); VP8_DST(2, 0) = VP8_DST(0, 1) = vp8_avg2(J, K); VP8_DST(2, 1) = VP8_DST(0, 2) = vp8_avg2(K, L);
            VP8_DST(1, 0) = vp8_avg3(I, J, K); VP8_DST(3, 0) = VP8_DST(1, 1) = vp8_avg3(J, K, L); VP8_DST(3, 1) = VP8_DST(1, 2) = vp8_avg3(K, L, L);
            VP8_DST(3, 2) = VP8_DST(2, 2) = VP8_DST(0, 3) = VP8_DST(1, 3) = VP8_DST(2, 3) = VP8_DST(3, 3) = L;
            break;
        default:   // VP8_HD_
            VP8_DST(0, 0) = VP8_DST(2, 1) = vp8_avg2(I, X); VP8_DST(0, 1) = VP8_DST(2, 2) = vp8_avg2(J, I);
            VP8_DST(0, 2) = VP8_DST(2, 3) = vp8_avg2(K, J); VP8_DST(0, 3) = vp8_avg2(L, K);
            VP8_DST(3, 0) = vp8_avg3(A, B, C); VP8_DST(2, 0) = vp8_avg3(X, A, B);
            VP8_DST(1, 0) = VP8_DST(3, 1) = vp8_avg3(I, X, A); VP8_DST(1, 1) = VP8_DST(3, 2) = vp8_avg3(J, I, X);
            VP8_DST(1, 2) = VP8_DST(3, 3) = vp8_avg3(K, J, I); VP8_DST(1, 3) = vp8_avg3(L, K, J);
            break;
    }
#undef VP8_DST
}

// luma block k = 4 by + bx of macroblock (mbx, mby)
VP8_HD void vp8_recon_luma(const Vp8Frame& F, const Vp8Mb& m, const int16_t* c, int mbx, int mby, int k, uint8_t* Y, int ys) {
    int p[16];
    const int bx = k & 3, by = k >> 2;
    if ((m.flags >> 3) & 1) vp8_predict_sub(Y, ys, 16 * mbx, 16 * mby, mbx == F.mbw - 1, m.sub[k], bx, by, p);
    else vp8_predict_mb(Y, ys, 16 * mbx, 16 * mby, 16, m.ymode, bx, by, p);
    vp8_add_store(Y, ys, 16 * mbx + 4 * bx, 16 * mby + 4 * by, p, (m.nz >> k) & 1 ? c + k * 16 : nullptr);
}
// chroma block k = 0..3 of U, 4..7 of V
VP8_HD void vp8_recon_chroma(const Vp8Mb& m, const int16_t* c, int mbx, int mby, int k, uint8_t* U, uint8_t* V, int uvs) {
    int p[16];
    uint8_t* P = k < 4 ? U : V;
    const int bx = k & 1, by = (k >> 1) & 1;
    vp8_predict_mb(P, uvs, 8 * mbx, 8 * mby, 8, m.uvmode, bx, by, p);
    vp8_add_store(P, uvs, 8 * mbx + 4 * bx, 8 * mby + 4 * by, p, (m.nz >> (16 + k)) & 1 ? c + (16 + k) * 16 : nullptr);
}

// ---- stage 4: the loop filter, one line of an edge at a time.  p: the first pixel after the edge; step: across the edge
VP8_HD int vp8_abs(int v) { return v < 0 ? -v : v; }
VP8_HD int vp8_sclip1(int v) { return v < -128 ? -128 : v > 127 ? 127 : v; }
VP8_HD int vp8_sclip2(int v) { return v < -16 ? -16 : v > 15 ? 15 : v; }
VP8_HD void vp8_do2(uint8_t* p, ptrdiff_t s) {
    const int p1 = p[-2 * s], p0 = p[-s], q0 = p[0], q1 = p[s];
    const int a = 3 * (q0 - p0) + vp8_sclip1(p1 - q1), a1 = vp8_sclip2((a + 4) >> 3), a2 = vp8_sclip2((a + 3) >> 3);
    p[-s] = (uint8_t)vp8_clip8(p0 + a2); p[0] = (uint8_t)vp8_clip8(q0 - a1);
}
VP8_HD void vp8_do4(uint8_t* p, ptrdiff_t s) {
    const int p1 = p[-2 * s], p0 = p[-s], q0 = p[0], q1 = p[s];
    const int a = 3 * (q0 - p0), a1 = vp8_sclip2((a + 4) >> 3), a2 = vp8_sclip2((a + 3) >> 3), a3 = (a1 + 1) >> 1;
    p[-2 * s] = (uint8_t)vp8_clip8(p1 + a3); p[-s] = (uint8_t)vp8_clip8(p0 + a2);
    p[0] = (uint8_t)vp8_clip8(q0 - a1); p[s] = (uint8_t)vp8_clip8(q1 - a3);
}
VP8_HD void vp8_do6(uint8_t* p, ptrdiff_t s) {
    const int p2 = p[-3 * s], p1 = p[-2 * s], p0 = p[-s], q0 = p[0], q1 = p[s], q2 = p[2 * s];
    const int a = vp8_sclip1(3 * (q0 - p0) + vp8_sclip1(p1 - q1));
    const int a1 = (27 * a + 63) >> 7, a2 = (18 * a + 63) >> 7, a3 = (9 * a + 63) >> 7;
    p[-3 * s] = (uint8_t)vp8_clip8(p2 + a3); p[-2 * s] = (uint8_t)vp8_clip8(p1 + a2); p[-s] = (uint8_t)vp8_clip8(p0 + a1);
    p[0] = (uint8_t)vp8_clip8(q0 - a1); p[s] = (uint8_t)vp8_clip8(q1 - a2); p[2 * s] = (uint8_t)vp8_clip8(q2 - a3);
}
VP8_HD bool vp8_needs(const uint8_t* p, ptrdiff_t s, int t2) { return 4 * vp8_abs(p[-s] - p[0]) + vp8_abs(p[-2 * s] - p[s]) <= t2; }
VP8_HD bool vp8_needs2(const uint8_t* p, ptrdiff_t s, int t2, int it) {
    const int p3 = p[-4 * s], p2 = p[-3 * s], p1 = p[-2 * s], p0 = p[-s], q0 = p[0], q1 = p[s], q2 = p[2 * s], q3 = p[3 * s];
    if (4 * vp8_abs(p0 - q0) + vp8_abs(p1 - q1) > t2) return false;
    return vp8_abs(p3 - p2) <= it && vp8_abs(p2 - p1) <= it && vp8_abs(p1 - p0) <= it && vp8_abs(q3 - q2) <= it && vp8_abs(q2 - q1) <= it &&
           vp8_abs(q1 - q0) <= it;
}
VP8_HD bool vp8_hev(const uint8_t* p, ptrdiff_t s, int t) { return vp8_abs(p[-2 * s] - p[-s]) > t || vp8_abs(p[s] - p[0]) > t; }
VP8_HD void vp8_simple_line(uint8_t* p, ptrdiff_t s, int thresh) {
    if (vp8_needs(p, s, 2 * thresh + 1)) vp8_do2(p, s);
}
VP8_HD void vp8_edge_line(uint8_t* p, ptrdiff_t s, int thresh, int it, int hev, bool inner) {
    if (!vp8_needs2(p, s, 2 * thresh + 1, it)) return;
    if (vp8_hev(p, s, hev)) vp8_do2(p, s);
    else if (inner) vp8_do4(p, s);
    else vp8_do6(p, s);
}

// One of the four steps of a macroblock's filtering (0: left edge, 1: inner vertical edges, 2: top edge, 3: inner horizontal edges) for
// line `lane` of 16: luma line `lane`, and U line `lane` (lanes 0..7) or V line `lane - 8`.  The steps of a macroblock follow each other,
// and the macroblocks in raster order or any order that keeps (x - 1, y), (x, y - 1) and (x + 1, y - 1) before (x, y).
VP8_HD void vp8_filter_step(const Vp8Frame& F, const Vp8Mb& m, int mbx, int mby, int step, int lane, uint8_t* Y, uint8_t* U, uint8_t* V, int ys,
                            int uvs) {
    const Vp8Strength fs = F.fs[m.flags & 3][(m.flags >> 3) & 1];
    const int limit = fs.limit;
    if (limit == 0) return;
    const bool edge = !(step & 1);
    if (edge ? (step == 0 ? mbx == 0 : mby == 0) : !m.inner) return;
    const bool vertical = step < 2;   // a vertical edge: lines are rows, the filter runs along x
    const int thresh = edge ? limit + 4 : limit;
    {
        uint8_t* p = Y + (size_t)(16 * mby) * ys + 16 * mbx + (vertical ? (size_t)lane * ys : (size_t)lane);
        const ptrdiff_t s = vertical ? 1 : ys;
        if (F.filter_type == 1) {
            if (edge) vp8_simple_line(p, s, thresh);
            else for (int k = 1; k < 4; ++k) vp8_simple_line(p + 4 * k * s, s, thresh);
        } else {
            if (edge) vp8_edge_line(p, s, thresh, fs.ilevel, fs.hev, false);
            else for (int k = 1; k < 4; ++k) vp8_edge_line(p + 4 * k * s, s, thresh, fs.ilevel, fs.hev, true);
        }
    }
    if (F.filter_type == 2) {
        uint8_t* C = lane < 8 ? U : V;
        const int ln = lane & 7;
        uint8_t* p = C + (size_t)(8 * mby) * uvs + 8 * mbx + (vertical ? (size_t)ln * uvs : (size_t)ln);
        const ptrdiff_t s = vertical ? 1 : uvs;
        if (edge) vp8_edge_line(p, s, thresh, fs.ilevel, fs.hev, false);
        else vp8_edge_line(p + 4 * s, s, thresh, fs.ilevel, fs.hev, true);
    }
}

// ---- stage 5: "fancy" chroma up-sampling, libwebp's 14-bit YUV -> RGB, cropped
VP8_HD int vp8_rgb_clip(int v) { return (v & ~16383) == 0 ? v >> 6 : v < 0 ? 0 : 255; }
VP8_HD void vp8_rgb_px(const uint8_t* Y, const uint8_t* U, const uint8_t* V, int ys, int uvs, int w, int h, int x, int y, uint8_t* rgb) {
    const int cw = (w + 1) >> 1, ch = (h + 1) >> 1;
    const int cx = x >> 1, cy = y >> 1;
    int nx = (x & 1) ? cx + 1 : cx - 1, ny = (y & 1) ? cy + 1 : cy - 1;
    nx = nx < 0 ? 0 : nx >= cw ? cw - 1 : nx;
    ny = ny < 0 ? 0 : ny >= ch ? ch - 1 : ny;
    const size_t a = (size_t)cy * uvs + cx, b = (size_t)cy * uvs + nx, c = (size_t)ny * uvs + cx, d = (size_t)ny * uvs + nx;
    const int u = (9 * U[a] + 3 * U[b] + 3 * U[c] + U[d] + 8) >> 4, v = (9 * V[a] + 3 * V[b] + 3 * V[c] + V[d] + 8) >> 4;
    const int yy = (Y[(size_t)y * ys + x] * 19077) >> 8;
    rgb[0] = (uint8_t)vp8_rgb_clip(yy + ((v * 26149) >> 8) - 14234);
    rgb[1] = (uint8_t)vp8_rgb_clip(yy - ((u * 6419) >> 8) - ((v * 13320) >> 8) + 8708);
    rgb[2] = (uint8_t)vp8_rgb_clip(yy + ((u * 33050) >> 8) - 17685);
}
