// JBIG2 generic-region decoding as plain functions: the decision walk of one row of an arithmetic-coded region (T.88 6.2.5) over
// contexts of one byte each and rows of packed words.  jbig2.hip runs them on the device (contexts and live rows in LDS, lane 0 of the
// region's wave walks); tests/jbig2_main.cpp compiles the same text for the host, where the sanitizers can see it.
// The arithmetic decoder is JPEG 2000's (T.88 Annex E = T.800 Annex C): the registers, byte-in, initialisation and the state table of
// jp2_t1.h / jp2_tables.h.  Only the place of the context differs: a byte in memory here, a byte of a register there.
#pragma once
#include <cstdint>

#include "jp2_t1.h"

// Rows are packed 32 pixels a word, pixel x at bit x & 31 of word x >> 5 (the fax decoder's line words); a row of W pixels has
// jb2_row_words(W) words, the bits from W on are 0, so the templates read 0 right of the region without a test.  (constexpr: for
// host and device alike)
constexpr int jb2_plane_words(int W) { return (W + 31) >> 5; }
constexpr int jb2_row_words(int W) { return jb2_plane_words(W) + 2; }

constexpr int jb2_context_bits(int tmpl) { return tmpl == 0 ? 16 : tmpl == 1 ? 13 : 10; }
constexpr int jb2_sltp_context(int tmpl) { return tmpl == 0 ? 0x9B25 : tmpl == 1 ? 0x0795 : tmpl == 2 ? 0x00E5 : 0x0195; }

// one decision in the context byte *cx (state << 1 | MPS); mq: jp2_mq_states
JP2_HD inline int jb2_mq_decode(Jp2Mq& m, const uint32_t* mq, uint8_t* cx) {
    const uint32_t s = *cx, st = mq[s >> 1], qe = st & 0xFFFF;
    int bit = (int)(s & 1);
    m.a -= qe;
    bool lps;
    if ((m.c >> 16) < qe) {
        lps = m.a >= qe;
        m.a = qe;
    } else {
        m.c -= qe << 16;
        if (m.a & 0x8000) return bit;
        lps = m.a < qe;
    }
    if (lps) {
        bit ^= 1;
        *cx = (uint8_t)((((st >> 22) & 63) << 1) | ((s & 1) ^ (st >> 28)));
    } else {
        *cx = (uint8_t)((((st >> 16) & 63) << 1) | (s & 1));
    }
    do {
        if (m.ct == 0) jp2_mq_bytein(m);
        m.a <<= 1; m.c <<= 1; --m.ct;
    } while (!(m.a & 0x8000));
    return bit;
}

// The pixels of the region above row y, for the templates.  r0: the row being decoded, r1 / r2: rows y - 1 and y - 2 (all zero above
// the region); plane: the finished rows of the region, `pw` words a row, for an adaptive pixel further up.
struct Jb2Rows {
    uint32_t* r0;
    const uint32_t* r1;
    const uint32_t* r2;
    const uint32_t* plane;
    int pw, W, y;
};

JP2_HD inline unsigned jb2_pixel(const Jb2Rows& R, int x, int dy) {
    if (x < 0 || x >= R.W || R.y + dy < 0) return 0;
    const uint32_t* row = dy == 0 ? R.r0 : dy == -1 ? R.r1 : dy == -2 ? R.r2 : R.plane + (size_t)(R.y + dy) * R.pw;
    return (row[x >> 5] >> (x & 31)) & 1u;
}

// The four templates (positions relative to the pixel (x, y); a pixel outside the region reads 0):
//   template  pixels  row y - 2        row y - 1        row y            nominal AT pixels
//   0         16      x - 1 .. x + 1   x - 2 .. x + 2   x - 4 .. x - 1   A1 (3, -1), A2 (-3, -1), A3 (2, -2), A4 (-2, -2)
//   1         13      x - 1 .. x + 2   x - 2 .. x + 2   x - 3 .. x - 1   A1 (3, -1)
//   2         10      x - 1 .. x + 1   x - 2 .. x + 1   x - 2, x - 1     A1 (2, -1)
//   3         10      none             x - 3 .. x + 1   x - 4 .. x - 1   A1 (2, -1)
// Context bit order, from bit 0 upwards: the current row from x - 1 leftwards; A1; row y - 1 from right to left; for template 0 A2
// and A3; row y - 2 from right to left; for template 0 A4.  An AT pixel may lie at y in -128 .. 0 (at y = 0 with x < 0) and x in
// -128 .. 127.  With typical prediction each row is preceded by one SLTP decision in the context jb2_sltp_context gives; LTP ^= SLTP,
// and a typical row copies the row above (row 0 copies zeros).
// jb2_shape: the template's fixed pixels in context bit order, without the AT slots: per template {pixels of row y, of row y - 1
// (rightmost offset first), of row y - 2 (the same)}
struct Jb2Shape { int ncur, n1, right1, n2, right2; };
JP2_HD inline Jb2Shape jb2_shape(int tmpl) {
    return tmpl == 0 ? Jb2Shape{4, 5, 2, 3, 1} : tmpl == 1 ? Jb2Shape{3, 5, 2, 4, 2} : tmpl == 2 ? Jb2Shape{2, 4, 1, 3, 1} : Jb2Shape{4, 5, 1, 0, 0};
}

// the context of pixel x from its definition: current row from x - 1 leftwards, A1, row y - 1 right to left, (T0: A2, A3,) row y - 2
// right to left, (T0: A4)
JP2_HD inline unsigned jb2_context(const Jb2Rows& R, int x, int tmpl, const int8_t* at) {
    const Jb2Shape s = jb2_shape(tmpl);
    unsigned cx = 0;
    int b = 0;
    for (int k = 1; k <= s.ncur; ++k) cx |= jb2_pixel(R, x - k, 0) << b++;
    cx |= jb2_pixel(R, x + at[0], at[1]) << b++;
    for (int k = 0; k < s.n1; ++k) cx |= jb2_pixel(R, x + s.right1 - k, -1) << b++;
    if (tmpl == 0) {
        cx |= jb2_pixel(R, x + at[2], at[3]) << b++;
        cx |= jb2_pixel(R, x + at[4], at[5]) << b++;
    }
    for (int k = 0; k < s.n2; ++k) cx |= jb2_pixel(R, x + s.right2 - k, -2) << b++;
    if (tmpl == 0) cx |= jb2_pixel(R, x + at[6], at[7]) << b++;
    return cx;
}

// one row, every context from its definition: the general path, for AT pixels anywhere
JP2_HD inline void jb2_row_general(Jp2Mq& m, const uint32_t* mq, uint8_t* cx, const Jb2Rows& R, int tmpl, const int8_t* at) {
    for (int x = 0; x < R.W; ++x) {
        const unsigned bit = (unsigned)jb2_mq_decode(m, mq, cx + jb2_context(R, x, tmpl, at));
        R.r0[x >> 5] |= bit << (x & 31);
    }
}

// One row with the AT pixels at their nominal places, where each row of the template is one run of pixels (row y - 1 of T0 is
// x - 3 .. x + 3 with A1 and A2 at its ends): the context is three windows that shift by one pixel a decision.  The rows are read a
// word at a time, two words of each held in a register.  r0 must be zero on entry.
JP2_HD inline void jb2_row_nominal(Jp2Mq& m, const uint32_t* mq, uint8_t* cx, const Jb2Rows& R, int tmpl) {
    // {pixels of row y, of row y - 1 and its rightmost offset, of row y - 2 and its rightmost offset}, AT pixels included
    const int ncur = tmpl == 1 ? 3 : tmpl == 2 ? 2 : 4, n1 = tmpl == 0 ? 7 : tmpl == 2 ? 5 : 6, right1 = tmpl <= 1 ? 3 : 2;
    const int n2 = tmpl == 0 ? 5 : tmpl == 1 ? 4 : tmpl == 2 ? 3 : 0, right2 = tmpl <= 1 ? 2 : 1;
    const unsigned mcur = (1u << ncur) - 1u, m1 = (1u << n1) - 1u, m2 = (1u << n2) - 1u;
    // windows at x = 0: bit k of w1 is pixel right1 - k of row y - 1
    unsigned cur = 0, w1 = 0, w2 = 0;
    for (int k = 0; k <= right1; ++k) w1 |= ((R.r1[0] >> (right1 - k)) & 1u) << k;
    for (int k = 0; k <= right2 && n2; ++k) w2 |= ((R.r2[0] >> (right2 - k)) & 1u) << k;
    const int nw = jb2_plane_words(R.W);
    for (int j = 0; j < nw; ++j) {
        const uint64_t v1 = (uint64_t)R.r1[j] | (uint64_t)R.r1[j + 1] << 32, v2 = n2 ? (uint64_t)R.r2[j] | (uint64_t)R.r2[j + 1] << 32 : 0;
        const int n = R.W - j * 32 < 32 ? R.W - j * 32 : 32;
        uint32_t word = 0;
        for (int i = 0; i < n; ++i) {
            const unsigned bit = (unsigned)jb2_mq_decode(m, mq, cx + (cur | w1 << ncur | w2 << (ncur + n1)));
            word |= bit << i;
            cur = ((cur << 1) | bit) & mcur;
            w1 = ((w1 << 1) | (unsigned)((v1 >> (i + right1 + 1)) & 1u)) & m1;
            w2 = ((w2 << 1) | (unsigned)((v2 >> (i + right2 + 1)) & 1u)) & m2;
        }
        R.r0[j] = word;
    }
}

// the SLTP decision in front of a row of a region with typical prediction -> 0 / 1
JP2_HD inline int jb2_sltp(Jp2Mq& m, const uint32_t* mq, uint8_t* cx, int tmpl) { return jb2_mq_decode(m, mq, cx + jb2_sltp_context(tmpl)); }
