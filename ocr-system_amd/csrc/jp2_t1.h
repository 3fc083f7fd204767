// JPEG 2000 tier 1, the 5/3 lifting steps and the 9/7 path (dequantisation, lifting, colour, rounding) as plain functions: the decision walk of one code-block (MQ decoder + EBCOT context
// modelling) over a Jp2T1State, and the per-sample inverse lifting.  jp2dec.hip runs them on the device (the state in LDS, one wave
// per block); tests/jp2_parse_main.cpp compiles the same text for the host, where the sanitizers can see it.
#pragma once
#include <cstdint>

#include "jp2_tables.h"

// The state of one code-block (sides <= 64).  Row r of the block is word r + 1 of each map (words 0 and 65 stay empty: the
// neighbours outside the block are insignificant); bit x of a word is column x.  The MQ state table sits beside them, so that no
// step of the walk waits for global memory.  10.5 KB: 15 blocks fit the 160 KB of a CU.
struct Jp2T1State {
    uint64_t sig[66], sgn[66], vis[66], ref[66];   // significant, negative, coded in this plane's significance pass, refined once
    uint16_t mag[64 * 64];                         // magnitude with one fractional bit (see jp2_t1_walk)
    uint32_t mq[48];                               // jp2_mq_states
};

// fills the table of S; `lane` of `lanes` callers takes every lanes-th entry
JP2_HD inline void jp2_t1_tables(Jp2T1State& S, int lane, int lanes) {
    for (int i = lane; i < 47; i += lanes) S.mq[i] = jp2_mq_states[i];
}

// the MQ decoder's registers, with the 19 contexts packed a byte each (state index << 1 | MPS) into three words: they stay in registers
struct Jp2Mq {
    const uint8_t* d;
    uint32_t len, p, c, a;
    int ct;
    uint64_t cx[3];
};

JP2_HD inline uint32_t jp2_mq_byte(const Jp2Mq& m, uint32_t i) { return i < m.len ? m.d[i] : 0xFFu; }   // 0xFF past the block's data

// byte-in: 0xFF followed by a byte over 0x8F is the end of the data (the decoder then feeds ones and stays there)
JP2_HD inline void jp2_mq_bytein(Jp2Mq& m) {
    const uint32_t cur = jp2_mq_byte(m, m.p), nxt = jp2_mq_byte(m, m.p + 1);
    if (cur == 0xFF) {
        if (nxt > 0x8F) { m.c += 0xFF00; m.ct = 8; }
        else { ++m.p; m.c += nxt << 9; m.ct = 7; }
    } else {
        ++m.p; m.c += nxt << 8; m.ct = 8;
    }
}

JP2_HD inline void jp2_mq_init(Jp2Mq& m, const uint8_t* d, uint32_t len) {
    m.d = d; m.len = len; m.p = 0;
    m.c = jp2_mq_byte(m, 0) << 16;
    jp2_mq_bytein(m);
    m.c <<= 7; m.ct -= 7; m.a = 0x8000;
}

JP2_HD inline int jp2_mq_decode(Jp2Mq& m, const Jp2T1State& S, int k) {
    const int sh = (k & 7) * 8;
    const uint64_t word = k < 8 ? m.cx[0] : k < 16 ? m.cx[1] : m.cx[2];
    const uint32_t s = (uint32_t)(word >> sh) & 0xFF, st = S.mq[s >> 1], qe = st & 0xFFFF;
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
    uint32_t next;
    if (lps) {
        bit ^= 1;
        next = (((st >> 22) & 63) << 1) | ((s & 1) ^ (st >> 28));
    } else {
        next = (((st >> 16) & 63) << 1) | (s & 1);
    }
    const uint64_t updated = (word & ~(0xFFull << sh)) | ((uint64_t)next << sh);
    if (k < 8) m.cx[0] = updated; else if (k < 16) m.cx[1] = updated; else m.cx[2] = updated;
    do {
        if (m.ct == 0) jp2_mq_bytein(m);
        m.a <<= 1; m.c <<= 1; --m.ct;
    } while (!(m.a & 0x8000));
    return bit;
}

// bits x-1, x, x+1 of a row word as bits 0, 1, 2
JP2_HD inline unsigned jp2_win3(uint64_t w, int x) { return x ? (unsigned)(w >> (x - 1)) & 7u : (unsigned)(w << 1) & 7u; }

// zero-coding context of (row word index r, column x); 0 <=> no significant neighbour
JP2_HD inline int jp2_zc(const Jp2T1State& S, int r, int x, int orient) {
    const unsigned up = jp2_win3(S.sig[r - 1], x), cur = jp2_win3(S.sig[r], x), dn = jp2_win3(S.sig[r + 1], x);
    if (!(up | (cur & 5u) | dn)) return 0;
    int h = __builtin_popcount(cur & 5u), v = (int)((up >> 1) & 1u) + (int)((dn >> 1) & 1u);
    const int d = __builtin_popcount(up & 5u) + __builtin_popcount(dn & 5u);
    if (orient == 3) return (int)(JP2_ZC_HH >> (((h + v > 2 ? 2 : h + v) * 5 + d) * 4)) & 15;
    if (orient == 1) { const int t = h; h = v; v = t; }
    const uint64_t row = h == 0 ? JP2_ZC_LH[0] : h == 1 ? JP2_ZC_LH[1] : JP2_ZC_LH[2];
    return (int)(row >> ((v * 5 + d) * 4)) & 15;
}

JP2_HD inline bool jp2_any_neighbour(const Jp2T1State& S, int r, int x) {
    return (jp2_win3(S.sig[r - 1], x) | (jp2_win3(S.sig[r], x) & 5u) | jp2_win3(S.sig[r + 1], x)) != 0;
}

// decodes the sign of (r, x), which has just become significant in plane bp
JP2_HD inline void jp2_become_significant(Jp2T1State& S, Jp2Mq& m, int r, int x, int bp) {
    const unsigned cs = jp2_win3(S.sig[r], x), cn = jp2_win3(S.sgn[r], x);
    const int us = (int)(S.sig[r - 1] >> x) & 1, un = (int)(S.sgn[r - 1] >> x) & 1, ds = (int)(S.sig[r + 1] >> x) & 1, dn = (int)(S.sgn[r + 1] >> x) & 1;
    int hc = (int)(cs & 1) * (1 - 2 * (int)(cn & 1)) + (int)((cs >> 2) & 1) * (1 - 2 * (int)((cn >> 2) & 1));
    int vc = us * (1 - 2 * un) + ds * (1 - 2 * dn);
    hc = hc > 1 ? 1 : hc < -1 ? -1 : hc;
    vc = vc > 1 ? 1 : vc < -1 ? -1 : vc;
    int x_or = 0;
    if (hc < 0 || (hc == 0 && vc < 0)) { hc = -hc; vc = -vc; x_or = 1; }
    const int neg = jp2_mq_decode(m, S, (hc ? 12 : 9) + vc) ^ x_or;
    S.sig[r] |= 1ull << x;
    if (neg) S.sgn[r] |= 1ull << x;
    S.mag[(r - 1) * 64 + x] = (uint16_t)(3u << bp);
}

// The decision walk: npasses coding passes from bit-plane nbps - 1 down, the first a clean-up pass.  S.sig/sgn/vis/ref/mag must be
// zero and the table filled (jp2_t1_tables) on entry.  Magnitudes carry one fractional bit, which is how a block that stops early is
// reconstructed: a coefficient that becomes significant in plane p is 1.5 * 2^p (3 << p in half units), a refinement in plane q adds or takes 2^q half units, and the
// caller halves toward zero.  A block decoded to plane 0 comes out exact.
JP2_HD inline void jp2_t1_walk(Jp2T1State& S, const uint8_t* data, uint32_t len, int w, int h, int orient, int nbps, int npasses) {
    Jp2Mq m;
    jp2_mq_init(m, data, len);
    // initial states (Table D.7): 4 for the first zero-coding context, 3 for the run-length context, 46 for UNIFORM, 0 elsewhere
    m.cx[0] = (uint64_t)(4 << 1);
    m.cx[1] = 0;
    m.cx[2] = (uint64_t)(3 << 1) << ((JP2_CX_RUN & 7) * 8) | (uint64_t)(46 << 1) << ((JP2_CX_UNI & 7) * 8);
    const uint64_t wmask = w == 64 ? ~0ull : (1ull << w) - 1;
    int bp = nbps - 1, kind = 2;
    for (int pass = 0; pass < npasses; ++pass) {
        for (int y0 = 0; y0 < h; y0 += 4) {
            const int rows = h - y0 < 4 ? h - y0 : 4, r0 = y0 + 1;
            if (kind == 0) {   // significance propagation: insignificant coefficients with a significant neighbour
                uint64_t any = 0;
                for (int r = r0 - 1; r <= r0 + rows; ++r) any |= S.sig[r];
                uint64_t cols = (any | any << 1 | any >> 1) & wmask;
                while (cols) {
                    const int x = __builtin_ctzll(cols);
                    cols &= cols - 1;
                    for (int k = 0; k < rows; ++k) {
                        const int r = r0 + k;
                        if ((S.sig[r] >> x) & 1) continue;
                        const int cx = jp2_zc(S, r, x, orient);
                        if (!cx) continue;
                        if (jp2_mq_decode(m, S, cx)) {
                            jp2_become_significant(S, m, r, x, bp);
                            if (x + 1 < w) cols |= 2ull << x;   // the next column now has a significant neighbour
                        }
                        S.vis[r] |= 1ull << x;
                    }
                }
            } else if (kind == 1) {   // magnitude refinement: significant before this plane
                uint64_t cols = 0;
                for (int k = 0; k < rows; ++k) cols |= S.sig[r0 + k] & ~S.vis[r0 + k];
                while (cols) {
                    const int x = __builtin_ctzll(cols);
                    cols &= cols - 1;
                    for (int k = 0; k < rows; ++k) {
                        const int r = r0 + k;
                        if (!(((S.sig[r] & ~S.vis[r]) >> x) & 1)) continue;
                        const int cx = ((S.ref[r] >> x) & 1) ? 16 : jp2_any_neighbour(S, r, x) ? 15 : 14;
                        uint16_t& mg = S.mag[(r - 1) * 64 + x];
                        mg = (uint16_t)(jp2_mq_decode(m, S, cx) ? mg + (1u << bp) : mg - (1u << bp));
                        S.ref[r] |= 1ull << x;
                    }
                }
            } else {   // clean-up: everything not coded in this plane yet, with the run-length mode on untouched columns
                // columns of a full stripe with no significant coefficient in the stripe or around it, and nothing visited
                uint64_t quiet = 0;
                if (rows == 4) {
                    uint64_t any = 0;
                    for (int r = r0 - 1; r <= r0 + 4; ++r) any |= S.sig[r];
                    quiet = ~(any | any << 1 | any >> 1 | S.vis[r0] | S.vis[r0 + 1] | S.vis[r0 + 2] | S.vis[r0 + 3]);
                }
                // what is left to code, per row of the stripe (a coefficient is coded only where the walk reaches it, so the words hold)
                uint64_t todo[4];
                uint64_t cols = 0;
                for (int k = 0; k < 4; ++k) {
                    todo[k] = k < rows ? ~(S.sig[r0 + k] | S.vis[r0 + k]) & wmask : 0;
                    cols |= todo[k];
                }
                while (cols) {
                    const int x = __builtin_ctzll(cols);
                    cols &= cols - 1;
                    const unsigned left = (unsigned)((todo[0] >> x) & 1) | (unsigned)((todo[1] >> x) & 1) << 1 | (unsigned)((todo[2] >> x) & 1) << 2 |
                                          (unsigned)((todo[3] >> x) & 1) << 3;
                    int k = 0;
                    // (a coefficient of column x - 1 that became significant in this pass ends the run mode of column x)
                    if (((quiet >> x) & 1) && !(x && (((S.sig[r0] | S.sig[r0 + 1] | S.sig[r0 + 2] | S.sig[r0 + 3]) >> (x - 1)) & 1))) {
                        if (!jp2_mq_decode(m, S, JP2_CX_RUN)) continue;
                        k = jp2_mq_decode(m, S, JP2_CX_UNI) << 1;
                        k |= jp2_mq_decode(m, S, JP2_CX_UNI);
                        jp2_become_significant(S, m, r0 + k, x, bp);
                        ++k;
                    }
                    for (; k < rows; ++k) {
                        const int r = r0 + k;
                        if (!((left >> k) & 1)) continue;
                        if (jp2_mq_decode(m, S, jp2_zc(S, r, x, orient))) jp2_become_significant(S, m, r, x, bp);
                    }
                }
            }
        }
        if (kind == 2) {
            for (int r = 1; r <= h; ++r) S.vis[r] = 0;
            --bp;
        }
        kind = kind == 2 ? 0 : kind + 1;
    }
}

// the coefficient of (y, x) after the walk
JP2_HD inline int jp2_t1_value(const Jp2T1State& S, int y, int x) {
    const int v = S.mag[y * 64 + x] >> 1;
    return ((S.sgn[y + 1] >> x) & 1) ? -v : v;
}

// ---- inverse 5/3 lifting of one line of n samples whose first canvas coordinate has parity cas, low-pass samples first (sn of them),
// sample i of the line at line[i * stride].  Sample i of the rebuilt line sits on a low-pass position where i + cas is even, and is
// the (i >> 1)-th of its kind either way.  Whole-sample symmetric extension by canvas parity: a neighbour outside the line is
// replaced by the other one.  A line of one sample is its low-pass sample (cas 0) or half its high-pass sample, toward zero (cas 1).
template <class T>
JP2_HD inline int jp2_lift_low(const T* line, long long stride, int n, int cas, int i) {   // i + cas even
    const int sn = (n + 1 - cas) >> 1;
    const int s = line[(i >> 1) * stride];
    if (n == sn) return s;
    const int l = i > 0 ? i - 1 : i + 1, r = i + 1 < n ? i + 1 : i - 1;
    const int dl = line[(sn + (l >> 1)) * stride], dr = line[(sn + (r >> 1)) * stride];
    return s - ((dl + dr + 2) >> 2);
}
template <class T>
JP2_HD inline int jp2_lift_high(const T* line, long long stride, int n, int cas, int i) {   // i + cas odd
    const int sn = (n + 1 - cas) >> 1;
    const int d = line[(sn + (i >> 1)) * stride];
    if (sn == 0) return d / 2;
    const int l = i > 0 ? i - 1 : i + 1, r = i + 1 < n ? i + 1 : i - 1;
    return d + ((jp2_lift_low(line, stride, n, cas, l) + jp2_lift_low(line, stride, n, cas, r)) >> 1);
}
template <class T>
JP2_HD inline int jp2_lift_at(const T* line, long long stride, int n, int cas, int i) {
    return ((i + cas) & 1) ? jp2_lift_high(line, stride, n, cas, i) : jp2_lift_low(line, stride, n, cas, i);
}
// the k-th low-pass position / the k-th high-pass position of the line
template <class T>
JP2_HD inline int jp2_lift_even(const T* line, long long stride, int n, int k, int cas = 0) { return jp2_lift_low(line, stride, n, cas, 2 * k + cas); }
template <class T>
JP2_HD inline int jp2_lift_odd(const T* line, long long stride, int n, int k, int cas = 0) { return jp2_lift_high(line, stride, n, cas, 2 * k + 1 - cas); }

// ---- the 9/7 irreversible path, in single precision in the order OpenJPEG evaluates it.  Every expression below is one rounding per
// operation (the project compiles with -ffp-contract=off, and subnormals are kept), so host, device and any tiling give the same bits.

// the coefficient of (y, x) after the walk, dequantised: the signed magnitude in half units times half the sub-band's step size
JP2_HD inline float jp2_t1_value_f(const Jp2T1State& S, int y, int x, float hs) {
    const int v = S.mag[y * 64 + x];
    return (float)(((S.sgn[y + 1] >> x) & 1) ? -v : v) * hs;
}

// the scaling of a low-pass / high-pass sample as it is interleaved, and the four lifting steps: step s updates the samples of canvas
// parity s & 1 (0: the low-pass positions; jp2_lift97_first) as x -= (left + right) * jp2_lift97_coef(s)
#define JP2_K97_LOW 1.230174105f
#define JP2_K97_HIGH 1.625732422f
JP2_HD inline float jp2_lift97_coef(int s) { return s == 0 ? 0.443506852f : s == 1 ? 0.882911075f : s == 2 ? -0.052980118f : -1.586134342f; }

// sample i of the interleaved line of n >= 2 samples whose first canvas coordinate has parity cas, read from the sub-band order
// (low-pass first, sn = (n + 1 - cas) / 2 of them): low-pass where i + cas is even
JP2_HD inline float jp2_lift97_load(const float* line, long long stride, int n, int i, int cas = 0) {
    return ((i + cas) & 1) ? line[(((n + 1 - cas) >> 1) + (i >> 1)) * stride] * JP2_K97_HIGH : line[(i >> 1) * stride] * JP2_K97_LOW;
}
// the first sample at or after lo that step s updates: the steps go by canvas parity (s & 1: 0 low-pass positions, 1 high-pass ones)
JP2_HD inline int jp2_lift97_first(int lo, int s, int cas) { return lo + ((lo + cas + s) & 1); }

// One lifting step at sample i of an interleaved line of n samples whose samples [lo, hi) are held at w[(i - lo) * stride].  A neighbour
// outside the line is replaced by the other one (whole-sample mirror); a sample with a neighbour inside the line but outside the window
// is left as it is: it belongs to the window's halo, which the four steps eat one sample a side each.  So a window that starts and
// ends on even samples comes out right from lo + JP2_LIFT97_HALO to hi - JP2_LIFT97_HALO, and up to an end of the line it holds.
constexpr int JP2_LIFT97_HALO = 4;
JP2_HD inline void jp2_lift97_at(float* w, long long stride, int lo, int hi, int n, int i, float c) {
    const int l = i > 0 ? i - 1 : i + 1, r = i + 1 < n ? i + 1 : i - 1;
    if (l < lo || r < lo || l >= hi || r >= hi) return;
    w[(i - lo) * stride] = w[(i - lo) * stride] - (w[(l - lo) * stride] + w[(r - lo) * stride]) * c;
}

// round to nearest even, level shift, clamp
JP2_HD inline uint8_t jp2_sample97(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
    const int i = __float2int_rn(v) + 128;
#else
    const int i = (int)__builtin_lrintf(v) + 128;
#endif
    return (uint8_t)(i < 0 ? 0 : i > 255 ? 255 : i);
}

// the inverse irreversible colour transform of one pixel, then jp2_sample97
JP2_HD inline void jp2_finish97(float y, float u, float v, int mct, uint8_t rgb[3]) {
    float r = y, g = u, b = v;
    if (mct) {
        r = y + v * 1.402f;
        g = y - u * 0.34413f - v * 0.71414f;
        b = y + u * 1.772f;
    }
    rgb[0] = jp2_sample97(r); rgb[1] = jp2_sample97(g); rgb[2] = jp2_sample97(b);
}
