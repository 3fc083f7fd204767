#pragma once
#include "common.h"

// Reed-Solomon over GF(256) for one wave64 that is its own work-group: a block in LDS is corrected in place.  The field comes as
// its exp / log tables (exp doubled: 512 entries, so that exp[log a + log b] needs no reduction) and the code as the exponent of
// its first root: the generator is (x - a^first_root) ... (x - a^(first_root + ec - 1)).  MAX_LEN (a multiple of 64) and MAX_EC size
// the arrays; the block's first codeword is the highest power.  Syndromes, Chien search and Forney run with lanes over positions;
// Berlekamp-Massey is one lane's serial loop (about 2 ec^2 field steps: 9.2 k at ec = 68).  Every loop has a constant bound and
// every index stays inside its array whatever the block holds.
template <int MAX_LEN, int MAX_EC>
struct RsLds {
    unsigned char exp[512], log[256], blk[MAX_LEN];
    int S[MAX_EC + 4], C[MAX_EC + 4], Bp[MAX_EC + 4], T[MAX_EC + 4], O[MAX_EC / 2 + 2];
    int L;
};

template <class S>
__device__ __forceinline__ void rs_load_tables(S& s, const unsigned char* exp, const unsigned char* log, int lane) {
    for (int i = lane; i < 512; i += 64) s.exp[i] = exp[i];
    for (int i = lane; i < 256; i += 64) s.log[i] = log[i];
}

template <class S>
__device__ __forceinline__ int rs_mul(const S& s, int a, int b) { return a && b ? s.exp[s.log[a & 255] + s.log[b & 255]] : 0; }
// a * alpha^e, 0 <= e <= 255 (log a + e <= 509, inside the doubled table)
template <class S>
__device__ __forceinline__ int rs_mul_exp(const S& s, int a, int e) { return a ? s.exp[s.log[a & 255] + e] : 0; }

// the ec syndromes of s.blk[0 .. len) -> s.S; true when one is not zero.  (barriers inside: the whole wave calls it)
template <int MAX_LEN, int MAX_EC>
__device__ __forceinline__ bool rs_syndromes(RsLds<MAX_LEN, MAX_EC>& s, int len, int ec, int first_root, int lane) {
    int nz = 0;
    for (int k = 0; k < MAX_EC; ++k) {
        if (k >= ec) break;
        int acc = 0;
#pragma unroll
        for (int p0 = 0; p0 < MAX_LEN; p0 += 64) {
            const int p = p0 + lane;
            if (p < len) acc ^= rs_mul_exp(s, s.blk[p], ((k + first_root) * (len - 1 - p)) % 255);
        }
        acc = wave_xor(acc);
        if (lane == 0) s.S[k] = acc;
        nz |= acc;
    }
    __syncthreads();
    return nz != 0;
}

// Berlekamp-Massey over s.S[0 .. ec) by one lane -> s.C (the locator), s.O (the evaluator's first L coefficients), s.L
template <int MAX_LEN, int MAX_EC>
__device__ __forceinline__ void rs_locator(RsLds<MAX_LEN, MAX_EC>& s, int ec) {
    for (int i = 0; i < MAX_EC + 4; ++i) { s.C[i] = 0; s.Bp[i] = 0; }
    s.C[0] = 1; s.Bp[0] = 1;
    int L = 0, m = 1, b = 1;
    for (int k = 0; k < MAX_EC; ++k) {
        if (k >= ec) break;
        int d = s.S[k];
        for (int i = 1; i <= MAX_EC; ++i) {
            if (i > L || i > k) break;
            d ^= rs_mul(s, s.C[i], s.S[k - i]);
        }
        if (d == 0) { ++m; continue; }
        for (int i = 0; i < MAX_EC + 4; ++i) s.T[i] = s.C[i];
        const int f = rs_mul_exp(s, d, 255 - s.log[b & 255]);
        for (int i = 0; i <= MAX_EC; ++i) {
            if (i + m > ec) break;
            s.C[i + m] ^= rs_mul(s, f, s.Bp[i]);
        }
        if (2 * L <= k) {
            L = k + 1 - L; b = d; m = 1;
            for (int i = 0; i < MAX_EC + 4; ++i) s.Bp[i] = s.T[i];
        } else ++m;
    }
    for (int i = 0; i < MAX_EC / 2 + 2; ++i) {
        int o = 0;
        if (i < L)
            for (int j = 0; j <= MAX_EC / 2 + 1; ++j) {
                if (j > i) break;
                o ^= rs_mul(s, s.S[i - j], s.C[j]);
            }
        s.O[i] = o;
    }
    s.L = L;
}

// s.blk[0 .. len) (len <= MAX_LEN, 2 <= ec <= MAX_EC, ec < len) corrected in place -> the number of errors, or -1 when the block
// has more than ec / 2 of them.  The whole wave calls it (barriers inside) and gets one answer.
template <int MAX_LEN, int MAX_EC>
__device__ __forceinline__ int rs_correct_block(RsLds<MAX_LEN, MAX_EC>& s, int len, int ec, int first_root, int lane) {
    if (!rs_syndromes(s, len, ec, first_root, lane)) return 0;
    if (lane == 0) rs_locator(s, ec);
    __syncthreads();
    const int L = s.L;
    if (L > ec / 2 || L > MAX_EC / 2) return -1;
    const int xpow = (256 - first_root) % 255;   // Forney's factor X^(1 - first_root)
    int roots = 0;
    bool bad = false;
#pragma unroll 1
    for (int p0 = 0; p0 < MAX_LEN; p0 += 64) {
        const int p = p0 + lane, e = (len - 1 - p + 255) % 255, xi = (255 - e) % 255;   // X = alpha^e, xi = log of X^-1
        int val = 1, den = 0, num = 0;
        if (p < len) {
            val = 0;
            for (int i = 0; i <= MAX_EC / 2; ++i) {
                if (i > L) break;
                val ^= rs_mul_exp(s, s.C[i], (xi * i) % 255);
                if (i & 1) den ^= rs_mul_exp(s, s.C[i], (xi * (i - 1)) % 255);
                if (i < L) num ^= rs_mul_exp(s, s.O[i], (xi * i) % 255);
            }
        }
        const bool root = val == 0;
        if (root) {
            if (den == 0) bad = true;
            else s.blk[p] ^= (unsigned char)rs_mul_exp(s, rs_mul_exp(s, num, 255 - s.log[den & 255]), (e * xpow) % 255);
        }
        roots += __popcll(__ballot(root));
    }
    __syncthreads();
    if (__ballot(bad) || roots != L) return -1;
    if (rs_syndromes(s, len, ec, first_root, lane)) return -1;
    return L;
}
