#pragma once
#include "common.h"

// Reed-Solomon over GF(2^m), 4 <= m <= MAX_M, for one wave64 that is its own work-group: a block in LDS is corrected in place.  The
// field comes as its exp / log tables (exp doubled: 2 * 2^m entries, so that exp[log a + log b] needs no reduction) and the code as the
// exponent of its first root: the generator is (x - a^first_root) ... (x - a^(first_root + ec - 1)).  The block's first word is the
// highest power.  SYM is the symbol type of the tables and the arrays; MAX_LEN (a multiple of 64), MAX_EC and MAX_M size them.  The
// instantiations:
//   <unsigned char, 192, 30, 8>        QR, both stages (field 0x11D, first root 0): 1.1 KiB of LDS
//   <unsigned char, 256, 68, 8>        Data Matrix (field 0x12D, first root 1): 1.3 KiB
//   <unsigned short, 320, 318, 10>     Aztec up to 11 layers (GF(16) .. GF(1024), first root 1)
//   <unsigned short, 1664, 1662, 12>   Aztec's 32 layers (GF(4096), 16 + 8 KiB of tables; az_layers of aztec.hip): 38.6 KiB in all
// Syndromes, Chien search and Forney run with lanes over positions.  Berlekamp-Massey runs its inner updates with lanes over the
// coefficients and takes the discrepancy as a wave xor: ec steps of at most 3 ceil((ec + 2) / 64) field multiplications a lane and
// two barriers, 4.7 k multiplications a lane at ec = 315 where a one-lane loop would take about 2 ec^2 = 198 k (9.2 k at Data
// Matrix's ec = 68).  Every loop has a constant bound and every index stays inside its array whatever the block holds.
template <class SYM, int MAX_LEN, int MAX_EC, int MAX_M>
struct RsLds {
    static_assert(MAX_M <= 8 * (int)sizeof(SYM) && MAX_LEN % 64 == 0, "a symbol holds a field element; lanes walk whole chunks");
    SYM exp[2 << MAX_M], log[1 << MAX_M], blk[MAX_LEN];
    SYM S[MAX_EC + 2], C[MAX_EC + 2], Bp[MAX_EC + 2], O[MAX_EC / 2 + 2];
    int order, mask;   // 2^m - 1 twice: the multiplicative order, the symbol mask
};

// (a barrier inside: the whole wave calls it)
template <class S, class SYM>
__device__ __forceinline__ void rs_load_tables(S& s, const SYM* exp, const SYM* log, int m, int lane) {
    const int n = 1 << m;
    for (int i = lane; i < 2 * n; i += 64) s.exp[i] = exp[i];
    for (int i = lane; i < n; i += 64) s.log[i] = log[i];
    if (lane == 0) { s.order = n - 1; s.mask = n - 1; }
    __syncthreads();
}

template <class S>
__device__ __forceinline__ int rs_mul(const S& s, int a, int b) { return a && b ? s.exp[s.log[a & s.mask] + s.log[b & s.mask]] : 0; }
// a * alpha^e, 0 <= e < order
template <class S>
__device__ __forceinline__ int rs_mul_exp(const S& s, int a, int e) { return a ? s.exp[s.log[a & s.mask] + e] : 0; }
template <class S>
__device__ __forceinline__ int rs_inv(const S& s, int a) { return s.exp[s.order - s.log[a & s.mask]]; }

// the ec syndromes of s.blk[0 .. len) -> s.S, syndrome k at alpha^(first_root + k); true when one is not zero.  (barriers inside)
template <class SYM, int MAX_LEN, int MAX_EC, int MAX_M>
__device__ __forceinline__ bool rs_syndromes(RsLds<SYM, MAX_LEN, MAX_EC, MAX_M>& s, int len, int ec, int first_root, int lane) {
    constexpr int NCH = MAX_LEN / 64;
    const int order = s.order;
    int step[NCH], e[NCH], v[NCH];   // position p = c * 64 + lane: its power len - 1 - p, the running exponent (first_root + k) * power mod order
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int p = c * 64 + lane;
        step[c] = p < len ? (len - 1 - p) % order : 0;
        e[c] = first_root == 1 ? 0 : (first_root + order - 1) % order * step[c] % order;   // one step short of syndrome 0's (< 2^24)
        v[c] = p < len ? s.blk[p] : 0;
    }
    int nz = 0;
#pragma unroll 1
    for (int k = 0; k < MAX_EC; ++k) {
        if (k >= ec) break;
        int acc = 0;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            e[c] += step[c];
            if (e[c] >= order) e[c] -= order;
            acc ^= rs_mul_exp(s, v[c], e[c]);
        }
        acc = wave_xor(acc);
        if (lane == 0) s.S[k] = (SYM)acc;
        nz |= acc;
    }
    __syncthreads();
    return nz != 0;
}

// Berlekamp-Massey over s.S[0 .. ec) by the whole wave -> s.C (the locator), s.O (the evaluator's first L coefficients); returns L
template <class SYM, int MAX_LEN, int MAX_EC, int MAX_M>
__device__ __forceinline__ int rs_locator(RsLds<SYM, MAX_LEN, MAX_EC, MAX_M>& s, int ec, int lane) {
    constexpr int NC = MAX_EC + 2, NCH = (NC + 63) / 64;
    for (int i = lane; i < NC; i += 64) { s.C[i] = i == 0; s.Bp[i] = i == 0; }
    __syncthreads();
    int L = 0, m = 1, b = 1;
#pragma unroll 1
    for (int k = 0; k < MAX_EC; ++k) {
        if (k >= ec) break;
        int d = 0;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int i = c * 64 + lane;
            if (i <= L && i <= k) d ^= rs_mul(s, s.C[i], s.S[k - i]);
        }
        d = wave_xor(d);
        if (d == 0) { ++m; continue; }   // (wave-uniform)
        const int f = rs_mul(s, d, rs_inv(s, b));
        int oc[NCH], nc[NCH];
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int i = c * 64 + lane;
            oc[c] = i < NC ? s.C[i] : 0;
            nc[c] = (i >= m && i <= ec && i < NC) ? rs_mul(s, f, s.Bp[i - m]) : 0;
        }
        __syncthreads();
        const bool grow = 2 * L <= k;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int i = c * 64 + lane;
            if (i < NC) {
                s.C[i] = (SYM)(oc[c] ^ nc[c]);
                if (grow) s.Bp[i] = (SYM)oc[c];
            }
        }
        __syncthreads();
        if (grow) { L = k + 1 - L; b = d; m = 1; } else ++m;
    }
    if (L > ec / 2 || L > MAX_EC / 2) return L;
    for (int i = lane; i < MAX_EC / 2 + 2; i += 64) {
        int o = 0;
        if (i < L)
            for (int j = 0; j <= MAX_EC / 2 + 1; ++j) {
                if (j > i) break;
                o ^= rs_mul(s, s.S[i - j], s.C[j]);
            }
        s.O[i] = (SYM)o;
    }
    __syncthreads();
    return L;
}

// s.blk[0 .. len) (len <= MAX_LEN, 2 <= ec <= MAX_EC, ec < len, len <= order, 0 <= first_root <= order) corrected in place -> the number
// of errors, or -1 when the block has more than ec / 2 of them.  The whole wave calls it (barriers inside) and gets one answer.
template <class SYM, int MAX_LEN, int MAX_EC, int MAX_M>
__device__ __forceinline__ int rs_correct_block(RsLds<SYM, MAX_LEN, MAX_EC, MAX_M>& s, int len, int ec, int first_root, int lane) {
    if (!rs_syndromes(s, len, ec, first_root, lane)) return 0;
    const int L = rs_locator(s, ec, lane);
    if (L > ec / 2 || L > MAX_EC / 2) return -1;
    const int order = s.order;
    const int xpow = (order + 1 - first_root) % order;   // Forney's factor X^(1 - first_root): none when the first root is a^1
    int roots = 0;
    bool bad = false;
#pragma unroll 1
    for (int p0 = 0; p0 < MAX_LEN; p0 += 64) {
        const int p = p0 + lane, e = (len - 1 - p + 2 * order) % order, xi = (order - e) % order;   // X = alpha^e, xi = log of X^-1
        int val = 1, den = 0, num = 0;
        if (p < len) {
            val = 0;
            int ei = 0, eprev = 0;   // xi * i mod order, xi * (i - 1) mod order
            for (int i = 0; i <= MAX_EC / 2; ++i) {
                if (i > L) break;
                const int c = s.C[i];
                val ^= rs_mul_exp(s, c, ei);
                if (i & 1) den ^= rs_mul_exp(s, c, eprev);
                if (i < L) num ^= rs_mul_exp(s, s.O[i], ei);
                eprev = ei;
                ei += xi;
                if (ei >= order) ei -= order;
            }
        }
        const bool root = val == 0;
        if (root) {
            if (den == 0) bad = true;
            else {
                int fix = rs_mul(s, num, rs_inv(s, den));
                if (xpow) fix = rs_mul_exp(s, fix, e * xpow % order);
                s.blk[p] ^= (SYM)fix;
            }
        }
        roots += __popcll(__ballot(root));
    }
    __syncthreads();
    if (__ballot(bad) || roots != L) return -1;
    if (rs_syndromes(s, len, ec, first_root, lane)) return -1;
    return L;
}
