// The line stages of the fax decoders, shared by the kernels that read T.6 lines: cc_decode and fx_decode (ccitt.hip) and the MMR
// regions of JBIG2 (jbig2.hip).  Device code for one wave64: the lookup tables and changing-element arrays in LDS, the wave-uniform
// bit reader, one run length, one two-dimensional line, and the finished line as packed words.  ccitt.hip says how they work together.
#pragma once
#include "ccitt.h"
#include "ccitt_tables.h"

namespace {

constexpr int CC_WBITS = 12, CC_BBITS = 13, CC_MBITS = 7;
constexpr size_t CC_Z_PAD = 512;   // zero tail per stream: the bit reader's word window may look past the stream

struct CcLds {
    unsigned short ce[2][CC_MAX_COLS + 8];   // changing elements of two lines, each followed by three sentinels (= columns)
    unsigned short wt[1 << CC_WBITS], bt[1 << CC_BBITS], mt[1 << CC_MBITS];   // code length << 12 | value; 0: no such code
    unsigned bits[CC_MAX_COLS / 32];   // the finished line, 1 = coded black, pixel x at bit x & 31 of word x >> 5
};

// wave-uniform MSB-first bit reader: lanes hold 64 consecutive byte-swapped words from word `wbase`
struct CcBits {
    const uint32_t* z32;
    unsigned zlen, pos, wbase;
    uint32_t w;
    bool bad;
    __device__ void load(int lane) {
        wbase = pos >> 5;
        if ((size_t)wbase * 4 > (size_t)zlen + 8) { bad = true; wbase = 0; }   // ran past the stream (the tail padding covers one window)
        w = __builtin_bswap32(z32[wbase + lane]);
    }
    // the next 32 bits, the first one on top
    __device__ uint32_t peek(int lane) {
        if (bad) return 0;
        if ((pos >> 5) - wbase >= 32) { load(lane); if (bad) return 0; }
        const int idx = (int)((pos >> 5) - wbase);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)w, idx), lo = (uint32_t)__builtin_amdgcn_readlane((int)w, idx + 1);
        return (uint32_t)((((((uint64_t)hi) << 32) | lo) << (pos & 31)) >> 32);
    }
};

__device__ void cc_fill(unsigned short* table, int bits, const unsigned* codes, int ncodes, int lane) {
    for (int i = lane; i < (1 << bits); i += 64) table[i] = 0;
    __syncthreads();
    for (int c = 0; c < ncodes; ++c) {
        const unsigned code = codes[c];
        const int len = (int)((code >> 12) & 15);
        const int base = (int)(code >> 16) << (bits - len), span = 1 << (bits - len);
        for (int i = lane; i < span; i += 64) table[base + i] = (unsigned short)(code & 0xFFFFu);
    }
    __syncthreads();
}

// one run length: make-up codes, then a terminating code.  -1: an unused code, a run longer than `room`, or bits past the stream.
// Ends: every pass returns or adds at least 64 to `total`.
__device__ int cc_run(const CcLds& L, CcBits& b, bool white, int room, unsigned limit, int lane) {
    int total = 0;
    for (;;) {
        const uint32_t top = b.peek(lane);
        const unsigned e = white ? L.wt[top >> (32 - CC_WBITS)] : L.bt[top >> (32 - CC_BBITS)];
        if (e == 0) return -1;
        b.pos += e >> 12;
        total += (int)(e & 4095);
        if (total > room || b.pos > limit) return -1;
        if ((e & 4095) < 64) return total;
    }
}

// one line in the two-dimensional coding against the changing elements `ref` of the line above (T.6; T.4 with K > 0): the line's
// changing elements go to `cur`.  -> their number, -1 corrupt.  Wave-uniform; lane 0 writes.
__device__ __forceinline__ int cc_line_2d(const CcLds& L, CcBits& b, const unsigned short* ref, unsigned short* cur, int W, unsigned limit, int lane) {
    int a0 = -1, n = 0, ri = 0;
    bool white = true;
    while (a0 < W) {
        while ((int)ref[ri] <= a0) ri += 2;   // b1: the first changing element right of a0 that changes to the opposite colour (ends at a sentinel: a0 < W)
        const int b1 = ref[ri], b2 = ref[ri + 1];
        const unsigned e = L.mt[b.peek(lane) >> (32 - CC_MBITS)];
        if (e == 0) return -1;
        b.pos += e >> 12;
        if (b.pos > limit) return -1;
        const int mode = (int)(e & 4095);
        if (mode == CC_M_PASS) {
            if (b2 >= W) return -1;   // T.6, pass mode: "identified when the position of b2 lies to the left of a1", and a1 <= columns
            a0 = b2;   // (b2 > b1 > a0)
            continue;
        }
        if (mode == CC_M_HORIZ) {
            const int start = a0 < 0 ? 0 : a0;
            const int r1 = cc_run(L, b, white, W - start, limit, lane);
            if (r1 < 0) return -1;
            const int r2 = cc_run(L, b, !white, W - start - r1, limit, lane);
            if (r2 < 0) return -1;
            const int t1 = start + r1, t2 = t1 + r2;
            if (t2 <= a0) return -1;
            // (a change at the line's end is the sentinel's and takes no room: a line of `columns` elements may end with such a pair)
            if (n + (t1 < W) + (t2 < W) > W + 1) return -1;
            if (lane == 0) {
                if (t1 < W) cur[n] = (unsigned short)t1;
                if (t2 < W) cur[n + (t1 < W)] = (unsigned short)t2;
            }
            n += (t1 < W) + (t2 < W);
            a0 = t2;
        } else {
            const int d = mode <= CC_M_VR3 ? mode - CC_M_V0 : CC_M_VR3 - mode;
            const int a1 = b1 + d;
            if (a1 <= a0 || a1 > W || (a1 < W && n + 1 > W + 1)) return -1;
            if (a1 < W) {
                if (lane == 0) cur[n] = (unsigned short)a1;
                ++n;
            }
            a0 = a1;
            white = !white;
            ri = ri > 0 ? ri - 1 : ri + 1;
        }
    }
    return n;
}

// the finished line, n <= W + 1 changing elements in `cur` (one of L.ce): its three sentinels, then its pixels as the words of L.bits.
// The whole wave: lanes over 32-pixel words.
__device__ __forceinline__ void cc_line_words(CcLds& L, unsigned short* cur, int n, int W, int lane) {
    if (lane < 3) cur[n + lane] = (unsigned short)W;
    __syncthreads();
    // the line's words: pixel x is coded black when an odd number of changing elements lie at or left of it
    for (int j = lane; j * 32 < W; j += 64) {
        const int x0 = j * 32;
        int lo = 0, hi = n;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((int)cur[mid] <= x0) lo = mid + 1; else hi = mid;
        }
        int k = lo, pos = 0;
        unsigned word = 0;
        for (;;) {
            const int next = k < n ? min((int)cur[k] - x0, 32) : 32;
            if ((k & 1) && next > pos) word |= (next >= 32 ? 0xFFFFFFFFu : ((1u << next) - 1u)) & ~((1u << pos) - 1u);
            pos = next;
            if (pos >= 32) break;
            ++k;
        }
        L.bits[j] = word;
    }
    __syncthreads();
}

__device__ __forceinline__ void cc_tables(CcLds& L, int W, int lane) {
    cc_fill(L.wt, CC_WBITS, cc_white_codes, CC_N_RUN_CODES, lane);
    cc_fill(L.bt, CC_BBITS, cc_black_codes, CC_N_RUN_CODES, lane);
    cc_fill(L.mt, CC_MBITS, cc_mode_codes, CC_N_MODE_CODES, lane);
    if (lane < 3) L.ce[0][lane] = (unsigned short)W;   // the imaginary white line above the first
    __syncthreads();
}

}  // namespace
