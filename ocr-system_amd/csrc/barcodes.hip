// Code 128, Code 39, EAN / UPC and ITF barcodes on the GPU (gfx950): the codes of a page as (x0, y0, x1, y1, kind, nsym, rows, flags) with their
// symbol values, in a canonical order.  Everything is integer and every reduction is order-free (min / max / add, first set bit of a
// ballot), so the lists equal the sequential definition restated in tests/barcode_reference.py (Code 128, Code 39) and
// tests/linear_reference.py (every kind).
//
// A row of a page is a list of runs; its ELEMENTS are the run widths (bars) and the gaps between them (spaces).  Read from bar t in
// direction d (+1 right, -1 left: a strip printed upside down), symbol k of a Code 128 is elements 6 k .. 6 k + 5 (bars t + 3 k d ..),
// of a Code 39 elements 10 k .. 10 k + 8 (bars t + 5 k d ..): where a symbol lies does not depend on what the symbols before it are,
// so the 64 lanes of the row's wave decode 64 symbols at once and ballots find the stop, the bad symbols and the checksum.  The same
// holds for the digits of an EAN-13, EAN-8 or UPC-E (four elements each at fixed offsets between the guards) and the pairs of an ITF
// (ten elements each); the kinds to read are a bit mask, and the set {Code 128, Code 39} is compiled in so that it pays for no other.
//
// All stream-ordered kernels, no host round trip:
//   1 ink_mask, ink_transpose            the mask (or the one the caller already has) and its transpose for the vertical codes
//   2 run_count / row_scan / run_fill    mask words -> run list [xs, xe] of every row (the shared kernels of runs.hip)
//   3 bc_rows    one wave per (page, row): lanes over runs test for starts (quiet zone, start pattern), then for each candidate in scan
//                order the wave decodes; a read claims its bars.  Going right, then going left; a read that shares a bar with one
//                already held is dropped; the four leftmost reads of the row go to the row's four slots
//   2-3 again on the transposed mask, rows and columns exchanged, into the slots behind the horizontal ones
//   4 bc_merge   one work-group per page: equal reads at most row_gap rows apart join (union-find over slots), hulls and counts are
//                accumulated at the roots, groups of min_rows reads are counted, gathered, rank-sorted by (y0, x0, y1, x1, slot)
#include "barcodes.h"
#include "barcode_tables.h"
#include "linear_tables.h"
#include "runs.h"

namespace {

typedef unsigned long long u64;
typedef unsigned short u16;

constexpr int C128_M = 11, C128_STOP = 106, C39_M = 15, C39_STAR = 43;

// the gap between bar a and the bar after it in direction d (b)
__device__ __forceinline__ int gap_of(int sa, int ea, int sb, int eb, int d) { return d > 0 ? sb - ea - 1 : sa - eb - 1; }

// the NB bars from bar j0 in direction d -> the 2 NB - 1 elements between the first and the last; false when a bar is off the row
template <int NB>
__device__ __forceinline__ bool load_elements(const u16* xs, const u16* xe, int n, int j0, int d, int (&w)[2 * NB - 1], int& s_last, int& e_last) {
    const int jl = j0 + d * (NB - 1);
    if (j0 < 0 || j0 >= n || jl < 0 || jl >= n) return false;
    int ps = xs[j0], pe = xe[j0];
#pragma unroll
    for (int i = 1; i < NB; ++i) {
        const int s = xs[j0 + d * i], e = xe[j0 + d * i];
        w[2 * i - 2] = pe - ps + 1;
        w[2 * i - 1] = gap_of(ps, pe, s, e, d);
        ps = s; pe = e;
    }
    w[2 * NB - 2] = pe - ps + 1;
    s_last = ps; e_last = pe;
    return true;
}

__device__ __forceinline__ int dist128(const int (&w)[6], int S, unsigned pat) {
    int dd = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) dd += iabs(w[i] * C128_M - (int)((pat >> (4 * i)) & 15u) * S);
    return dd;
}
__device__ __forceinline__ int dist39(const int (&w)[9], int S, unsigned pat) {
    int dd = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) dd += iabs(w[i] * C39_M - (int)(1u + 2u * ((pat >> i) & 1u)) * S);
    return dd;
}

// the gap before bar t (read in direction d) is quiet for a start symbol of S pixels and M modules; the page edge is quiet
__device__ __forceinline__ bool quiet_ok(const u16* xs, const u16* xe, int n, int t, int d, int S, int M, int quiet) {
    const int j = t - d;
    if (j < 0 || j >= n) return true;
    const int lo = j < t ? j : t;
    return ((int)xs[lo + 1] - (int)xe[lo] - 1) * M >= quiet * S;
}

// could a code start at bar t?  bit 0: a Code 128 start pattern lies within the bound, bit 1: Code 39's `*` does (what the decode asks
// of symbol 0, less the other patterns: a filter that lets every start through); kinds: the kinds asked for
__device__ __forceinline__ int start_filter(const u16* xs, const u16* xe, int n, int t, int d, int quiet, int max_dist, int kinds) {
    int out = 0, sl, el;
    int w9[9];
    if (kinds & 1) {
        int w[7];
        if (load_elements<4>(xs, xe, n, t, d, w, sl, el)) {
            int w6[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) w6[i] = w[i];
            const int S = w[0] + w[1] + w[2] + w[3] + w[4] + w[5];
            if (quiet_ok(xs, xe, n, t, d, S, C128_M, quiet)) {
                const int bound = max_dist * S * C128_M / 256;
                if (dist128(w6, S, BC_C128[103]) <= bound || dist128(w6, S, BC_C128[104]) <= bound || dist128(w6, S, BC_C128[105]) <= bound) out |= 1;
            }
        }
    }
    if ((kinds & 2) && load_elements<5>(xs, xe, n, t, d, w9, sl, el)) {
        int S = 0;
#pragma unroll
        for (int i = 0; i < 9; ++i) S += w9[i];
        if (quiet_ok(xs, xe, n, t, d, S, C39_M, quiet) && dist39(w9, S, BC_C39[C39_STAR]) <= max_dist * S * C39_M / 256) out |= 2;
    }
    return out;
}

// ---- EAN-13, EAN-8, UPC-E, ITF (kinds 2-5) ----
constexpr int EAN_M = 7;
template <int KIND> struct EanLayout;   // digits read, digits of the left half, first element of the centre guard (-1: none) and of the end guard, its elements, bars
template <> struct EanLayout<2> { static constexpr int nd = 12, nleft = 6, centre = 27, end = 56, nend = 3, bars = 30; };
template <> struct EanLayout<3> { static constexpr int nd = 8, nleft = 4, centre = 19, end = 40, nend = 3, bars = 22; };
template <> struct EanLayout<4> { static constexpr int nd = 6, nleft = 6, centre = -1, end = 27, nend = 6, bars = 17; };
template <int KIND>
__device__ __forceinline__ int ean_digit_at(int k) { return 3 + 4 * k + (EanLayout<KIND>::centre >= 0 && k >= EanLayout<KIND>::nleft ? 5 : 0); }

// element m read from bar t in direction d (its bars are on the row)
__device__ __forceinline__ int elem(const u16* xs, const u16* xe, int t, int d, int m) {
    const int j = t + d * (m >> 1);
    if (!(m & 1)) return (int)xe[j] - (int)xs[j] + 1;
    const int lo = d > 0 ? j : j - 1;
    return (int)xs[lo + 1] - (int)xe[lo] - 1;
}
template <int N>
__device__ __forceinline__ int elems(const u16* xs, const u16* xe, int t, int d, int m0, int (&w)[N]) {
    int S = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) { w[i] = elem(xs, xe, t, d, m0 + i); S += w[i]; }
    return S;
}
// N elements of one module each, by the measure
template <int N>
__device__ __forceinline__ bool units_ok(const int (&w)[N], int S, int max_dist) {
    int dd = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) dd += iabs(w[i] * N - S);
    return dd <= max_dist * S * N / 256;
}
// a guard of N elements from element m0, beside a digit of Sd pixels: N single modules, and N modules of the digit's within a quarter
template <int N>
__device__ __forceinline__ bool guard_ok(const u16* xs, const u16* xe, int t, int d, int m0, int Sd, int max_dist) {
    int w[N];
    const int G = elems<N>(xs, xe, t, d, m0, w);
    return units_ok<N>(w, G, max_dist) && 4 * iabs(EAN_M * G - N * Sd) <= N * Sd;
}

// could an EAN-13 / EAN-8 / UPC-E start at bar t?  Its bars are on the row, every guard holds and both ends are quiet: all a read
// asks but for the digits
template <int KIND>
__device__ __forceinline__ bool ean_filter(const u16* xs, const u16* xe, int n, int t, int d, int quiet, int max_dist) {
    typedef EanLayout<KIND> L;
    const int last = t + d * (L::bars - 1);
    if (last < 0 || last >= n) return false;
    int w[4];
    const int S0 = elems<4>(xs, xe, t, d, ean_digit_at<KIND>(0), w);
    if (!guard_ok<3>(xs, xe, t, d, 0, S0, max_dist) || !quiet_ok(xs, xe, n, t, d, S0, EAN_M, quiet)) return false;
    if (L::centre >= 0 && !guard_ok<5>(xs, xe, t, d, L::centre, elems<4>(xs, xe, t, d, ean_digit_at<KIND>(L::nleft - 1), w), max_dist)) return false;
    const int Sl = elems<4>(xs, xe, t, d, ean_digit_at<KIND>(L::nd - 1), w);
    return guard_ok<L::nend>(xs, xe, t, d, L::end, Sl, max_dist) && quiet_ok(xs, xe, n, last, -d, Sl, EAN_M, quiet);
}

// EAN-13 / EAN-8 / UPC-E from bar t (past ean_filter): lane k decodes digit k.  -> wave-uniform: true with symbol `lane` in v
template <int KIND>
__device__ __forceinline__ bool ean_decode(const u16* xs, const u16* xe, int t, int d, int max_dist, int lane, int& v) {
    typedef EanLayout<KIND> L;
    int w[4];
    const int S = elems<4>(xs, xe, t, d, ean_digit_at<KIND>(lane < L::nd ? lane : 0), w);
    const int np = lane < L::nleft ? BC_NEAN : 10;   // left half: sets L and G; right half: set R, which has L's widths
    int best = 0x7fffffff, bv = 0;
    for (int p = 0; p < BC_NEAN; ++p) {
        int dd = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) dd += iabs(w[i] * EAN_M - (int)((BC_EAN[p] >> (4 * i)) & 15u) * S);
        if (p < np && dd < best) { best = dd; bv = p; }
    }
    const bool ok = best <= max_dist * S * EAN_M / 256;
    const u64 all = (1ull << L::nd) - 1ull;
    if ((__ballot(ok) & all) != all) return false;
    const unsigned gmask = (unsigned)(__ballot(bv >= 10) & ((1ull << L::nleft) - 1ull));
    const int digit = bv >= 10 ? bv - 10 : bv;
    const int before = __shfl(digit, (lane + 63) & 63);
    if (KIND == 2) {   // the L / G pattern is the first digit; d0 + 3 d1 + d2 + .. + 3 d11 + d12 = 0 mod 10
        int first = -1;
        for (int r = 0; r < 10; ++r) if (BC_EAN13_PARITY[r] == gmask) first = r;
        if (first < 0) return false;
        if ((first + wave_sum(lane < 12 ? (lane & 1 ? 1 : 3) * digit : 0)) % 10 != 0) return false;
        v = lane == 0 ? first : before;
    } else if (KIND == 3) {
        if (gmask != 0u || wave_sum(lane < 8 ? (lane & 1 ? 1 : 3) * digit : 0) % 10 != 0) return false;
        v = digit;
    } else {   // the pattern is number system and check digit; the check is that of the UPC-A the six digits abbreviate
        int row = -1;
        for (int r = 0; r < BC_NUPCE; ++r) if (BC_UPCE_PARITY[r] == gmask) row = r;
        if (row < 0) return false;
        const int ns = row / 10, chk = row % 10;
        const int a = __shfl(digit, 0), b = __shfl(digit, 1), c = __shfl(digit, 2), e4 = __shfl(digit, 3), e5 = __shfl(digit, 4), f = __shfl(digit, 5);
        // ns a b f 0 0 | 0 0 c d e (f <= 2), ns a b c 0 0 | 0 0 0 d e (3), ns a b c d 0 | 0 0 0 0 e (4), ns a b c d e | 0 0 0 0 f: odd places weigh 3
        int sum;
        if (f <= 2) sum = 3 * (ns + b + c + e5) + a + f + e4;
        else if (f == 3) sum = 3 * (ns + b + e5) + a + c + e4;
        else if (f == 4) sum = 3 * (ns + b + e4 + e5) + a + c;
        else sum = 3 * (ns + b + e4 + f) + a + c + e5;
        if ((sum + chk) % 10 != 0) return false;
        v = lane == 0 ? ns : lane == 7 ? chk : before;
    }
    return true;
}

// could an ITF start at bar t?  Four single modules with a quiet gap before them
__device__ __forceinline__ bool itf_filter(const u16* xs, const u16* xe, int n, int t, int d, int quiet, int max_dist) {
    const int j2 = t + 2 * d;
    if (j2 < 0 || j2 >= n) return false;
    int w[4];
    const int S4 = elems<4>(xs, xe, t, d, 0, w);
    return units_ok<4>(w, S4, max_dist) && quiet_ok(xs, xe, n, t, d, S4, 4, quiet);
}

// the nearest of the ten two-of-five digits to a quintuple of S pixels at M half-modules (narrow 2, wide (M - 6) / 2) -> its distance
__device__ __forceinline__ int itf_best(const int (&w)[5], int S, int M, int& bv) {
    const int wide = (M - 6) / 2;
    int best = 0x7fffffff;
    bv = 0;
    for (int p = 0; p < 10; ++p) {
        int dd = 0;
#pragma unroll
        for (int i = 0; i < 5; ++i) dd += iabs(w[i] * M - (((BC_ITF[p] >> i) & 1u) ? wide : 2) * S);
        if (dd < best) { best = dd; bv = p; }
    }
    return best;
}

// ITF from bar t (past itf_filter): lane k decodes pair k with the three elements behind it, which are the stop when the code ends there.
// -> wave-uniform: true with symbol `lane` in v, the number of digits in nsym and the ITF-14 bit in f14
__device__ __forceinline__ bool itf_decode(const u16* xs, const u16* xe, int n, int t, int d, int quiet, int max_dist, int lane, int& v, int& nsym, int& f14) {
    const int j0 = t + d * (2 + 5 * lane), jl = j0 + 6 * d;   // the pair's five bars and the two behind them
    const bool there = lane < BARCODE_MAX_SYMS / 2 && j0 >= 0 && j0 < n && jl >= 0 && jl < n;
    int w[13], wb[5], ws[5], Sb = 0, Ss = 0;
#pragma unroll
    for (int i = 0; i < 13; ++i) w[i] = there ? elem(xs, xe, j0, d, i) : 1;
#pragma unroll
    for (int i = 0; i < 5; ++i) { wb[i] = w[2 * i]; ws[i] = w[2 * i + 1]; Sb += wb[i]; Ss += ws[i]; }
    if (!(__ballot(there) & 1ull)) return false;
    // the ratio: pair 0's bars at 14, 16, 18 half-modules, the distances brought to one scale (1008 = lcm); ties to the lower
    int tmp, M = 14;
    {
        const int s14 = itf_best(wb, Sb, 14, tmp) * 72, s16 = itf_best(wb, Sb, 16, tmp) * 63, s18 = itf_best(wb, Sb, 18, tmp) * 56;
        int sc = s14;
        if (s16 < sc) { sc = s16; M = 16; }
        if (s18 < sc) M = 18;
    }
    M = __shfl(M, 0);
    int w4[4];
    const int S4 = elems<4>(xs, xe, t, d, 0, w4), Sb0 = __shfl(Sb, 0);
    if (4 * iabs(S4 * M - 8 * Sb0) > 8 * Sb0) return false;   // the start is four narrow elements of pair 0's scale
    int db, ds;
    const bool pair_ok = there && itf_best(wb, Sb, M, db) <= max_dist * Sb * M / 256 && itf_best(ws, Ss, M, ds) <= max_dist * Ss * M / 256;
    const int Ms = M / 2 + 1, S3 = w[10] + w[11] + w[12];   // the stop: wide, narrow, narrow
    const int dist = iabs(w[10] * Ms - (Ms - 4) * S3) + iabs(w[11] * Ms - 2 * S3) + iabs(w[12] * Ms - 2 * S3);
    const bool stop = pair_ok && lane >= 2 && dist <= max_dist * S3 * Ms / 256 && 4 * iabs(S3 * M - Ms * Sb) <= Ms * Sb &&
                      quiet_ok(xs, xe, n, jl, -d, S3, Ms, 2 * quiet);
    const u64 stops = __ballot(stop);
    if (!stops) return false;
    const int kstop = __ffsll((long long)stops) - 1;
    const u64 below = (1ull << kstop) - 1ull;
    if ((__ballot(pair_ok) & below) != below) return false;
    nsym = 2 * kstop + 2;
    const int vb = __shfl(db, lane >> 1), vs = __shfl(ds, lane >> 1);
    v = lane & 1 ? vs : vb;
    f14 = nsym == 14 && wave_sum(lane < 14 ? (lane & 1 ? 1 : 3) * v : 0) % 10 == 0 ? 1 : 0;
    return true;
}

// Code 128 from bar t: lane k decodes symbol k.  -> wave-uniform: true with the lane's value in v and the stop's index in kstop
__device__ __forceinline__ bool decode128(const u16* xs, const u16* xe, int n, int t, int d, int max_dist, int lane, int& v, int& kstop) {
    int w7[7], sl, el;
    bool ok = load_elements<4>(xs, xe, n, t + d * 3 * lane, d, w7, sl, el);   // six elements and the bar behind them
    if (!ok) {
#pragma unroll
        for (int i = 0; i < 7; ++i) w7[i] = 1;
    }
    int w[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) w[i] = w7[i];
    const int S = w[0] + w[1] + w[2] + w[3] + w[4] + w[5], term = w7[6];
    int best = 0x7fffffff, bv = 0;
    for (int p = 0; p < BC_N128; ++p) {
        const int dd = dist128(w, S, BC_C128[p]);
        if (dd < best) { best = dd; bv = p; }
    }
    ok = ok && best <= max_dist * S * C128_M / 256;
    const u64 valid = __ballot(ok), stops = __ballot(ok && bv == C128_STOP);
    if (!stops) return false;
    kstop = __ffsll((long long)stops) - 1;
    if (kstop < 2) return false;
    const u64 below = (1ull << kstop) - 1ull;
    if ((valid & below) != below) return false;
    if (__ballot(lane < kstop && (lane == 0 ? (bv < 103 || bv > 105) : bv > 102))) return false;
    const bool term_ok = 3 * S <= 2 * term * C128_M && 2 * term * C128_M <= 5 * S;   // the stop's last bar: 1.5 .. 2.5 modules
    if (!((__ballot(term_ok) >> kstop) & 1ull)) return false;
    const int sum = wave_sum(lane < kstop - 1 ? (lane ? lane : 1) * bv : 0);
    if (sum % 103 != __shfl(bv, kstop - 1)) return false;
    v = bv;
    return true;
}

// Code 39 from bar t: lane k decodes character k
__device__ __forceinline__ bool decode39(const u16* xs, const u16* xe, int n, int t, int d, int max_dist, int lane, int& v, int& kstop) {
    int w[9], sl = 0, el = 0;
    const int j0 = t + d * 5 * lane;
    bool ok = load_elements<5>(xs, xe, n, j0, d, w, sl, el);
    if (!ok) {
#pragma unroll
        for (int i = 0; i < 9; ++i) w[i] = 1;
    }
    int S = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) S += w[i];
    bool gap_ok = false;   // the gap to the next character: there, and at most two modules
    const int j5 = j0 + 5 * d;
    if (ok && j5 >= 0 && j5 < n) gap_ok = gap_of(sl, el, xs[j5], xe[j5], d) * C39_M <= 2 * S;
    int best = 0x7fffffff, bv = 0;
    for (int p = 0; p < BC_N39; ++p) {
        const int dd = dist39(w, S, BC_C39[p]);
        if (dd < best) { best = dd; bv = p; }
    }
    ok = ok && best <= max_dist * S * C39_M / 256;
    const u64 stops = __ballot(ok && bv == C39_STAR && lane >= 1);
    if (!stops) return false;
    kstop = __ffsll((long long)stops) - 1;
    const u64 below = (1ull << kstop) - 1ull;   // (kstop >= 1)
    if ((__ballot(ok && gap_ok && (lane != 0 || bv == C39_STAR)) & below) != below) return false;
    v = bv;
    return true;
}

// 3: the reads of a row -> its slots.  slot = 4 * (row_base + row) + s of the page's slots_pp; hdr = a0, a1, kind | nsym << 8 | rev << 16 |
// ITF-14 << 17.  CK: the kinds as a constant (no code of another kind is compiled in), or -1 for kinds_rt
template <int CK>
__global__ __launch_bounds__(256) void bc_rows_kernel(const int* runoff, const u16* rxs, const u16* rxe, int H, size_t runcap, int quiet, int max_dist,
                                                      int row_base, int rows_pp, int* rowcnt, int4* hdr, int4* box, int* nreads, int* parent, uint8_t* syms8,
                                                      int rows_total, int kinds_rt) {
    const int kinds = CK >= 0 ? CK : kinds_rt;
    int pg, row, lane;
    if (!row_wave(H, rows_total, pg, row, lane)) return;
    const int* ro = runoff + (size_t)pg * (H + 1);
    const int r0 = ro[row], n = ro[row + 1] - r0;
    const size_t prow = (size_t)pg * rows_pp + row_base + row;
    if (n < 10) {   // the shortest code has ten bars
        if (lane == 0) rowcnt[prow] = 0;
        return;
    }
    const u16* xs = rxs + (size_t)pg * runcap + r0;
    const u16* xe = rxe + (size_t)pg * runcap + r0;
    // the row's reads, by x0 (wave-uniform but for lv, the lane's symbol value)
    int lx0[BARCODE_ROW_READS], lx1[BARCODE_ROW_READS], lmeta[BARCODE_ROW_READS], lv[BARCODE_ROW_READS], cnt = 0;
#pragma unroll
    for (int s = 0; s < BARCODE_ROW_READS; ++s) { lx0[s] = 0; lx1[s] = 0; lmeta[s] = 0; lv[s] = 0; }
    for (int pass = 0; pass < 2; ++pass) {
        const int d = pass ? -1 : 1;
        int free = 0;   // in scan order: the first position no read has claimed
        for (int i0 = 0; i0 < n; i0 += 64) {
            if (pass == 0 && cnt == BARCODE_ROW_READS) break;   // going right the reads come leftmost first: four fill the row
            const int pos = i0 + lane;
            int c = pos < n ? start_filter(xs, xe, n, d > 0 ? pos : n - 1 - pos, d, quiet, max_dist, kinds) : 0;
            if (CK < 0 && pos < n) {
                const int t = d > 0 ? pos : n - 1 - pos;
                if ((kinds & 4) && ean_filter<2>(xs, xe, n, t, d, quiet, max_dist)) c |= 4;
                if ((kinds & 8) && ean_filter<3>(xs, xe, n, t, d, quiet, max_dist)) c |= 8;
                if ((kinds & 16) && ean_filter<4>(xs, xe, n, t, d, quiet, max_dist)) c |= 16;
                if ((kinds & 32) && itf_filter(xs, xe, n, t, d, quiet, max_dist)) c |= 32;
            }
            u64 todo = __ballot(c != 0);
            while (todo) {   // wave-uniform: every lane works on the candidate of lane `src`
                const int src = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const int p = i0 + src;
                if (p < free) continue;
                const int t = d > 0 ? p : n - 1 - p, cs = __shfl(c, src);
                int v = 0, kstop = 0, kind = 0, bars = 0, nsym = 0, f14 = 0;
                bool got = false;
                if (cs & 1) { got = decode128(xs, xe, n, t, d, max_dist, lane, v, kstop); bars = 3 * kstop + 4; nsym = kstop + 1; }
                if (!got && (cs & 2)) { got = decode39(xs, xe, n, t, d, max_dist, lane, v, kstop); kind = 1; bars = 5 * kstop + 5; nsym = kstop + 1; }
                if (CK < 0) {
                    if (!got && (cs & 4)) { got = ean_decode<2>(xs, xe, t, d, max_dist, lane, v); kind = 2; bars = EanLayout<2>::bars; nsym = 13; }
                    if (!got && (cs & 8)) { got = ean_decode<3>(xs, xe, t, d, max_dist, lane, v); kind = 3; bars = EanLayout<3>::bars; nsym = 8; }
                    if (!got && (cs & 16)) { got = ean_decode<4>(xs, xe, t, d, max_dist, lane, v); kind = 4; bars = EanLayout<4>::bars; nsym = 8; }
                    if (!got && (cs & 32)) { got = itf_decode(xs, xe, n, t, d, quiet, max_dist, lane, v, nsym, f14); kind = 5; bars = 5 * (nsym / 2) + 4; }
                }
                if (!got) continue;
                free = p + bars;
                const int last = t + d * (bars - 1);   // (on the row: the decode saw every bar)
                const int x0 = xs[t < last ? t : last], x1 = xe[t < last ? last : t];
                bool clash = false;
                int at = 0;
#pragma unroll
                for (int s = 0; s < BARCODE_ROW_READS; ++s)
                    if (s < cnt) { clash = clash || (x0 <= lx1[s] && lx0[s] <= x1); at += lx0[s] < x0 ? 1 : 0; }
                if (clash || at >= BARCODE_ROW_READS) continue;
#pragma unroll
                for (int s = BARCODE_ROW_READS - 1; s >= 1; --s)
                    if (s > at) { lx0[s] = lx0[s - 1]; lx1[s] = lx1[s - 1]; lmeta[s] = lmeta[s - 1]; lv[s] = lv[s - 1]; }
#pragma unroll
                for (int s = 0; s < BARCODE_ROW_READS; ++s)
                    if (s == at) { lx0[s] = x0; lx1[s] = x1; lmeta[s] = kind | (nsym << 8) | (pass << 16) | (f14 << 17); lv[s] = v; }
                if (cnt < BARCODE_ROW_READS) ++cnt;
                if (pass == 0 && cnt == BARCODE_ROW_READS) todo = 0;
            }
        }
    }
    if (lane == 0) rowcnt[prow] = cnt;
#pragma unroll
    for (int s = 0; s < BARCODE_ROW_READS; ++s) {
        if (s < cnt) {
            const int slot = 4 * (row_base + row) + s;
            const size_t gi = (size_t)pg * rows_pp * 4 + slot;
            if (lane == 0) {
                hdr[gi] = make_int4(lx0[s], lx1[s], lmeta[s], 0);
                box[gi] = make_int4(lx0[s], lx1[s], row, row);
                nreads[gi] = 1;
                parent[gi] = slot;
            }
            syms8[gi * BARCODE_MAX_SYMS + lane] = (uint8_t)(lane < ((lmeta[s] >> 8) & 255) ? lv[s] : 0);
        }
    }
}

// the used slots of a page, thread by thread: f(slot, row of the page's H + W, first row of the slot's direction)
template <class F>
__device__ __forceinline__ void for_slots(const int* rowcnt, int H, int rows_pp, F f) {
    for (int r = threadIdx.x; r < rows_pp; r += 256) {
        const int c = rowcnt[r];
        for (int s = 0; s < c; ++s) f(4 * r + s, r, r < H ? 0 : H);
    }
}

// 4: tmp [B][max_codes][9] = y0, x0, y1, x1, slot, kind, nsym, rows, flags
__global__ __launch_bounds__(256) void bc_merge_kernel(const int* rowcnt_all, const int4* hdr_all, int4* box_all, int* nreads_all, int* parent_all,
                                                       const uint8_t* syms8_all, int H, int rows_pp, int min_rows, int row_gap, int max_codes, int* tmp_all,
                                                       int* counts, int* codes, int* syms) {
    __shared__ int s_key[BARCODE_MAX_CODES * 5];
    __shared__ int s_n;
    const int pg = blockIdx.x;
    const size_t sb = (size_t)pg * rows_pp * 4;
    const int* rowcnt = rowcnt_all + (size_t)pg * rows_pp;
    const int4* hdr = hdr_all + sb;
    int4* box = box_all + sb;
    int* nreads = nreads_all + sb;
    int* parent = parent_all + sb;
    const unsigned* sym32 = reinterpret_cast<const unsigned*>(syms8_all + sb * BARCODE_MAX_SYMS);   // 16 words a slot
    int* tmp = tmp_all + (size_t)pg * max_codes * 9;
    if (threadIdx.x == 0) s_n = 0;
    // equal reads of nearby rows join
    for_slots(rowcnt, H, rows_pp, [&](int slot, int r, int first) {
        const int4 a = hdr[slot];
        for (int dy = 1; dy <= row_gap && r - dy >= first; ++dy) {
            const int r2 = r - dy, c2 = rowcnt[r2];
            for (int s2 = 0; s2 < c2; ++s2) {
                const int other = 4 * r2 + s2;
                const int4 b = hdr[other];
                if (a.z != b.z || a.x > b.y || b.x > a.y) continue;
                bool same = true;
                for (int i = 0; i < BARCODE_MAX_SYMS / 4; ++i) same = same && sym32[(size_t)slot * 16 + i] == sym32[(size_t)other * 16 + i];
                if (same) uf_union(parent, slot, other);
            }
        }
    });
    __syncthreads();
    // hull and number of reads at the root (the root holds its own)
    for_slots(rowcnt, H, rows_pp, [&](int slot, int r, int first) {
        const int root = uf_find(parent, slot);
        if (root == slot) return;
        const int4 a = hdr[slot];
        int* b = reinterpret_cast<int*>(box + root);
        atomicMin(b + 0, a.x); atomicMax(b + 1, a.y); atomicMin(b + 2, r - first); atomicMax(b + 3, r - first);
        atomicAdd(nreads + root, 1);
    });
    __syncthreads();
    for_slots(rowcnt, H, rows_pp, [&](int slot, int r, int first) {
        if (parent[slot] != slot || nreads[slot] < min_rows) return;
        const int idx = atomicAdd(&s_n, 1);
        if (idx >= max_codes) return;
        const int4 a = hdr[slot], b = box[slot];
        const bool vertical = first != 0;
        int* o = tmp + (size_t)idx * 9;
        o[0] = vertical ? b.x : b.z; o[1] = vertical ? b.z : b.x; o[2] = vertical ? b.y : b.w; o[3] = vertical ? b.w : b.y; o[4] = slot;
        o[5] = a.z & 255; o[6] = (a.z >> 8) & 255; o[7] = nreads[slot]; o[8] = ((a.z >> 16) & 1) | (vertical ? 2 : 0) | (((a.z >> 17) & 1) << 2);
    });
    __syncthreads();
    const int n = s_n;
    if (threadIdx.x == 0) counts[pg] = n;
    if (n > max_codes) return;   // overflow: the count is all that is reported
    int* out = codes + (size_t)pg * max_codes * 8;
    int* osym = syms + (size_t)pg * max_codes * BARCODE_MAX_SYMS;
    const uint8_t* s8 = syms8_all + sb * BARCODE_MAX_SYMS;
    rank_sort<5>(s_key, tmp, 9, n, [=](int i, int rank, const int (&k)[5]) {
        int* o = out + (size_t)rank * 8;
        o[0] = k[1]; o[1] = k[0]; o[2] = k[3]; o[3] = k[2];
        o[4] = tmp[i * 9 + 5]; o[5] = tmp[i * 9 + 6]; o[6] = tmp[i * 9 + 7]; o[7] = tmp[i * 9 + 8];
        for (int j = 0; j < BARCODE_MAX_SYMS; ++j) osym[(size_t)rank * BARCODE_MAX_SYMS + j] = s8[(size_t)k[4] * BARCODE_MAX_SYMS + j];
    });
}

}  // namespace

// the workspace's regions: one layout sizes it (barcodes_workspace_bytes) and carves it (barcodes_launch)
struct BarcodeWorkspace {
    unsigned long long *mask, *vmask; int* runoff; unsigned short *rxs, *rxe; int* run_parent;
    int* rowcnt; int4 *hdr, *box; int *nreads, *parent; uint8_t* syms8; int* tmp;
};
static BarcodeWorkspace barcodes_layout(Arena& a, int B, int H, int W, int max_codes) {
    const size_t nw = (W + 63) / 64, nhw = (H + 63) / 64, side = H > W ? H : W, runcap = run_cap(H, W) > run_cap(W, H) ? run_cap(H, W) : run_cap(W, H);
    const size_t slots = (size_t)B * ((size_t)H + W) * BARCODE_ROW_READS;
    BarcodeWorkspace w;
    w.mask = a.take<unsigned long long>((size_t)B * H * nw);
    w.vmask = a.take<unsigned long long>((size_t)B * W * nhw);
    w.runoff = a.take<int>((size_t)B * (side + 1));   // run counts -> offsets, of one direction at a time (as the run list below)
    w.rxs = a.take<unsigned short>((size_t)B * runcap); w.rxe = a.take<unsigned short>((size_t)B * runcap);
    w.run_parent = a.take<int>((size_t)B * runcap);   // (run_fill's; the pass joins reads, not runs)
    w.rowcnt = a.take<int>((size_t)B * ((size_t)H + W));   // reads of every row, then of every column
    w.hdr = a.take<int4>(slots); w.box = a.take<int4>(slots);
    w.nreads = a.take<int>(slots); w.parent = a.take<int>(slots);
    w.syms8 = a.take<uint8_t>(slots * BARCODE_MAX_SYMS);
    w.tmp = a.take<int>((size_t)B * max_codes * 9);
    return w;
}

static bool barcodes_args_ok(int B, int H, int W, int max_codes) {
    if (B <= 0 || H <= 0 || W <= 0 || H > 65535 || W > 65535 || max_codes < 1 || max_codes > BARCODE_MAX_CODES) return false;
    return (size_t)B * H < (1ull << 31) && (size_t)B * W < (1ull << 31) && run_cap(H, W) < (1ull << 31) && run_cap(W, H) < (1ull << 31);
}

bool barcode_params_ok(int quiet, int max_dist, int min_rows, int row_gap, int max_codes) {
    return quiet >= 0 && quiet <= BARCODE_MAX_QUIET && max_dist >= 0 && max_dist <= BARCODE_MAX_DIST && min_rows >= 1 && row_gap >= 1 &&
           row_gap <= BARCODE_MAX_ROW_GAP && max_codes >= 1 && max_codes <= BARCODE_MAX_CODES;
}

bool barcode_kinds_ok(int kinds) { return kinds > 0 && kinds <= BARCODE_KINDS_ALL; }

size_t barcodes_workspace_bytes(int B, int H, int W, int max_codes) {
    if (!barcodes_args_ok(B, H, W, max_codes)) return 0;
    Arena a;
    barcodes_layout(a, B, H, W, max_codes);
    return a.off;
}

hipError_t barcodes_launch(const BarcodeParams& p, void* workspace, size_t ws_bytes, hipStream_t st) {
    const int B = p.B, H = p.H, W = p.W;
    if (!barcodes_args_ok(B, H, W, p.max_codes) || !barcode_params_ok(p.quiet, p.max_dist, p.min_rows, p.row_gap, p.max_codes)) return hipErrorInvalidValue;
    if (!p.rgb || !p.codes || !p.syms || !p.counts || !barcode_kinds_ok(p.kinds)) return hipErrorInvalidValue;
    Arena a(workspace, ws_bytes);
    const BarcodeWorkspace w = barcodes_layout(a, B, H, W, p.max_codes);
    if (a.overflow) return hipErrorOutOfMemory;
    const int nw = (W + 63) / 64, nhw = (H + 63) / 64, rows_pp = H + W;
    const size_t runcap = run_cap(H, W) > run_cap(W, H) ? run_cap(H, W) : run_cap(W, H);
    const unsigned long long* mask;
    hipError_t e;
    if ((e = ink_mask_resolve(p.rgb, p.mask_in, p.mask_out, w.mask, B, H, W, p.threshold, st, &mask)) != hipSuccess) return e;
    if ((e = ink_transpose_launch(mask, w.vmask, B, H, W, st)) != hipSuccess) return e;
    for (int dir = 0; dir < 2; ++dir) {   // rows, then columns as the rows of the transpose; the run list is one direction's at a time
        const unsigned long long* m = dir ? w.vmask : mask;
        const int R = dir ? W : H, words = dir ? nhw : nw;
        run_count_launch(m, w.runoff, B, R, words, st);
        row_scan_launch(w.runoff, nullptr, B, R, st);
        run_fill_launch(m, w.runoff, w.rxs, w.rxe, w.run_parent, nullptr, B, R, words, runcap, st);
        hipLaunchKernelGGL(p.kinds == BARCODE_KINDS_DEFAULT ? bc_rows_kernel<BARCODE_KINDS_DEFAULT> : bc_rows_kernel<-1>, row_wave_grid(B * R), dim3(256), 0, st,
                           w.runoff, w.rxs, w.rxe, R, runcap, p.quiet, p.max_dist, dir ? H : 0, rows_pp, w.rowcnt, w.hdr, w.box, w.nreads, w.parent, w.syms8,
                           B * R, p.kinds);
    }
    hipLaunchKernelGGL(bc_merge_kernel, dim3(B), dim3(256), 0, st, w.rowcnt, w.hdr, w.box, w.nreads, w.parent, w.syms8, H, rows_pp, p.min_rows, p.row_gap,
                       p.max_codes, w.tmp, p.counts, p.codes, p.syms);
    return hipGetLastError();
}
