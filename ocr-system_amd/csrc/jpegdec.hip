// Baseline JPEG decoder on the device (jpegdec.h): what the reference's Image.open(...) does for .jpg inputs
// (/root/reference/backend/utils/image_preprocessing.py:57-75), byte-identical to Pillow / libjpeg-turbo.
//
// A JPEG scan is ONE sequential bit stream per file (no restart markers in what Pillow, scanners' firmware or this engine's own
// encoder write by default), so the entropy decode is made parallel the way self-synchronising Huffman streams allow:
//   1. un-stuff: the 0xFF00 pairs and RSTn markers leave the stream (three byte-parallel kernels: mark / scan / compact); the RSTn
//      positions become a segment table (a segment start is an exact synchronisation point: byte aligned, state reset);
//   2. the clean stream is cut into 256-byte chunks, one thread each.  A chunk's decoder state is (bit position, block-in-MCU,
//      coefficient index).  Pass 0 decodes every chunk from a GUESSED state (its first bit, block 0, DC next); wrong guesses
//      re-synchronise with the true decode inside the chunk most of the time (Huffman codes self-synchronise within a few symbols,
//      the coefficient index at the next end-of-block, the block phase after a few table switches).  Pass j >= 1 starts chunk i from
//      chunk i-1's end state of pass j-1 and re-decodes only if that differs from what it started from before: a Jacobi iteration
//      whose fixed point IS the sequential decode (chunk 0 starts exact; by induction every chunk does).  Typically 2-4 passes;
//   3. a last pass writes the quantised coefficients (block indices from a prefix sum of the per-chunk DC counts), DC differences
//      are integrated per component (segmented by restart interval), then inverse DCT ("islow" integer), fancy chroma up-sampling
//      and YCbCr -> RGB are embarrassingly parallel kernels.
// Header parsing (a few hundred bytes of markers) is host code.
// Progressive files (SOF2, jpegdec_run_progressive) reuse stages 1 and 3; their entropy stage is the jp_* kernels further down: every scan
// is one un-stuffed stream, first scans decode in one round, refinement scans after them in file order.
#include "jpegdec.h"

#include <cstring>
#include <vector>

#include "engine.h"

namespace {

constexpr int JD_CH = 1024;     // clean-stream bytes per chunk (256: a busy A4 page holds ~3 MCUs per chunk and only 36 % of the guessed starts re-synchronise inside it: 28 passes; 1024: 8)
constexpr int JD_UB = 1024;     // raw bytes per un-stuff block (256 threads x 4)
constexpr int JD_PASSES = 4;    // synchronisation passes between two looks at the "changed" flags

struct JdHuff { int maxcode[17]; int valptr[17]; unsigned short fast[256]; unsigned char vals[256]; };   // fast[8 bits] = len << 8 | symbol for codes of <= 8 bits, else 0
struct JdFile {
    unsigned raw_off, raw_len, clean_off, ublk_off, nublk, chunk_off, nchunk_cap, seg_off, seg_cap, coef_off, plane_off[3];
    int width, height, ncomp, hs, vs, mcux, mcuy, bpm, restart, nblk, valid;
    int pw[3], ph[3], comp_of_blk[6], first_blk_of_comp[3], td[3], ta[3];
    unsigned short q[3][64];
    JdHuff dc[3], ac[3];
};
struct JdDyn { unsigned clean_len; int nseg; int err; int total_dc; };   // per file, written on the device

__constant__ unsigned char JD_ZZ[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48,
                                        41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22,
                                        15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
const unsigned char H_ZZ[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48,
                                41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22,
                                15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// ------------------------------------------------------------------------------------------------ 1. un-stuff
__device__ __forceinline__ bool jd_is_rst(unsigned char c) { return (c & 0xF8) == 0xD0; }
// raw byte j leaves the stream: a stuffed zero, or either byte of an RSTn marker
__device__ __forceinline__ bool jd_drop(const unsigned char* raw, unsigned j, unsigned len) {
    const unsigned char c = raw[j];
    if (c == 0x00) return j > 0 && raw[j - 1] == 0xFF;
    if (c == 0xFF) return j + 1 < len && jd_is_rst(raw[j + 1]);
    return jd_is_rst(c) && j > 0 && raw[j - 1] == 0xFF;
}
__device__ __forceinline__ bool jd_marker_start(const unsigned char* raw, unsigned j, unsigned len) {
    return raw[j] == 0xFF && j + 1 < len && jd_is_rst(raw[j + 1]);
}

__global__ __launch_bounds__(256) void jd_mark_kernel(const JdFile* files, const unsigned char* rawbuf, int* blk_keep, int* blk_rst) {
    const JdFile& F = files[blockIdx.y];
    if (!F.valid || blockIdx.x >= F.nublk) return;
    __shared__ int sk, sr;
    if (threadIdx.x == 0) { sk = 0; sr = 0; }
    __syncthreads();
    const unsigned char* raw = rawbuf + F.raw_off;
    int k = 0, r = 0;
    for (int e = 0; e < 4; ++e) {
        const unsigned j = blockIdx.x * JD_UB + threadIdx.x * 4 + e;
        if (j >= F.raw_len) break;
        k += jd_drop(raw, j, F.raw_len) ? 0 : 1;
        r += jd_marker_start(raw, j, F.raw_len) ? 1 : 0;
    }
    if (k) atomicAdd(&sk, k);
    if (r) atomicAdd(&sr, r);
    __syncthreads();
    if (threadIdx.x == 0) { blk_keep[F.ublk_off + blockIdx.x] = sk; blk_rst[F.ublk_off + blockIdx.x] = sr; }
}

// exclusive scan of n ints by one 256-thread workgroup (in place)
__device__ void jd_block_scan(int* a, int n) {
    __shared__ int part[256];
    const int t = threadIdx.x, per = (n + 255) / 256, lo = t * per, hi = min(lo + per, n);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += a[i];
    part[t] = s;
    __syncthreads();
    if (t == 0) { int c = 0; for (int i = 0; i < 256; ++i) { const int v = part[i]; part[i] = c; c += v; } }
    __syncthreads();
    int c = part[t];
    for (int i = lo; i < hi; ++i) { const int v = a[i]; a[i] = c; c += v; }
    __syncthreads();
}

__global__ __launch_bounds__(256) void jd_scan_kernel(const JdFile* files, int* blk_keep, int* blk_rst, JdDyn* dyn) {
    const JdFile& F = files[blockIdx.x];
    if (!F.valid) return;
    __shared__ int tk, tr;
    int* k = blk_keep + F.ublk_off;
    int* r = blk_rst + F.ublk_off;
    const int n = (int)F.nublk;
    if (threadIdx.x == 0) {   // totals first (the scans below overwrite the counts)
        tk = 0; tr = 0;
    }
    __syncthreads();
    int sk = 0, sr = 0;
    for (int i = threadIdx.x; i < n; i += 256) { sk += k[i]; sr += r[i]; }
    if (sk) atomicAdd(&tk, sk);
    if (sr) atomicAdd(&tr, sr);
    __syncthreads();
    const int total_k = tk, total_r = tr;
    jd_block_scan(k, n);
    jd_block_scan(r, n);
    if (threadIdx.x == 0) {
        dyn[blockIdx.x].clean_len = (unsigned)total_k;
        // exactly one marker between two restart intervals: a missing, extra or empty segment is corrupt
        dyn[blockIdx.x].nseg = total_r != (F.seg_cap ? (int)F.seg_cap - 1 : 0) ? -1 : total_r;
        dyn[blockIdx.x].err = 0;
        dyn[blockIdx.x].total_dc = 0;
    }
}

__global__ __launch_bounds__(256) void jd_compact_kernel(const JdFile* files, const unsigned char* rawbuf, const int* blk_keep, const int* blk_rst,
                                                         JdDyn* dyn, unsigned char* cleanbuf, unsigned* seg_start) {
    const JdFile& F = files[blockIdx.y];
    if (!F.valid || blockIdx.x >= F.nublk) return;
    __shared__ int wk[4], wr[4];
    const unsigned char* raw = rawbuf + F.raw_off;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool keep[4], mark[4];
    int k = 0, r = 0;
    for (int e = 0; e < 4; ++e) {
        const unsigned j = blockIdx.x * JD_UB + threadIdx.x * 4 + e;
        keep[e] = j < F.raw_len && !jd_drop(raw, j, F.raw_len);
        mark[e] = j < F.raw_len && jd_marker_start(raw, j, F.raw_len);
        k += keep[e]; r += mark[e];
    }
    // exclusive scan over the 256 threads: wave scan by shuffles, wave totals through LDS
    int ik = k, ir = r;
    for (int d = 1; d < 64; d <<= 1) {
        const int a = __shfl_up(ik, d), b = __shfl_up(ir, d);
        if (lane >= d) { ik += a; ir += b; }
    }
    if (lane == 63) { wk[wave] = ik; wr[wave] = ir; }
    __syncthreads();
    int bk = 0, br = 0;
    for (int w = 0; w < wave; ++w) { bk += wk[w]; br += wr[w]; }
    int pk = blk_keep[F.ublk_off + blockIdx.x] + bk + ik - k;     // clean index of this thread's first kept byte
    int pr = blk_rst[F.ublk_off + blockIdx.x] + br + ir - r;
    unsigned char* clean = cleanbuf + F.clean_off;
    const int nseg = dyn[blockIdx.y].nseg;
    for (int e = 0; e < 4; ++e) {
        const unsigned j = blockIdx.x * JD_UB + threadIdx.x * 4 + e;
        if (mark[e] && nseg >= 0 && pr < (int)F.seg_cap) seg_start[F.seg_off + pr] = (unsigned)pk;   // the segment after this marker starts at the next kept byte
        if (mark[e] && raw[j + 1] != 0xD0 + (pr & 7)) dyn[blockIdx.y].err = 1;                        // RSTn out of sequence
        pr += mark[e];
        if (keep[e]) clean[pk] = raw[j];
        pk += keep[e];
    }
}

// ------------------------------------------------------------------------------------------------ 2. parallel Huffman decode
struct JdRd {   // bit reader over the clean stream: acc holds `have` valid bits, MSB first, starting at stream bit `pos`
    const unsigned* w; unsigned pos; unsigned long long acc; int have;
};
__device__ __forceinline__ void jd_seek(JdRd& r, unsigned pos) {
    const unsigned byte = pos >> 3, wi = byte >> 2, sh = (byte & 3) * 8 + (pos & 7);
    const unsigned a = __builtin_bswap32(r.w[wi]), b = __builtin_bswap32(r.w[wi + 1]), c = __builtin_bswap32(r.w[wi + 2]);
    const unsigned long long hi = ((unsigned long long)a << 32) | b;
    r.acc = sh ? (hi << sh) | ((unsigned long long)c >> (32 - sh)) : hi;
    r.have = 64; r.pos = pos;
}
__device__ __forceinline__ unsigned jd_peek(JdRd& r, int n) {   // 1 <= n <= 32
    if (r.have < n) jd_seek(r, r.pos);
    return (unsigned)(r.acc >> (64 - n));
}
__device__ __forceinline__ void jd_skip(JdRd& r, int n) { r.acc <<= n; r.have -= n; r.pos += (unsigned)n; }
// -> symbol, or -1 (no code matches: corrupt data or a decoder that is not synchronised); always consumes at least one bit
__device__ __forceinline__ int jd_sym(JdRd& r, const JdHuff& t) {
    const unsigned p16 = jd_peek(r, 16);
    const unsigned f = t.fast[p16 >> 8];
    if (f) { jd_skip(r, (int)(f >> 8)); return (int)(f & 255u); }
    for (int l = 9; l <= 16; ++l) {
        const int code = (int)(p16 >> (16 - l));
        if (code <= t.maxcode[l]) { jd_skip(r, l); return t.vals[(t.valptr[l] + code) & 255]; }
    }
    jd_skip(r, 16);
    return -1;
}
__device__ __forceinline__ int jd_extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// Decodes from state (pos, b, k) until the first symbol boundary at or beyond end_bit (or the end of the stream).
// WRITE: stores the coefficients (DC as a difference) — blk = index of the block in progress (k > 0) or of the next block (k == 0).
template <bool WRITE>
__device__ void jd_span(const JdFile& F, const unsigned* clean_w, unsigned total_bits, const unsigned* seg, int nseg, unsigned pos, int b, int k,
                        unsigned end_bit, unsigned* out_pos, int* out_bk, int* out_ndc, short* coef, int blk, int* err) {
    JdRd r; r.w = clean_w; r.have = 0; r.pos = pos; r.acc = 0;
    // the segment (restart interval) the position lies in: seg[s] = byte offset where segment s + 1 starts
    int s = 0;
    { int lo = 0, hi = nseg; while (lo < hi) { const int mid = (lo + hi) >> 1; if (seg[mid] * 8u <= pos) lo = mid + 1; else hi = mid; } s = lo; }
    unsigned seg_end = s < nseg ? seg[s] * 8u : total_bits;
    // WRITE: every segment holds exactly `restart` MCUs (the last one the rest) and its data ends with them — the next block at a
    // segment start is s * restart MCUs in, at block 0 of an MCU, and no symbol is cut short by the end of the data
    const int seg_blks = F.restart * F.bpm;
    if (WRITE && s > 0 && pos == seg[s - 1] * 8u && (b != 0 || k != 0 || blk != s * seg_blks)) *err = 1;
    int ndc = 0;
    int cur = k > 0 ? blk - 1 : blk;   // block whose AC coefficients are being written
    if (!WRITE) (void)cur;
    while (r.pos < end_bit) {
        const unsigned rem = seg_end - r.pos;
        if (rem < 8u) {   // inside the last byte of a segment: 1-bits up to its end are padding (no Huffman code is all ones, and no symbol crosses a marker)
            bool pad = rem == 0u;
            if (!pad) pad = jd_peek(r, (int)rem) == ((1u << rem) - 1u);
            if (pad) {
                if (WRITE && (b != 0 || k != 0 || (seg_end < total_bits && blk + ndc != (s + 1) * seg_blks))) *err = 1;
                if (seg_end >= total_bits) { r.pos = total_bits; b = 0; k = 0; break; }
                r.pos = seg_end; r.have = 0; b = 0; k = 0;
                ++s; seg_end = s < nseg ? seg[s] * 8u : total_bits;
                continue;
            }
        }
        const int comp = F.comp_of_blk[b];
        if (k == 0) {
            int sym = jd_sym(r, F.dc[F.td[comp]]);
            if (sym < 0 || sym > 11) { if (WRITE) *err = 1; sym = 0; }
            int diff = 0;
            if (sym) { diff = jd_extend((int)jd_peek(r, sym), sym); jd_skip(r, sym); }
            if (WRITE) { cur = blk + ndc; if (cur < F.nblk) coef[(size_t)cur * 64] = (short)diff; else *err = 1; }
            ++ndc; k = 1;
        } else {
            const int rs = jd_sym(r, F.ac[F.ta[comp]]);
            bool end_block = false;
            if (rs < 0) { if (WRITE) *err = 1; end_block = true; }
            else {
                const int run = rs >> 4, sz = rs & 15;
                if (sz == 0) {
                    if (run == 15) { k += 16; if (k > 63) { end_block = true; if (WRITE && k > 64) *err = 1; } }
                    else end_block = true;
                } else {
                    k += run;
                    const int v = jd_extend((int)jd_peek(r, sz), sz);
                    jd_skip(r, sz);
                    if (k > 63) { if (WRITE) *err = 1; end_block = true; }
                    else {
                        if (WRITE && cur >= 0 && cur < F.nblk) coef[(size_t)cur * 64 + JD_ZZ[k]] = (short)v;
                        if (++k > 63) end_block = true;
                    }
                }
            }
            if (end_block) { k = 0; b = b + 1 == F.bpm ? 0 : b + 1; }
        }
        if (r.pos > seg_end) {   // a symbol ran over a segment boundary: only a decoder that is not synchronised (or a corrupt file) gets here
            if (WRITE) *err = 1;
            if (seg_end >= total_bits) { r.pos = total_bits; b = 0; k = 0; break; }
            r.pos = seg_end; r.have = 0; b = 0; k = 0;
            ++s; seg_end = s < nseg ? seg[s] * 8u : total_bits;
        }
    }
    if (WRITE && r.pos >= total_bits && (b != 0 || k != 0)) *err = 1;   // the data ran out inside a block
    *out_pos = r.pos; *out_bk = (b << 8) | k; *out_ndc = ndc;
}

struct JdChunks { unsigned* start_pos; int* start_bk; unsigned* end_pos[2]; int* end_bk[2]; int* ndc; int* first_blk; };

__global__ __launch_bounds__(64) void jd_sync_kernel(const JdFile* files, const JdDyn* dyn, const unsigned char* cleanbuf, const unsigned* seg_start, JdChunks C,
                                                     int pass, int* changed /* [file] of this pass */) {
    const JdFile& F = files[blockIdx.y];
    const JdDyn& D = dyn[blockIdx.y];
    if (!F.valid || D.nseg < 0) return;
    const unsigned i = blockIdx.x * 64 + threadIdx.x;
    const unsigned nchunks = (D.clean_len + JD_CH - 1) / JD_CH;
    if (i >= nchunks) return;
    const unsigned ci = F.chunk_off + i;
    const int src = pass & 1, dst = src ^ 1;   // pass j reads end[j & 1] (written by pass j - 1), writes end[(j & 1) ^ 1]
    unsigned pos; int bk;
    if (i == 0) { pos = 0; bk = 0; }
    else if (pass == 0) { pos = i * (JD_CH * 8u); bk = 0; }
    else { pos = C.end_pos[src][ci - 1]; bk = C.end_bk[src][ci - 1]; }
    if (pass > 0 && pos == C.start_pos[ci] && bk == C.start_bk[ci]) {   // same start as before: same end
        C.end_pos[dst][ci] = C.end_pos[src][ci]; C.end_bk[dst][ci] = C.end_bk[src][ci];
        return;
    }
    C.start_pos[ci] = pos; C.start_bk[ci] = bk;
    const unsigned total_bits = D.clean_len * 8u;
    unsigned end_bit = (i + 1) * (JD_CH * 8u);
    if (end_bit > total_bits) end_bit = total_bits;
    unsigned op = pos; int obk = bk, ondc = 0, err = 0;
    if (pos < end_bit)
        jd_span<false>(F, reinterpret_cast<const unsigned*>(cleanbuf + F.clean_off), total_bits, seg_start + F.seg_off, D.nseg, pos, bk >> 8, bk & 255, end_bit,
                       &op, &obk, &ondc, nullptr, 0, &err);
    C.end_pos[dst][ci] = op; C.end_bk[dst][ci] = obk; C.ndc[ci] = ondc;
    if (pass > 0) changed[blockIdx.y] = 1;
}

__global__ __launch_bounds__(256) void jd_blkscan_kernel(const JdFile* files, JdDyn* dyn, JdChunks C) {
    const JdFile& F = files[blockIdx.x];
    JdDyn& D = dyn[blockIdx.x];
    if (!F.valid || D.nseg < 0) return;
    const int n = (int)((D.clean_len + JD_CH - 1) / JD_CH);
    __shared__ int tot;
    if (threadIdx.x == 0) tot = 0;
    __syncthreads();
    int s = 0;
    for (int i = threadIdx.x; i < n; i += 256) { const int v = C.ndc[F.chunk_off + i]; C.first_blk[F.chunk_off + i] = v; s += v; }
    if (s) atomicAdd(&tot, s);
    __syncthreads();
    jd_block_scan(C.first_blk + F.chunk_off, n);
    if (threadIdx.x == 0) { D.total_dc = tot; if (tot != F.nblk) D.err = 1; }
}

__global__ __launch_bounds__(64) void jd_write_kernel(const JdFile* files, JdDyn* dyn, const unsigned char* cleanbuf, const unsigned* seg_start, JdChunks C,
                                                      short* coefbuf) {
    const JdFile& F = files[blockIdx.y];
    JdDyn& D = dyn[blockIdx.y];
    if (!F.valid || D.nseg < 0 || D.err) return;
    const unsigned i = blockIdx.x * 64 + threadIdx.x;
    const unsigned nchunks = (D.clean_len + JD_CH - 1) / JD_CH;
    if (i >= nchunks) return;
    const unsigned ci = F.chunk_off + i;
    const unsigned pos = C.start_pos[ci];
    const int bk = C.start_bk[ci];
    const unsigned total_bits = D.clean_len * 8u;
    unsigned end_bit = (i + 1) * (JD_CH * 8u);
    if (end_bit > total_bits) end_bit = total_bits;
    if (pos >= end_bit) return;
    unsigned op; int obk, ondc, err = 0;
    jd_span<true>(F, reinterpret_cast<const unsigned*>(cleanbuf + F.clean_off), total_bits, seg_start + F.seg_off, D.nseg, pos, bk >> 8, bk & 255, end_bit, &op, &obk,
                  &ondc, coefbuf + (size_t)F.coef_off * 64, C.first_blk[ci], &err);
    if (err) D.err = 1;
}

// ------------------------------------------------------------------------------------------------ 3. DC integration, IDCT, colour
// one workgroup per (file, component): DC differences -> absolute values, the prediction reset at every restart interval
__global__ __launch_bounds__(256) void jd_dc_kernel(const JdFile* files, const JdDyn* dyn, short* coefbuf) {
    const JdFile& F = files[blockIdx.y];
    const int c = blockIdx.x;
    if (!F.valid || dyn[blockIdx.y].nseg < 0 || dyn[blockIdx.y].err || c >= F.ncomp) return;
    short* coef = coefbuf + (size_t)F.coef_off * 64;
    const int nb = c == 0 ? F.hs * F.vs : 1, mcus = F.mcux * F.mcuy, n = mcus * nb, first = F.first_blk_of_comp[c];
    __shared__ int ssum[256], sreset[256], carry[256];
    const int t = threadIdx.x, per = (n + 255) / 256, lo = t * per, hi = min(lo + per, n);
    auto blk_of = [&](int j) { return (j / nb) * F.bpm + first + (j % nb); };
    auto resets = [&](int j) { return F.restart > 0 && j % nb == 0 && (j / nb) % F.restart == 0; };
    int s = 0, rs = 0;
    for (int j = lo; j < hi; ++j) {
        if (resets(j)) { s = 0; rs = 1; }
        s += coef[(size_t)blk_of(j) * 64];
    }
    ssum[t] = s; sreset[t] = rs;
    __syncthreads();
    if (t == 0) { int cc = 0; for (int i = 0; i < 256; ++i) { carry[i] = cc; cc = sreset[i] ? ssum[i] : cc + ssum[i]; } }
    __syncthreads();
    int run = carry[t];
    for (int j = lo; j < hi; ++j) {
        if (resets(j)) run = 0;
        run += coef[(size_t)blk_of(j) * 64];
        coef[(size_t)blk_of(j) * 64] = (short)run;
    }
}

#define JD_DESCALE(x, n) (((x) + (1 << ((n) - 1))) >> (n))
__device__ __forceinline__ unsigned char jd_limit(int x) {   // the IDCT's range_limit[x & RANGE_MASK]: clamp(x + 128) for -512 <= x < 512
    const int i = x & 1023;
    return (unsigned char)(i < 128 ? i + 128 : (i < 512 ? 255 : (i < 896 ? 0 : i - 896)));
}
// 1-D "islow" butterfly on 8 de-quantised inputs (jidctint.c); outputs before the final descale
__device__ __forceinline__ void jd_idct8(const int in[8], int out[8]) {
    int z2 = in[2], z3 = in[6];
    int z1 = (z2 + z3) * 4433;
    int tmp2 = z1 + z3 * (-15137), tmp3 = z1 + z2 * 6270;
    int tmp0 = (in[0] + in[4]) * 8192, tmp1 = (in[0] - in[4]) * 8192;
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in[7]; tmp1 = in[5]; tmp2 = in[3]; tmp3 = in[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    int z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * 9633;
    tmp0 *= 2446; tmp1 *= 16819; tmp2 *= 25172; tmp3 *= 12299;
    z1 *= -7373; z2 *= -20995; z3 *= -16069; z4 *= -3196;
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    out[0] = tmp10 + tmp3; out[7] = tmp10 - tmp3; out[1] = tmp11 + tmp2; out[6] = tmp11 - tmp2;
    out[2] = tmp12 + tmp1; out[5] = tmp12 - tmp1; out[3] = tmp13 + tmp0; out[4] = tmp13 - tmp0;
}

// The range where libjpeg-turbo's C islow IDCT and its SIMD versions (16-bit lanes, saturating packs) give the same samples: every
// de-quantised input and pass-1 output in [-16384, 16383], every output sample before the +128 in [-512, 511] (range_limit wraps
// beyond it, the SIMD code saturates).  Outside it Pillow's answer depends on the host CPU, so the file is refused (err).
__device__ __forceinline__ bool jd_out16k(int v) { return (unsigned)(v + 16384) > 32767u; }
__device__ __forceinline__ bool jd_out512(int v) { return (unsigned)(v + 512) > 1023u; }

// 8 lanes per block: lane l does column l (pass 1, into LDS), then row l (pass 2, one 8-byte store into the component plane)
__global__ __launch_bounds__(256) void jd_idct_kernel(const JdFile* files, JdDyn* dyn, const short* coefbuf, unsigned char* planebuf) {
    const JdFile& F = files[blockIdx.y];
    __shared__ int ws[32][64];
    const int lb = threadIdx.x >> 3, l = threadIdx.x & 7;
    const int B = blockIdx.x * 32 + lb;
    const bool on = F.valid && dyn[blockIdx.y].nseg >= 0 && !dyn[blockIdx.y].err && B < F.nblk;
    int comp = 0, sub = 0, m = 0;
    bool bad = false;
    if (on) {
        m = B / F.bpm;
        const int i = B - m * F.bpm;
        comp = F.comp_of_blk[i]; sub = i - F.first_blk_of_comp[comp];
        const short* c = coefbuf + ((size_t)F.coef_off + B) * 64;
        const unsigned short* q = F.q[comp];
        int in[8], o[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) { in[r] = (int)c[8 * r + l] * (int)q[8 * r + l]; bad |= jd_out16k(in[r]); }
        jd_idct8(in, o);
#pragma unroll
        for (int r = 0; r < 8; ++r) { const int v = JD_DESCALE(o[r], 11); bad |= jd_out16k(v); ws[lb][8 * r + l] = v; }
    }
    __syncthreads();
    if (on) {
        int in[8], o[8];
#pragma unroll
        for (int cc = 0; cc < 8; ++cc) in[cc] = ws[lb][8 * l + cc];
        jd_idct8(in, o);
        const int hsc = comp == 0 ? F.hs : 1, vsc = comp == 0 ? F.vs : 1;
        const int my = m / F.mcux, mx = m - my * F.mcux, by = sub / hsc, bx = sub - by * hsc;
        unsigned char* dst = planebuf + F.plane_off[comp] + (size_t)((my * vsc + by) * 8 + l) * F.pw[comp] + (mx * hsc + bx) * 8;
        unsigned lo = 0, hi = 0;
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
            const int x0 = JD_DESCALE(o[cc], 18), x1 = JD_DESCALE(o[4 + cc], 18);
            bad |= jd_out512(x0);
            bad |= jd_out512(x1);
            lo |= (unsigned)jd_limit(x0) << (8 * cc); hi |= (unsigned)jd_limit(x1) << (8 * cc);
        }
        *reinterpret_cast<uint2*>(dst) = make_uint2(lo, hi);
        if (bad) dyn[blockIdx.y].err = 1;   // (read by jd_color_kernel, jd_status_kernel and the synchronous path: that page is not written)
    }
}

// chroma sample at full-resolution position (x, y): libjpeg-turbo's fancy up-sampling (jdsample.c), or replication for very narrow planes
__device__ __forceinline__ int jd_chroma(const unsigned char* pl, int pw, int dw, int dh, int x, int y, int h2, int v2) {
    if (!h2) return pl[(size_t)y * pw + x];
    const int cx = x >> 1, cy = v2 ? y >> 1 : y;
    const unsigned char* r0 = pl + (size_t)cy * pw;
    if (dw <= 2) return r0[cx];
    if (!v2) {
        if (x == 0) return r0[0];
        if (x == 2 * dw - 1) return r0[dw - 1];
        return (x & 1) ? (3 * r0[cx] + r0[cx + 1] + 2) >> 2 : (3 * r0[cx] + r0[cx - 1] + 1) >> 2;
    }
    int far = (y & 1) ? cy + 1 : cy - 1;
    far = far < 0 ? 0 : (far > dh - 1 ? dh - 1 : far);
    const unsigned char* r1 = pl + (size_t)far * pw;
    const int cur = 3 * r0[cx] + r1[cx];
    if (x & 1) {
        if (cx == dw - 1) return (cur * 4 + 7) >> 4;
        return (cur * 3 + 3 * r0[cx + 1] + r1[cx + 1] + 7) >> 4;
    }
    if (cx == 0) return (cur * 4 + 8) >> 4;
    return (cur * 3 + 3 * r0[cx - 1] + r1[cx - 1] + 8) >> 4;
}
__device__ __forceinline__ unsigned char jd_clamp(int v) { return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

__global__ __launch_bounds__(256) void jd_color_kernel(const JdFile* files, const JdDyn* dyn, const unsigned char* planebuf, unsigned char* out, int height, int width) {
    const JdFile& F = files[blockIdx.z];
    if (!F.valid || dyn[blockIdx.z].nseg < 0 || dyn[blockIdx.z].err) return;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= width || y >= height) return;
    const int yy = planebuf[F.plane_off[0] + (size_t)y * F.pw[0] + x];
    unsigned char* o = out + (((size_t)blockIdx.z * height + y) * width + x) * 3;
    if (F.ncomp == 1) { o[0] = o[1] = o[2] = (unsigned char)yy; return; }
    const int h2 = F.hs == 2, v2 = F.vs == 2;
    const int dw = (width + F.hs - 1) / F.hs, dh = (height + F.vs - 1) / F.vs;
    const int cb = jd_chroma(planebuf + F.plane_off[1], F.pw[1], dw, dh, x, y, h2, v2) - 128;
    const int cr = jd_chroma(planebuf + F.plane_off[2], F.pw[2], dw, dh, x, y, h2, v2) - 128;
    o[0] = jd_clamp(yy + ((91881 * cr + 32768) >> 16));
    o[1] = jd_clamp(yy + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
    o[2] = jd_clamp(yy + ((116130 * cb + 32768) >> 16));
}

// per-file outcome of an asynchronous decode: host parse code, else -1 (corrupt), -5 (the fixed number of passes did not reach the fixed point), 0
__global__ void jd_status_kernel(const JdFile* files, const JdDyn* dyn, const int* host_rc, const int* changed_last, int* status, int n) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    int rc = host_rc[i];
    if (rc == 0 && files[i].valid) rc = dyn[i].nseg < 0 ? -1 : (changed_last[i] ? -5 : (dyn[i].err ? -1 : 0));   // (before the fixed point the error flag means nothing)
    status[i] = rc;
}

// ------------------------------------------------------------------------------------------------ progressive files (SOF2)
// A progressive file is a sequence of scans over one coefficient buffer.  Every scan is un-stuffed as a stream of its own by the three
// kernels above (a JdFile per scan carries its byte range and the Huffman tables in force at its SOS), then decoded in rounds:
//   round 0      every first scan (Ah = 0, DC or AC) of every file: they read no coefficient and write disjoint ones;
//   round r >= 1 the r-th refinement scan of its components: it reads what the rounds before it wrote.
// Within a round a restart segment (the whole scan where the file has none) is one serial stream: a thread for a first scan, a thread per
// block for DC refinement, a wave64 for AC refinement — the bit cost of an AC refinement symbol depends on which coefficients of the block
// are non-zero already, so no chunk can be decoded from a guessed state.
constexpr int JP_MAX_SCANS = 32;   // scans per file (Pillow's script has 10, libjpeg's cjpeg -progressive 10, mozjpeg's up to 17): more is refused with -2
struct JpScan {
    int file, round, ncs, ss, se, ah, al, restart, bps, nmcu, wc, hc;
    int comp[3], sblk[6], sci[6];   // frame component of scan component i; block-in-frame-MCU and scan component of block i of a scan MCU
};

// block index in the coefficient buffer (MCU-interleaved, padded to whole MCUs) of block i of MCU m of the scan: a single-component scan
// walks that component's own raster of ceil(w_c / 8) x ceil(h_c / 8) blocks, not the padded grid
__device__ __forceinline__ int jp_blk(const JdFile& F, const JpScan& P, int m, int i) {
    if (P.ncs > 1) return m * F.bpm + P.sblk[i];
    const int c = P.comp[0], hsc = c == 0 ? F.hs : 1, vsc = c == 0 ? F.vs : 1;
    const int by = m / P.wc, bx = m - by * P.wc;
    return ((by / vsc) * F.mcux + bx / hsc) * F.bpm + F.first_blk_of_comp[c] + (by % vsc) * hsc + bx % hsc;
}
__device__ __forceinline__ int jp_bits(JdRd& r, int nb) {   // 0 <= nb <= 16
    if (nb == 0) return 0;
    const int v = (int)jd_peek(r, nb);
    jd_skip(r, nb);
    return v;
}
// zig-zag index of the coefficient at natural position n (the inverse of JD_ZZ)
__device__ constexpr unsigned char JP_IZZ[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
                                                 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};
// correction bits of the coefficients in `range` (a mask over zig-zag positions, ascending): one stream bit each -> the mask of those set
__device__ __forceinline__ unsigned long long jp_corrections(JdRd& r, unsigned long long range) {
    unsigned long long got = 0;
    int n = __popcll(range);
    while (n > 0) {   // up to 16 stream bits at a time, first bit first
        const int c = n < 16 ? n : 16;
        unsigned v = (unsigned)jp_bits(r, c) << (32 - c);
        for (int i = 0; i < c; ++i, v <<= 1) {
            const unsigned long long low = range & (0ull - range);
            if (v & 0x80000000u) got |= low;
            range ^= low;
        }
        n -= c;
    }
    return got;
}

// AC refinement: one wave64 per restart segment (per scan where the file has none).  The bits a symbol takes depend on which coefficients
// of its block are non-zero already, so the stream itself is walked in order, by all lanes alike (wave-uniform, nothing diverges).  What the
// lanes share out is the memory work around it, 64 blocks at a time: lane j loads block j and packs its non-zero history into one 64-bit
// word over zig-zag positions; the walk reads block j's word by a cross-lane read and works on words alone — a zero run is the position of
// the (r + 1)-th clear bit from k, the history coefficients on the way are the set bits below it and take one correction bit each in that
// order — and leaves block j's outcome (corrected / new / negative, three words) with lane j; then every lane applies its block's words and
// stores it.  Corrections go away from zero, and only where the bit is not yet set.
__global__ __launch_bounds__(64) void jp_acref_kernel(const JdFile* files, JdDyn* fdyn, const JdFile* streams, const JpScan* scans, const JdDyn* sdyn,
                                                      const unsigned char* cleanbuf, const unsigned* seg_start, short* coefbuf, int round) {
    const int si = blockIdx.y;
    const JpScan& P = scans[si];
    if (P.round != round || P.ss == 0 || P.ah == 0) return;
    const JdFile& S = streams[si];
    const JdDyn& SD = sdyn[si];
    const JdFile& F = files[P.file];
    JdDyn& D = fdyn[P.file];
    const int nsegs = S.seg_cap ? (int)S.seg_cap : 1, s = blockIdx.x, lane = threadIdx.x;
    if (s >= nsegs) return;
    __shared__ JdHuff T;
    for (int i = lane; i < (int)(sizeof(JdHuff) / 4); i += 64) reinterpret_cast<unsigned*>(&T)[i] = reinterpret_cast<const unsigned*>(&S.ac[0])[i];
    __syncthreads();
    if (SD.nseg < 0 || SD.err) { D.err = 1; return; }
    const unsigned* seg = seg_start + S.seg_off;
    const unsigned total = SD.clean_len * 8u, pos0 = s ? seg[s - 1] * 8u : 0u, end = s < SD.nseg ? seg[s] * 8u : total;
    if (pos0 >= end || end > total) { D.err = 1; return; }
    const int per = P.restart > 0 ? P.restart : P.nmcu, m0 = s * per, m1 = min(m0 + per, P.nmcu);
    uint4* coef4 = reinterpret_cast<uint4*>(coefbuf + (size_t)F.coef_off * 64);   // a block: 8 x 16 bytes
    JdRd r; r.w = reinterpret_cast<const unsigned*>(cleanbuf + S.clean_off); r.have = 0; r.pos = pos0; r.acc = 0;
    const int ss = P.ss, se = P.se, p1 = 1 << P.al;
    const unsigned long long band = (se >= 63 ? ~0ull : (1ull << (se + 1)) - 1ull) & (~0ull << ss);
    bool bad = m0 >= m1;
    int eobrun = 0;
    for (int mb = m0; mb < m1 && !bad; mb += 64) {
        // ---- lane j: the history word of block mb + j ----
        const int cnt = min(64, m1 - mb);
        int B = -1;
        unsigned long long nz = 0;
        if (lane < cnt) {
            B = jp_blk(F, P, mb + lane, 0);
            if (B < 0 || B >= F.nblk) B = -1;
        }
        if (B >= 0) {
            uint4 v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = coef4[(size_t)B * 8 + q];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const unsigned w[4] = {v[q].x, v[q].y, v[q].z, v[q].w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (w[e] & 0xFFFFu) nz |= 1ull << JP_IZZ[q * 8 + e * 2];
                    if (w[e] >> 16) nz |= 1ull << JP_IZZ[q * 8 + e * 2 + 1];
                }
            }
            nz &= band;
        }
        if (__any(lane < cnt && B < 0)) { bad = true; break; }
        // ---- the walk: wave-uniform ----
        // Every lane runs it with the same values: the reader's state comes from loads at addresses that do not depend on the lane, h is
        // lane j's word read by all lanes, and `bad`, eobrun, k and the three outcome words follow from those alone.  So no branch below
        // diverges, all 64 lanes are active at each __shfl, and `lane == j` is the only place where a lane keeps something of its own.
        unsigned long long my_corr = 0, my_new = 0, my_neg = 0;
        for (int j = 0; j < cnt && !bad; ++j) {
            const unsigned long long h = ((unsigned long long)(unsigned)__shfl((int)(nz >> 32), j) << 32) | (unsigned)__shfl((int)(nz & 0xFFFFFFFFull), j);
            unsigned long long corr = 0, nw = 0, neg = 0;
            int k = ss;
            if (eobrun == 0) {
                while (k <= se) {
                    const int rs = jd_sym(r, T);
                    if (rs < 0) { bad = true; break; }
                    int run = rs >> 4, val = 0;
                    const int sz = rs & 15;
                    if (sz) {
                        if (sz != 1) { bad = true; break; }   // a new coefficient is +-1 at this depth
                        val = jp_bits(r, 1) ? 1 : -1;
                    } else if (run != 15) {
                        eobrun = (1 << run) + jp_bits(r, run);
                        break;   // the rest of the band takes its correction bits below
                    }
                    // the (run + 1)-th zero coefficient from k (past the band if there are fewer)
                    unsigned long long z = ~h & band & (~0ull << k);
                    for (int i = 0; i < run; ++i) z &= z - 1ull;
                    const int kend = z ? __ffsll((long long)z) - 1 : se + 1;
                    corr |= jp_corrections(r, h & (~0ull << k) & (kend > 63 ? ~0ull : (1ull << kend) - 1ull));
                    k = kend;
                    if (r.pos > end) { bad = true; break; }
                    if (val) {
                        if (k > se) { bad = true; break; }
                        nw |= 1ull << k;
                        if (val < 0) neg |= 1ull << k;
                    }
                    ++k;
                }
            }
            if (!bad && eobrun > 0) {
                if (k <= se) corr |= jp_corrections(r, h & (~0ull << k));
                --eobrun;
            }
            if (r.pos > end) bad = true;
            if (lane == j) { my_corr = corr; my_new = nw; my_neg = neg; }
        }
        // ---- lane j: apply and store (a page that went bad is not written out, so its blocks may stay half done) ----
        if (B >= 0 && (my_corr | my_new)) {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                uint4 v = coef4[(size_t)B * 8 + q];
                unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int zz = JP_IZZ[q * 8 + e];
                    int c = (short)(e & 1 ? w[e >> 1] >> 16 : w[e >> 1] & 0xFFFFu);
                    if (((my_corr >> zz) & 1ull) && (c & p1) == 0) c = c >= 0 ? c + p1 : c - p1;
                    if ((my_new >> zz) & 1ull) c = ((my_neg >> zz) & 1ull) ? -p1 : p1;
                    w[e >> 1] = e & 1 ? (w[e >> 1] & 0xFFFFu) | ((unsigned)(unsigned short)c << 16) : (w[e >> 1] & 0xFFFF0000u) | (unsigned short)c;
                }
                coef4[(size_t)B * 8 + q] = make_uint4(w[0], w[1], w[2], w[3]);
            }
        }
    }
    // the segment's data ends with its blocks: fewer than 8 bits are left, all ones, and no end-of-band run is open
    if (!bad) {
        const unsigned rem = end - r.pos;
        if (eobrun != 0 || rem >= 8u || (rem > 0u && jd_peek(r, (int)rem) != (1u << rem) - 1u)) bad = true;
    }
    if (bad && lane == 0) D.err = 1;
}

__global__ __launch_bounds__(64) void jp_entropy_kernel(const JdFile* files, JdDyn* fdyn, const JdFile* streams, const JpScan* scans, const JdDyn* sdyn,
                                                        const unsigned char* cleanbuf, const unsigned* seg_start, short* coefbuf, int round) {
    const int si = blockIdx.y;
    const JpScan& P = scans[si];
    if (P.round != round || P.ah != 0) return;   // (refinement: jp_dcref_kernel, jp_acref_kernel)
    const JdFile& S = streams[si];
    const JdDyn& SD = sdyn[si];
    const JdFile& F = files[P.file];
    JdDyn& D = fdyn[P.file];
    // the scan's tables in LDS: every symbol is a dependent look-up (T[0 .. 2]: the DC tables of the scan's components, T[3]: its AC table)
    __shared__ JdHuff T[4];
    for (int i = threadIdx.x; i < (int)(sizeof(JdHuff) / 4) * 4; i += 64) {
        const int t = i / (int)(sizeof(JdHuff) / 4), o = i - t * (int)(sizeof(JdHuff) / 4);
        reinterpret_cast<unsigned*>(&T[t])[o] = reinterpret_cast<const unsigned*>(t < 3 ? &S.dc[t] : &S.ac[0])[o];
    }
    __syncthreads();
    const int nsegs = S.seg_cap ? (int)S.seg_cap : 1, s = blockIdx.x * 64 + threadIdx.x;
    if (s >= nsegs) return;
    if (SD.nseg < 0 || SD.err) { D.err = 1; return; }
    const unsigned* seg = seg_start + S.seg_off;
    const unsigned total = SD.clean_len * 8u, pos0 = s ? seg[s - 1] * 8u : 0u, end = s < SD.nseg ? seg[s] * 8u : total;
    if (pos0 >= end || end > total) { D.err = 1; return; }
    const int per = P.restart > 0 ? P.restart : P.nmcu, m0 = s * per, m1 = min(m0 + per, P.nmcu);
    short* coef = coefbuf + (size_t)F.coef_off * 64;
    JdRd r; r.w = reinterpret_cast<const unsigned*>(cleanbuf + S.clean_off); r.have = 0; r.pos = pos0; r.acc = 0;
    bool bad = m0 >= m1;
    int eobrun = 0;
    if (P.ss == 0) {   // DC first: the baseline state machine without AC; the prediction restarts with the segment
        int pred[3] = {0, 0, 0};
        for (int m = m0; m < m1 && !bad; ++m)
            for (int i = 0; i < P.bps && !bad; ++i) {
                const int ci = P.sci[i];
                const int sym = jd_sym(r, T[ci]);
                if (sym < 0 || sym > 11) { bad = true; break; }
                pred[ci] += sym ? jd_extend(jp_bits(r, sym), sym) : 0;
                const int B = jp_blk(F, P, m, i);
                if (r.pos > end || (unsigned)(pred[ci] + 32768) > 65535u || (unsigned)(pred[ci] * (1 << P.al) + 32768) > 65535u || B >= F.nblk) { bad = true; break; }
                coef[(size_t)B * 64] = (short)(pred[ci] * (1 << P.al));
            }
    } else {   // AC first
        for (int m = m0; m < m1 && !bad; ++m) {
            if (eobrun > 0) { --eobrun; continue; }
            const int B = jp_blk(F, P, m, 0);
            if (B >= F.nblk) { bad = true; break; }
            short* c = coef + (size_t)B * 64;
            for (int k = P.ss; k <= P.se; ++k) {
                const int rs = jd_sym(r, T[3]);
                if (rs < 0) { bad = true; break; }
                const int run = rs >> 4, sz = rs & 15;
                if (sz) {
                    k += run;
                    const int v = jd_extend(jp_bits(r, sz), sz) * (1 << P.al);
                    if (k > P.se || r.pos > end || (unsigned)(v + 32768) > 65535u) { bad = true; break; }
                    c[JD_ZZ[k]] = (short)v;
                } else if (run == 15) {
                    k += 15;
                    if (k > P.se || r.pos > end) { bad = true; break; }   // (libjpeg lets a zero run end past the band; no encoder writes one)
                } else {   // EOBn: this block and 2^n + extra - 1 more end here
                    eobrun = (1 << run) + jp_bits(r, run) - 1;
                    if (r.pos > end) bad = true;
                    break;
                }
            }
        }
    }
    // the segment's data ends with its blocks: fewer than 8 bits are left, all ones, and no end-of-band run is open
    if (!bad) {
        const unsigned rem = end - r.pos;
        if (eobrun != 0 || rem >= 8u || (rem > 0u && jd_peek(r, (int)rem) != (1u << rem) - 1u)) bad = true;
    }
    if (bad) D.err = 1;
}

// DC refinement: one raw bit per block, bit i of a segment belongs to its block i
__global__ __launch_bounds__(256) void jp_dcref_kernel(const JdFile* files, JdDyn* fdyn, const JdFile* streams, const JpScan* scans, const JdDyn* sdyn,
                                                       const unsigned char* cleanbuf, const unsigned* seg_start, short* coefbuf, int round) {
    const int si = blockIdx.y;
    const JpScan& P = scans[si];
    if (P.round != round || P.ss != 0 || P.ah == 0) return;
    const JdFile& S = streams[si];
    const JdDyn& SD = sdyn[si];
    const JdFile& F = files[P.file];
    JdDyn& D = fdyn[P.file];
    const int nb = P.nmcu * P.bps, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= nb) return;
    if (SD.nseg < 0 || SD.err) { D.err = 1; return; }
    const int per = (P.restart > 0 ? P.restart : P.nmcu) * P.bps, s = j / per, bit = j - s * per;
    const unsigned* seg = seg_start + S.seg_off;
    const unsigned total = SD.clean_len * 8u, pos0 = s ? seg[s - 1] * 8u : 0u, end = s < SD.nseg ? seg[s] * 8u : total;
    const unsigned char* clean = cleanbuf + S.clean_off;
    const unsigned pos = pos0 + (unsigned)bit;
    if (end > total || pos >= end) { D.err = 1; return; }
    const int m = j / P.bps, B = jp_blk(F, P, m, j - m * P.bps);
    if (B >= F.nblk) { D.err = 1; return; }
    if ((clean[pos >> 3] >> (7 - (pos & 7))) & 1) coefbuf[((size_t)F.coef_off + B) * 64] |= (short)(1 << P.al);
    if (bit == min(per, nb - s * per) - 1) {   // the segment's last block: only padding may follow
        const unsigned rem = end - pos - 1u;
        if (rem >= 8u || (rem > 0u && (clean[(pos + 1) >> 3] & ((1u << rem) - 1u)) != (1u << rem) - 1u)) D.err = 1;
    }
}

// ------------------------------------------------------------------------------------------------ host: headers
struct HostHeader {
    int width = 0, height = 0, ncomp = 0, hs[3] = {1, 1, 1}, vs[3] = {1, 1, 1}, tq[3] = {0, 0, 0}, td[3] = {0, 0, 0}, ta[3] = {0, 0, 0}, restart = 0;
    unsigned short q[4][64];
    unsigned char bits[2][4][17], vals[2][4][256];
    bool have_q[4] = {false, false, false, false}, have_h[2][4] = {{false, false, false, false}, {false, false, false, false}};
    size_t scan_off = 0, scan_end = 0;
};

// libjpeg's table check (jdhuff.c jpeg_make_d_derived_tbl): at every length the codes must fit WITHOUT the all-ones code, i.e. the
// code space is never full, let alone oversubscribed; a DC table holds categories 0 .. 15 only
bool huff_counts_ok(const unsigned char bits[17], const unsigned char* vals, bool dc) {
    int code = 0, cnt = 0;
    for (int l = 1; l <= 16; ++l) {
        code += bits[l]; cnt += bits[l];
        if (code >= (1 << l)) return false;
        code <<= 1;
    }
    if (dc)
        for (int i = 0; i < cnt; ++i)
            if (vals[i] > 15) return false;
    return true;
}

// The same rules as the oracle's parse_header (oracle/csrc/jpegdec_oracle.c): a file one of them accepts, the other accepts too.
int parse_header(const uint8_t* f, size_t n, HostHeader* h) {
    if (n < 4 || f[0] != 0xFF || f[1] != 0xD8) return -1;
    size_t p = 2;
    bool sof = false;
    int adobe = -1;   // the APP14 transform flag, -1 = no Adobe marker
    for (;;) {
        if (p + 4 > n || f[p] != 0xFF) return -1;
        while (p < n && f[p] == 0xFF) ++p;
        if (p >= n) return -1;
        const int m = f[p++];
        if (m == 0xD8 || (m >= 0xD0 && m <= 0xD7) || m == 0x01) continue;
        if (m == 0xD9 || p + 2 > n) return -1;
        const size_t len = ((size_t)f[p] << 8) | f[p + 1];
        if (len < 2 || p + len > n) return -1;
        const uint8_t* s = f + p + 2;
        const size_t sl = len - 2;
        if (m == 0xDB) {
            size_t i = 0;
            while (i < sl) {
                const int pq = s[i] >> 4, t = s[i] & 15;
                ++i;
                if (t > 3 || pq > 1 || i + (pq ? 128 : 64) > sl) return -1;
                for (int k = 0; k < 64; ++k) { h->q[t][H_ZZ[k]] = pq ? (unsigned short)((s[i] << 8) | s[i + 1]) : s[i]; i += pq ? 2 : 1; }
                h->have_q[t] = true;
            }
        } else if (m == 0xC4) {
            size_t i = 0;
            while (i < sl) {
                const int tc = s[i] >> 4, t = s[i] & 15;
                ++i;
                if (tc > 1 || t > 3 || i + 16 > sl) return -1;
                int cnt = 0;
                h->bits[tc][t][0] = 0;
                for (int k = 1; k <= 16; ++k) { h->bits[tc][t][k] = s[i + k - 1]; cnt += s[i + k - 1]; }
                i += 16;
                if (cnt > 256 || i + cnt > sl) return -1;
                memset(h->vals[tc][t], 0, 256);
                memcpy(h->vals[tc][t], s + i, (size_t)cnt);
                if (!huff_counts_ok(h->bits[tc][t], h->vals[tc][t], tc == 0)) return -1;
                i += cnt;
                h->have_h[tc][t] = true;
            }
        } else if (m == 0xC0 || m == 0xC1) {
            if (sl < 6 || sof) return -1;
            if (s[0] != 8) return -2;
            h->height = (s[1] << 8) | s[2]; h->width = (s[3] << 8) | s[4]; h->ncomp = s[5];
            if (h->height == 0 || h->width == 0 || (h->ncomp != 1 && h->ncomp != 3)) return -2;
            if (sl != (size_t)(6 + 3 * h->ncomp)) return -1;   // libjpeg: JERR_BAD_LENGTH
            for (int c = 0; c < h->ncomp; ++c) {
                if (s[6 + 3 * c] != c + 1) return -2;
                h->hs[c] = s[7 + 3 * c] >> 4; h->vs[c] = s[7 + 3 * c] & 15; h->tq[c] = s[8 + 3 * c];
                if (h->tq[c] > 3) return -1;
            }
            sof = true;
        } else if (m >= 0xC2 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {
            return -2;
        } else if (m == 0xDD) {
            if (sl != 2) return -1;
            h->restart = (s[0] << 8) | s[1];
        } else if (m == 0xEE) {   // Adobe: the transform flag is judged after SOF (APP14 usually precedes it)
            if (sl >= 12 && memcmp(s, "Adobe", 5) == 0) adobe = s[11];
        } else if (m == 0xDA) {
            if (!sof) return -1;
            if (sl < 1 || s[0] != h->ncomp || sl < (size_t)(1 + 2 * h->ncomp + 3)) return -2;
            for (int c = 0; c < h->ncomp; ++c) {
                if (s[1 + 2 * c] != c + 1) return -2;
                h->td[c] = s[2 + 2 * c] >> 4; h->ta[c] = s[2 + 2 * c] & 15;
                if (h->td[c] > 3 || h->ta[c] > 3 || !h->have_h[0][h->td[c]] || !h->have_h[1][h->ta[c]] || !h->have_q[h->tq[c]]) return -1;
            }
            h->scan_off = p + len;
            break;
        }
        p += len;
    }
    if (h->ncomp == 1) { h->hs[0] = h->vs[0] = 1; }
    else {
        if (h->hs[1] != 1 || h->vs[1] != 1 || h->hs[2] != 1 || h->vs[2] != 1) return -2;
        if (!((h->hs[0] == 1 && h->vs[0] == 1) || (h->hs[0] == 2 && h->vs[0] == 1) || (h->hs[0] == 2 && h->vs[0] == 2))) return -2;
    }
    if (h->ncomp == 3 && adobe >= 0 && adobe != 1) return -2;   // a colour transform other than YCbCr changes the colour model
    // the entropy-coded segment ends at the last EOI (trailing bytes after it are ignored, as libjpeg does)
    size_t e = n;
    while (e >= h->scan_off + 2 && !(f[e - 2] == 0xFF && f[e - 1] == 0xD9)) --e;
    if (e < h->scan_off + 2) return -1;
    h->scan_end = e - 2;
    if (h->scan_end - h->scan_off >= ((size_t)1 << 29)) return -2;   // bit positions on the device are 32-bit
    // inside the scan 0xFF starts a stuffed zero or an RSTn marker; fill bytes (FF FF) or a last byte 0xFF are corrupt, any other
    // marker (DNL, a second SOS ...) is outside the subset
    for (const uint8_t* q = f + h->scan_off; q < f + h->scan_end;) {   // (memchr: the scan is megabytes, 0xFF bytes are rare)
        q = static_cast<const uint8_t*>(memchr(q, 0xFF, (size_t)(f + h->scan_end - q)));
        if (q == nullptr) break;
        if (q + 1 >= f + h->scan_end || q[1] == 0xFF) return -1;
        if (q[1] != 0x00 && (q[1] & 0xF8) != 0xD0) return -2;
        q += 2;
    }
    return 0;
}

bool build_huff(const unsigned char bits[17], const unsigned char* vals, JdHuff* t) {
    int code = 0, k = 0;
    memset(t, 0, sizeof(*t));
    if (!huff_counts_ok(bits, vals, false)) return false;   // (checked before fast[] is filled: an oversubscribed table would write past it)
    memcpy(t->vals, vals, 256);
    for (int l = 1; l <= 16; ++l) {
        t->valptr[l] = k - code;
        if (bits[l]) {
            if (l <= 8)
                for (int i = 0; i < bits[l]; ++i) {
                    const int c = code + i;
                    for (int f = 0; f < (1 << (8 - l)); ++f) t->fast[(c << (8 - l)) | f] = (unsigned short)((l << 8) | vals[k + i]);
                }
            k += bits[l]; code += bits[l];
            t->maxcode[l] = code - 1;
        } else t->maxcode[l] = -1;
        code <<= 1;
    }
    return true;
}

// ---- progressive files: every scan's parameters, the tables in force at its SOS and its entropy-coded bytes ----
struct ProgScan { int ncs, comp[3], ss, se, ah, al, restart; size_t off, end; JdHuff dc[3], ac; };
struct ProgHeader { HostHeader h; std::vector<ProgScan> scans; };

// 0 = a progressive file of the subset; 1 = a sequential file (SOF0 / SOF1: parse_header judges it); -1 / -2 as parse_header.
// The progression rules are libjpeg's (jdmaster / jdphuff start_pass): what it raises or warns on is corrupt here.  A file is taken only
// if its scans bring all 64 coefficients of every component down to Al = 0: short of that libjpeg smooths across blocks.
int parse_progressive(const uint8_t* f, size_t n, ProgHeader* ph) {
    HostHeader& h = ph->h;
    if (n < 4 || f[0] != 0xFF || f[1] != 0xD8) return -1;
    size_t p = 2;
    bool sof = false;
    int adobe = -1;
    int cbits[3][64];
    for (auto& c : cbits) for (int& v : c) v = -1;
    for (;;) {
        if (p + 2 > n || f[p] != 0xFF) return -1;
        while (p < n && f[p] == 0xFF) ++p;
        if (p >= n) return -1;
        const int m = f[p++];
        if (m == 0xD9) break;
        if (m == 0xD8 || (m >= 0xD0 && m <= 0xD7) || m == 0x01) continue;
        if (p + 2 > n) return -1;
        const size_t len = ((size_t)f[p] << 8) | f[p + 1];
        if (len < 2 || p + len > n) return -1;
        const uint8_t* s = f + p + 2;
        const size_t sl = len - 2;
        if (m == 0xDB) {
            if (!ph->scans.empty()) return -2;   // libjpeg latches a component's table at its first scan: a later DQT is not followed here
            size_t i = 0;
            while (i < sl) {
                const int pq = s[i] >> 4, t = s[i] & 15;
                ++i;
                if (t > 3 || pq > 1 || i + (pq ? 128 : 64) > sl) return -1;
                for (int k = 0; k < 64; ++k) { h.q[t][H_ZZ[k]] = pq ? (unsigned short)((s[i] << 8) | s[i + 1]) : s[i]; i += pq ? 2 : 1; }
                h.have_q[t] = true;
            }
        } else if (m == 0xC4) {
            size_t i = 0;
            while (i < sl) {
                const int tc = s[i] >> 4, t = s[i] & 15;
                ++i;
                if (tc > 1 || t > 3 || i + 16 > sl) return -1;
                int cnt = 0;
                h.bits[tc][t][0] = 0;
                for (int k = 1; k <= 16; ++k) { h.bits[tc][t][k] = s[i + k - 1]; cnt += s[i + k - 1]; }
                i += 16;
                if (cnt > 256 || i + cnt > sl) return -1;
                memset(h.vals[tc][t], 0, 256);
                memcpy(h.vals[tc][t], s + i, (size_t)cnt);
                if (!huff_counts_ok(h.bits[tc][t], h.vals[tc][t], tc == 0)) return -1;
                i += cnt;
                h.have_h[tc][t] = true;
            }
        } else if (m == 0xC0 || m == 0xC1) {
            return sof ? -1 : 1;
        } else if (m == 0xC2) {
            if (sl < 6 || sof) return -1;
            if (s[0] != 8) return -2;
            h.height = (s[1] << 8) | s[2]; h.width = (s[3] << 8) | s[4]; h.ncomp = s[5];
            if (h.height == 0 || h.width == 0 || (h.ncomp != 1 && h.ncomp != 3)) return -2;
            if (sl != (size_t)(6 + 3 * h.ncomp)) return -1;
            for (int c = 0; c < h.ncomp; ++c) {
                if (s[6 + 3 * c] != c + 1) return -2;
                h.hs[c] = s[7 + 3 * c] >> 4; h.vs[c] = s[7 + 3 * c] & 15; h.tq[c] = s[8 + 3 * c];
                if (h.tq[c] > 3) return -1;
            }
            if (h.ncomp == 1) { h.hs[0] = h.vs[0] = 1; }
            else {
                if (h.hs[1] != 1 || h.vs[1] != 1 || h.hs[2] != 1 || h.vs[2] != 1) return -2;
                if (!((h.hs[0] == 1 && h.vs[0] == 1) || (h.hs[0] == 2 && h.vs[0] == 1) || (h.hs[0] == 2 && h.vs[0] == 2))) return -2;
            }
            sof = true;
        } else if (m >= 0xC3 && m <= 0xCF && m != 0xC8) {   // lossless, differential, arithmetic (DAC = 0xCC included)
            return -2;
        } else if (m == 0xDD) {
            if (sl != 2) return -1;
            h.restart = (s[0] << 8) | s[1];
        } else if (m == 0xEE) {
            if (sl >= 12 && memcmp(s, "Adobe", 5) == 0) adobe = s[11];
        } else if (m == 0xDC) {   // DNL
            return -2;
        } else if (m == 0xDA) {
            if (!sof || sl < 1) return -1;
            ProgScan sc;
            sc.ncs = s[0];
            if (sc.ncs < 1 || sc.ncs > h.ncomp || sl != (size_t)(1 + 2 * sc.ncs + 3)) return -1;
            if (ph->scans.size() >= (size_t)JP_MAX_SCANS) return -2;
            if (ph->scans.empty())
                for (int c = 0; c < h.ncomp; ++c)
                    if (!h.have_q[h.tq[c]]) return -2;   // (a table that arrives after the first scan: left to libjpeg)
            sc.ss = s[1 + 2 * sc.ncs]; sc.se = s[2 + 2 * sc.ncs]; sc.ah = s[3 + 2 * sc.ncs] >> 4; sc.al = s[3 + 2 * sc.ncs] & 15;
            sc.restart = h.restart;
            if (sc.ss > sc.se || sc.se > 63 || sc.ah > 13 || sc.al > 13) return -1;
            if (sc.ss == 0 ? sc.se != 0 : sc.ncs != 1) return -1;   // a DC scan holds DC only, an AC scan one component
            if (sc.ah != 0 && sc.al != sc.ah - 1) return -1;
            memset(sc.dc, 0, sizeof(sc.dc)); memset(&sc.ac, 0, sizeof(sc.ac));
            for (int i = 0; i < sc.ncs; ++i) {
                const int c = s[1 + 2 * i] - 1, td = s[2 + 2 * i] >> 4, ta = s[2 + 2 * i] & 15;
                if (c < 0 || c >= h.ncomp || td > 3 || ta > 3) return -1;
                if (i > 0 && c <= sc.comp[i - 1]) return c == sc.comp[i - 1] ? -1 : -2;
                sc.comp[i] = c;
                if (sc.ss != 0 && cbits[c][0] < 0) return -1;   // AC before this component's DC
                for (int k = sc.ss; k <= sc.se; ++k) {
                    // a coefficient that is complete (Al = 0) sent again as a first scan: libjpeg takes it in silence and the later scan wins;
                    // here all first scans run at once and must write disjoint coefficients, so such a file is left to libjpeg
                    if (sc.ah == 0 && cbits[c][k] == 0) return -2;
                    if (sc.ah != (cbits[c][k] < 0 ? 0 : cbits[c][k])) return -1;   // not the successor of this coefficient's last scan
                    cbits[c][k] = sc.al;
                }
                if (sc.ss == 0 && sc.ah == 0 && (!h.have_h[0][td] || !build_huff(h.bits[0][td], h.vals[0][td], &sc.dc[i]))) return -1;
                if (sc.ss != 0 && (!h.have_h[1][ta] || !build_huff(h.bits[1][ta], h.vals[1][ta], &sc.ac))) return -1;
            }
            // the entropy-coded bytes run to the next marker that is neither a stuffed zero nor RSTn
            size_t q = p + len;
            sc.off = q;
            for (;;) {
                const uint8_t* x = q < n ? static_cast<const uint8_t*>(memchr(f + q, 0xFF, n - q)) : nullptr;
                if (x == nullptr) return -1;   // no EOI
                q = (size_t)(x - f);
                if (q + 1 >= n || f[q + 1] == 0xFF) return -1;
                if (f[q + 1] != 0x00 && (f[q + 1] & 0xF8) != 0xD0) break;
                q += 2;
            }
            sc.end = q;
            if (sc.end - sc.off >= ((size_t)1 << 29)) return -2;
            ph->scans.push_back(sc);
            p = q;
            continue;
        }
        p += len;
    }
    if (!sof || ph->scans.empty()) return -1;
    if (h.ncomp == 3 && adobe >= 0 && adobe != 1) return -2;
    for (int c = 0; c < h.ncomp; ++c)
        for (int k = 0; k < 64; ++k)
            if (cbits[c][k] != 0) return -2;   // a coefficient never sent, or short of full precision
    return 0;
}

// the workspace's regions for a batch with these totals: one layout sizes it and carves it (jpegdec_run)
struct JdWorkspace {
    JdFile* F; JdDyn* D; uint8_t *raw, *clean;   // scan bytes as uploaded / un-stuffed (+ 64: the bit reader's look-ahead)
    int *keep, *rst; unsigned* seg; JdChunks C; short* coef; uint8_t* plane; int *changed, *host_rc, *status;
    JdFile* S; JpScan* P; JdDyn* SD;   // progressive batches: one stream per scan (at most JP_MAX_SCANS per file)
};
JdWorkspace jd_layout(Arena& a, int n, size_t raw_total, size_t ublk_total, size_t seg_total, size_t chunk_total, size_t blk_total, size_t plane_total,
                      size_t nstreams = 0) {
    JdWorkspace w;
    w.S = a.take<JdFile>(nstreams); w.P = a.take<JpScan>(nstreams); w.SD = a.take<JdDyn>(nstreams);
    w.F = a.take<JdFile>(n); w.D = a.take<JdDyn>(n);
    w.raw = a.take<uint8_t>(raw_total); w.clean = a.take<uint8_t>(raw_total + 64);
    w.keep = a.take<int>(ublk_total + 8); w.rst = a.take<int>(ublk_total + 8);
    w.seg = a.take<unsigned>(seg_total);
    w.C.start_pos = a.take<unsigned>(chunk_total + 8); w.C.start_bk = a.take<int>(chunk_total + 8);
    w.C.end_pos[0] = a.take<unsigned>(chunk_total + 8); w.C.end_pos[1] = a.take<unsigned>(chunk_total + 8);
    w.C.end_bk[0] = a.take<int>(chunk_total + 8); w.C.end_bk[1] = a.take<int>(chunk_total + 8);
    w.C.ndc = a.take<int>(chunk_total + 8); w.C.first_blk = a.take<int>(chunk_total + 8);
    w.coef = a.take<short>(blk_total * 64); w.plane = a.take<uint8_t>(plane_total);
    w.changed = a.take<int>((size_t)n * (JD_PASSES + 1)); w.host_rc = a.take<int>(n); w.status = a.take<int>(n);
    return w;
}

}  // namespace

int jpegdec_probe(const uint8_t* file, size_t n, JdInfo* info) {
    HostHeader h;
    const int rc = parse_header(file, n, &h);
    if (info) { info->width = h.width; info->height = h.height; info->ncomp = h.ncomp; info->hs = h.hs[0]; info->vs = h.vs[0]; info->restart = h.restart; }
    return rc;
}

int jpegdec_run(lumina_ocr* eng, const uint8_t* const* files, const size_t* sizes, int n, int height, int width, uint8_t* out_dev, int* status, hipStream_t st,
                int async_passes) {
    // async_passes > 0: that many synchronisation passes are enqueued without looking at their result, nothing is synchronised, and
    // `status` (PINNED host memory of the caller) is filled by a copy at the end of the stream's work: -5 = the passes did not suffice
    std::vector<JdFile> F((size_t)n);
    std::vector<const uint8_t*> scan_src((size_t)n, nullptr);
    // the scan bytes of all files go through ONE pinned staging buffer (kept by the engine) and ONE asynchronous copy
    size_t raw_cap = 0;
    for (int i = 0; i < n; ++i) raw_cap += ((sizes[i] + 16 + 255) & ~(size_t)255);
    // two staging buffers in turn: an asynchronous call's upload may still be queued when the next call fills its buffer
    lumina_ocr::Staging& stage = eng->jd_stage[eng->jd_stage_next]; eng->jd_stage_next ^= 1;
    if (stage.uploaded) LOCR_CHECK(hipEventSynchronize(stage.uploaded.get()));
    else {
        hipEvent_t ev = nullptr;
        LOCR_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        stage.uploaded.reset(ev);
    }
    LOCR_CHECK(stage.buf.reserve(raw_cap, stage.uploaded.get()));
    uint8_t* raw = stage.buf.get();
    size_t raw_total = 0, ublk_total = 0, chunk_total = 0, seg_total = 0, blk_total = 0, plane_total = 0;
    unsigned max_ublk = 0, max_chunks = 0;
    int max_blk = 0, any = 0;
    for (int i = 0; i < n; ++i) {
        JdFile& f = F[(size_t)i];
        memset(&f, 0, sizeof(f));
        HostHeader h;
        int rc = parse_header(files[i], sizes[i], &h);
        if (rc == 0 && (h.width != width || h.height != height)) rc = -4;
        status[i] = rc;
        if (rc) continue;
        f.valid = 1; ++any;
        f.width = h.width; f.height = h.height; f.ncomp = h.ncomp; f.hs = h.hs[0]; f.vs = h.vs[0]; f.restart = h.restart;
        f.mcux = (h.width + 8 * f.hs - 1) / (8 * f.hs); f.mcuy = (h.height + 8 * f.vs - 1) / (8 * f.vs);
        f.bpm = f.hs * f.vs + (h.ncomp == 3 ? 2 : 0);
        f.nblk = f.mcux * f.mcuy * f.bpm;
        int b = 0;
        for (int c = 0; c < h.ncomp; ++c) {
            f.first_blk_of_comp[c] = b;
            for (int k = 0; k < (c == 0 ? f.hs * f.vs : 1); ++k) f.comp_of_blk[b++] = c;
            f.pw[c] = f.mcux * (c == 0 ? f.hs : 1) * 8; f.ph[c] = f.mcuy * (c == 0 ? f.vs : 1) * 8;
            f.plane_off[c] = (unsigned)plane_total; plane_total += ((size_t)f.pw[c] * f.ph[c] + 255) & ~(size_t)255;
            memcpy(f.q[c], h.q[h.tq[c]], sizeof(f.q[c]));
            f.td[c] = c; f.ta[c] = c;   // every component gets its own copy of its tables: no index indirection on the device
            if (!build_huff(h.bits[0][h.td[c]], h.vals[0][h.td[c]], &f.dc[c]) || !build_huff(h.bits[1][h.ta[c]], h.vals[1][h.ta[c]], &f.ac[c])) { status[i] = -1; f.valid = 0; }
        }
        if (!f.valid) { --any; continue; }
        f.raw_len = (unsigned)(h.scan_end - h.scan_off);
        f.raw_off = (unsigned)raw_total; f.clean_off = f.raw_off;
        const size_t padded = ((size_t)f.raw_len + 16 + 255) & ~(size_t)255;   // (the bit reader loads three aligned words past its position)
        scan_src[(size_t)i] = files[i] + h.scan_off;
        raw_total += padded;
        f.nublk = (f.raw_len + JD_UB - 1) / JD_UB; f.ublk_off = (unsigned)ublk_total; ublk_total += f.nublk;
        f.nchunk_cap = (f.raw_len + JD_CH - 1) / JD_CH + 1; f.chunk_off = (unsigned)chunk_total; chunk_total += f.nchunk_cap;
        f.seg_cap = h.restart ? (unsigned)((f.mcux * f.mcuy + h.restart - 1) / h.restart) : 0; f.seg_off = (unsigned)seg_total; seg_total += f.seg_cap + 1;
        f.coef_off = (unsigned)blk_total; blk_total += (size_t)f.nblk;
        if (f.nublk > max_ublk) max_ublk = f.nublk;
        if (f.nchunk_cap > max_chunks) max_chunks = f.nchunk_cap;
        if (f.nblk > max_blk) max_blk = f.nblk;
        if (raw_total >= (1ull << 31) || blk_total >= (1ull << 31)) return locr_fail(eng, "jpeg_decode", "batch too large (2 GiB of scan data / 2^31 blocks)");
    }
    if (!any) { if (async_passes > 0) { /* status is already final */ } return 0; }
    // ---- workspace ----
    Arena sizing;
    jd_layout(sizing, n, raw_total, ublk_total, seg_total, chunk_total, blk_total, plane_total);
    if (eng_ws_reserve(eng, sizing.off)) return 1;
    Arena a(eng->ws.get(), eng->ws.cap);
    const JdWorkspace w = jd_layout(a, n, raw_total, ublk_total, seg_total, chunk_total, blk_total, plane_total);
    if (a.overflow) return locr_fail(eng, "jpeg_decode", "workspace layout exceeds the reservation");
    LOCR_CHECK(hipMemcpyAsync(w.F, F.data(), sizeof(JdFile) * n, hipMemcpyHostToDevice, st));
    // scan bytes: host copy into the pinned buffer and the asynchronous upload of the previous files overlap (groups of ~8 MB)
    {
        size_t sent = 0;
        for (int i = 0; i < n; ++i) {
            const JdFile& f = F[(size_t)i];
            if (!f.valid) continue;
            const size_t padded = ((size_t)f.raw_len + 16 + 255) & ~(size_t)255;
            memcpy(raw + f.raw_off, scan_src[(size_t)i], f.raw_len);
            memset(raw + f.raw_off + f.raw_len, 0, padded - f.raw_len);
            const size_t end = (size_t)f.raw_off + padded;
            if (end - sent >= (8u << 20) || end == raw_total) {
                LOCR_CHECK(hipMemcpyAsync(w.raw + sent, raw + sent, end - sent, hipMemcpyHostToDevice, st));
                sent = end;
            }
        }
        if (sent < raw_total) LOCR_CHECK(hipMemcpyAsync(w.raw + sent, raw + sent, raw_total - sent, hipMemcpyHostToDevice, st));
    }
    LOCR_CHECK(hipEventRecord(stage.uploaded.get(), st));   // the staging buffer is free again once the uploads have run
    LOCR_CHECK(hipMemsetAsync(w.clean, 0, raw_total + 64, st));
    LOCR_CHECK(hipMemsetAsync(w.coef, 0, blk_total * 128, st));
    // ---- 1. un-stuff ----
    hipLaunchKernelGGL(jd_mark_kernel, dim3(max_ublk, n), dim3(256), 0, st, w.F, w.raw, w.keep, w.rst);
    hipLaunchKernelGGL(jd_scan_kernel, dim3(n), dim3(256), 0, st, w.F, w.keep, w.rst, w.D);
    hipLaunchKernelGGL(jd_compact_kernel, dim3(max_ublk, n), dim3(256), 0, st, w.F, w.raw, w.keep, w.rst, w.D, w.clean, w.seg);
    // ---- 2. synchronise the chunk decoders (Jacobi passes until nothing changes) ----
    std::vector<int> changed((size_t)n * (JD_PASSES + 1));
    const dim3 cgrid((max_chunks + 63) / 64, n);
    int pass = 0;
    if (async_passes > 0) {
        // host parse codes travel with the call (the descriptor upload above was from pageable memory: already consumed)
        LOCR_CHECK(hipMemcpyAsync(w.host_rc, status, sizeof(int) * n, hipMemcpyHostToDevice, st));
        LOCR_CHECK(hipMemsetAsync(w.changed, 0, sizeof(int) * (size_t)n * (JD_PASSES + 1), st));
        for (; pass < async_passes; ++pass) {
            if (pass == async_passes - 1) LOCR_CHECK(hipMemsetAsync(w.changed, 0, sizeof(int) * n, st));
            hipLaunchKernelGGL(jd_sync_kernel, cgrid, dim3(64), 0, st, w.F, w.D, w.clean, w.seg, w.C, pass, w.changed);
        }
        eng->jd_last_passes = pass;
        hipLaunchKernelGGL(jd_blkscan_kernel, dim3(n), dim3(256), 0, st, w.F, w.D, w.C);
        hipLaunchKernelGGL(jd_write_kernel, cgrid, dim3(64), 0, st, w.F, w.D, w.clean, w.seg, w.C, w.coef);
        hipLaunchKernelGGL(jd_dc_kernel, dim3(3, n), dim3(256), 0, st, w.F, w.D, w.coef);
        hipLaunchKernelGGL(jd_idct_kernel, dim3((max_blk + 31) / 32, n), dim3(256), 0, st, w.F, w.D, w.coef, w.plane);
        hipLaunchKernelGGL(jd_color_kernel, dim3((width + 63) / 64, (height + 3) / 4, n), dim3(256), 0, st, w.F, w.D, w.plane, out_dev, height, width);
        hipLaunchKernelGGL(jd_status_kernel, dim3((n + 63) / 64), dim3(64), 0, st, w.F, w.D, w.host_rc, w.changed, w.status, n);
        LOCR_CHECK(hipMemcpyAsync(status, w.status, sizeof(int) * n, hipMemcpyDeviceToHost, st));
        LOCR_CHECK(hipGetLastError());
        return 0;
    }
    for (;;) {
        LOCR_CHECK(hipMemsetAsync(w.changed, 0, sizeof(int) * changed.size(), st));
        for (int k = 0; k < JD_PASSES; ++k, ++pass) hipLaunchKernelGGL(jd_sync_kernel, cgrid, dim3(64), 0, st, w.F, w.D, w.clean, w.seg, w.C, pass, w.changed + (size_t)k * n);
        LOCR_CHECK(hipMemcpyAsync(changed.data(), w.changed, sizeof(int) * changed.size(), hipMemcpyDeviceToHost, st));
        LOCR_CHECK(hipStreamSynchronize(st));
        bool again = false;
        for (int i = 0; i < n; ++i) again = again || changed[(size_t)(JD_PASSES - 1) * n + i] != 0;
        if (!again) break;
        if ((unsigned)pass > max_chunks + JD_PASSES) return locr_fail(eng, "jpeg_decode", "the chunk decoders did not reach a fixed point");
    }
    eng->jd_last_passes = pass;
    // ---- 3. coefficients, DC, IDCT, colour ----
    hipLaunchKernelGGL(jd_blkscan_kernel, dim3(n), dim3(256), 0, st, w.F, w.D, w.C);
    hipLaunchKernelGGL(jd_write_kernel, cgrid, dim3(64), 0, st, w.F, w.D, w.clean, w.seg, w.C, w.coef);
    hipLaunchKernelGGL(jd_dc_kernel, dim3(3, n), dim3(256), 0, st, w.F, w.D, w.coef);
    hipLaunchKernelGGL(jd_idct_kernel, dim3((max_blk + 31) / 32, n), dim3(256), 0, st, w.F, w.D, w.coef, w.plane);
    hipLaunchKernelGGL(jd_color_kernel, dim3((width + 63) / 64, (height + 3) / 4, n), dim3(256), 0, st, w.F, w.D, w.plane, out_dev, height, width);
    std::vector<JdDyn> dyn((size_t)n);
    LOCR_CHECK(hipMemcpyAsync(dyn.data(), w.D, sizeof(JdDyn) * n, hipMemcpyDeviceToHost, st));
    LOCR_CHECK(hipStreamSynchronize(st));
    LOCR_CHECK(hipGetLastError());
    for (int i = 0; i < n; ++i)
        if (F[(size_t)i].valid && (dyn[(size_t)i].err || dyn[(size_t)i].nseg < 0)) status[i] = -1;
    return 0;
}

int jpegdec_probe_progressive(const uint8_t* file, size_t n, JdProgInfo* info) {
    ProgHeader ph;
    int rc = parse_progressive(file, n, &ph);
    if (rc == 1) {
        HostHeader h;
        rc = parse_header(file, n, &h);
        if (info) *info = JdProgInfo{h.width, h.height, h.ncomp, h.hs[0], h.vs[0], h.restart, 0, rc == 0 ? 1 : 0};
        return rc;
    }
    const HostHeader& h = ph.h;
    if (info) *info = JdProgInfo{h.width, h.height, h.ncomp, h.hs[0], h.vs[0], ph.scans.empty() ? h.restart : ph.scans[0].restart, 1, (int)ph.scans.size()};
    return rc;
}

int jpegdec_run_progressive(lumina_ocr* eng, const uint8_t* const* files, const size_t* sizes, int n, int height, int width, uint8_t* out_dev, int* status,
                            hipStream_t st) {
    std::vector<ProgHeader> PH((size_t)n);
    std::vector<int> prc((size_t)n);
    bool any_seq = false;
    for (int i = 0; i < n; ++i) { prc[(size_t)i] = parse_progressive(files[i], sizes[i], &PH[(size_t)i]); any_seq = any_seq || prc[(size_t)i] == 1; }
    // sequential files take the existing kernels (the others are hidden from that call: an empty file is refused before it is read)
    if (any_seq) {
        static const uint8_t none = 0;
        std::vector<const uint8_t*> bf((size_t)n);
        std::vector<size_t> bs((size_t)n);
        for (int i = 0; i < n; ++i) { const bool q = prc[(size_t)i] == 1; bf[(size_t)i] = q ? files[i] : &none; bs[(size_t)i] = q ? sizes[i] : 0; }
        const int rc = jpegdec_run(eng, bf.data(), bs.data(), n, height, width, out_dev, status, st);
        if (rc) return rc;
    }
    std::vector<JdFile> F((size_t)n), S;
    std::vector<JpScan> P;
    std::vector<JdDyn> D((size_t)n);
    std::vector<const uint8_t*> src;
    size_t raw_total = 0, ublk_total = 0, seg_total = 0, blk_total = 0, plane_total = 0;
    unsigned max_ublk = 1;
    int max_blk = 0, max_seg = 1, max_dcref = 0, rounds = 0, any = 0;
    for (int i = 0; i < n; ++i) {
        JdFile& f = F[(size_t)i];
        memset(&f, 0, sizeof(f));
        D[(size_t)i] = JdDyn{0u, 0, 0, 0};
        if (prc[(size_t)i] == 1) continue;
        const HostHeader& h = PH[(size_t)i].h;
        int rc = prc[(size_t)i];
        if (rc == 0 && (h.width != width || h.height != height)) rc = -4;
        status[i] = rc;
        if (rc) continue;
        f.valid = 1; ++any;
        f.width = h.width; f.height = h.height; f.ncomp = h.ncomp; f.hs = h.hs[0]; f.vs = h.vs[0];
        f.mcux = (h.width + 8 * f.hs - 1) / (8 * f.hs); f.mcuy = (h.height + 8 * f.vs - 1) / (8 * f.vs);
        f.bpm = f.hs * f.vs + (h.ncomp == 3 ? 2 : 0);
        f.nblk = f.mcux * f.mcuy * f.bpm;
        int b = 0;
        for (int c = 0; c < h.ncomp; ++c) {
            f.first_blk_of_comp[c] = b;
            for (int k = 0; k < (c == 0 ? f.hs * f.vs : 1); ++k) f.comp_of_blk[b++] = c;
            f.pw[c] = f.mcux * (c == 0 ? f.hs : 1) * 8; f.ph[c] = f.mcuy * (c == 0 ? f.vs : 1) * 8;
            f.plane_off[c] = (unsigned)plane_total; plane_total += ((size_t)f.pw[c] * f.ph[c] + 255) & ~(size_t)255;
            memcpy(f.q[c], h.q[h.tq[c]], sizeof(f.q[c]));
        }
        f.coef_off = (unsigned)blk_total; blk_total += (size_t)f.nblk;
        if (f.nblk > max_blk) max_blk = f.nblk;
        int nref[3] = {0, 0, 0};
        for (const ProgScan& sc : PH[(size_t)i].scans) {
            JdFile s;
            memset(&s, 0, sizeof(s));
            JpScan q;
            memset(&q, 0, sizeof(q));
            q.file = i; q.ncs = sc.ncs; q.ss = sc.ss; q.se = sc.se; q.ah = sc.ah; q.al = sc.al;
            for (int k = 0; k < sc.ncs; ++k) {
                const int c = sc.comp[k];
                q.comp[k] = c;
                s.dc[k] = sc.dc[k];
                if (sc.ncs > 1)
                    for (int j = 0; j < (c == 0 ? f.hs * f.vs : 1); ++j) { q.sblk[q.bps] = f.first_blk_of_comp[c] + j; q.sci[q.bps] = k; ++q.bps; }
            }
            s.ac[0] = sc.ac;
            if (sc.ncs > 1) { q.nmcu = f.mcux * f.mcuy; q.wc = f.mcux; q.hc = f.mcuy; }
            else {   // the component's own raster
                const int c = sc.comp[0], wc = c == 0 ? h.width : (h.width + f.hs - 1) / f.hs, hc = c == 0 ? h.height : (h.height + f.vs - 1) / f.vs;
                q.bps = 1; q.wc = (wc + 7) / 8; q.hc = (hc + 7) / 8; q.nmcu = q.wc * q.hc;
            }
            q.restart = sc.restart;
            if (sc.ah != 0) {
                int r = 0;
                for (int k = 0; k < sc.ncs; ++k) r = nref[sc.comp[k]] > r ? nref[sc.comp[k]] : r;
                q.round = r + 1;
                for (int k = 0; k < sc.ncs; ++k) nref[sc.comp[k]] = q.round;
                if (q.round > rounds) rounds = q.round;
                if (sc.ss == 0 && q.nmcu * q.bps > max_dcref) max_dcref = q.nmcu * q.bps;
            }
            s.valid = 1;
            s.raw_len = (unsigned)(sc.end - sc.off);
            s.raw_off = (unsigned)raw_total; s.clean_off = s.raw_off;
            raw_total += ((size_t)s.raw_len + 16 + 255) & ~(size_t)255;
            s.nublk = (s.raw_len + JD_UB - 1) / JD_UB; s.ublk_off = (unsigned)ublk_total; ublk_total += s.nublk;
            s.seg_cap = sc.restart ? (unsigned)((q.nmcu + sc.restart - 1) / sc.restart) : 0; s.seg_off = (unsigned)seg_total; seg_total += s.seg_cap + 1;
            if (s.nublk > max_ublk) max_ublk = s.nublk;
            if ((int)s.seg_cap > max_seg) max_seg = (int)s.seg_cap;
            S.push_back(s); P.push_back(q); src.push_back(files[i] + sc.off);
            if (raw_total >= (1ull << 31) || blk_total >= (1ull << 31)) return locr_fail(eng, "jpeg_decode_progressive", "batch too large (2 GiB of scan data / 2^31 blocks)");
        }
    }
    if (!any) return 0;
    const int ns = (int)S.size();
    if (ns > 65535) return locr_fail(eng, "jpeg_decode_progressive", "batch too large (more than 65535 scans: the streams are a grid's second dimension)");
    lumina_ocr::Staging& stage = eng->jd_stage[eng->jd_stage_next]; eng->jd_stage_next ^= 1;
    if (stage.uploaded) LOCR_CHECK(hipEventSynchronize(stage.uploaded.get()));
    else {
        hipEvent_t ev = nullptr;
        LOCR_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        stage.uploaded.reset(ev);
    }
    LOCR_CHECK(stage.buf.reserve(raw_total, stage.uploaded.get()));
    uint8_t* raw = stage.buf.get();
    Arena sizing;
    jd_layout(sizing, n, raw_total, ublk_total, seg_total, 0, blk_total, plane_total, (size_t)ns);
    if (eng_ws_reserve(eng, sizing.off)) return 1;
    Arena a(eng->ws.get(), eng->ws.cap);
    const JdWorkspace w = jd_layout(a, n, raw_total, ublk_total, seg_total, 0, blk_total, plane_total, (size_t)ns);
    if (a.overflow) return locr_fail(eng, "jpeg_decode_progressive", "workspace layout exceeds the reservation");
    for (int k = 0; k < ns; ++k) {
        const JdFile& s = S[(size_t)k];
        const size_t padded = ((size_t)s.raw_len + 16 + 255) & ~(size_t)255;
        memcpy(raw + s.raw_off, src[(size_t)k], s.raw_len);
        memset(raw + s.raw_off + s.raw_len, 0, padded - s.raw_len);
    }
    LOCR_CHECK(hipMemcpyAsync(w.raw, raw, raw_total, hipMemcpyHostToDevice, st));
    LOCR_CHECK(hipEventRecord(stage.uploaded.get(), st));
    LOCR_CHECK(hipMemcpyAsync(w.F, F.data(), sizeof(JdFile) * n, hipMemcpyHostToDevice, st));
    LOCR_CHECK(hipMemcpyAsync(w.D, D.data(), sizeof(JdDyn) * n, hipMemcpyHostToDevice, st));
    LOCR_CHECK(hipMemcpyAsync(w.S, S.data(), sizeof(JdFile) * ns, hipMemcpyHostToDevice, st));
    LOCR_CHECK(hipMemcpyAsync(w.P, P.data(), sizeof(JpScan) * ns, hipMemcpyHostToDevice, st));
    LOCR_CHECK(hipMemsetAsync(w.clean, 0, raw_total + 64, st));
    LOCR_CHECK(hipMemsetAsync(w.seg, 0, sizeof(unsigned) * seg_total, st));
    LOCR_CHECK(hipMemsetAsync(w.coef, 0, blk_total * 128, st));
    // ---- un-stuff: once over all scans of all files ----
    hipLaunchKernelGGL(jd_mark_kernel, dim3(max_ublk, ns), dim3(256), 0, st, w.S, w.raw, w.keep, w.rst);
    hipLaunchKernelGGL(jd_scan_kernel, dim3(ns), dim3(256), 0, st, w.S, w.keep, w.rst, w.SD);
    hipLaunchKernelGGL(jd_compact_kernel, dim3(max_ublk, ns), dim3(256), 0, st, w.S, w.raw, w.keep, w.rst, w.SD, w.clean, w.seg);
    // ---- entropy decode: first scans, then the refinement rounds ----
    hipLaunchKernelGGL(jp_entropy_kernel, dim3((max_seg + 63) / 64, ns), dim3(64), 0, st, w.F, w.D, w.S, w.P, w.SD, w.clean, w.seg, w.coef, 0);
    for (int r = 1; r <= rounds; ++r) {
        hipLaunchKernelGGL(jp_acref_kernel, dim3(max_seg, ns), dim3(64), 0, st, w.F, w.D, w.S, w.P, w.SD, w.clean, w.seg, w.coef, r);
        if (max_dcref > 0)
            hipLaunchKernelGGL(jp_dcref_kernel, dim3((max_dcref + 255) / 256, ns), dim3(256), 0, st, w.F, w.D, w.S, w.P, w.SD, w.clean, w.seg, w.coef, r);
    }
    // ---- pixels: unchanged ----
    hipLaunchKernelGGL(jd_idct_kernel, dim3((max_blk + 31) / 32, n), dim3(256), 0, st, w.F, w.D, w.coef, w.plane);
    hipLaunchKernelGGL(jd_color_kernel, dim3((width + 63) / 64, (height + 3) / 4, n), dim3(256), 0, st, w.F, w.D, w.plane, out_dev, height, width);
    LOCR_CHECK(hipMemcpyAsync(D.data(), w.D, sizeof(JdDyn) * n, hipMemcpyDeviceToHost, st));
    LOCR_CHECK(hipStreamSynchronize(st));
    LOCR_CHECK(hipGetLastError());
    for (int i = 0; i < n; ++i)
        if (F[(size_t)i].valid && D[(size_t)i].err) status[i] = -1;
    return 0;
}
