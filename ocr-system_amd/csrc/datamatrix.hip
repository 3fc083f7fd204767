// Data Matrix (ECC 200; 10 x 10 .. 52 x 52 and the six rectangles; 64 x 64 .. 144 x 144 behind lumina_ocr_datamatrix_sizes) on the GPU (gfx950): the symbols of a page as (x0, y0, x1, y1, rows,
// cols, ndata, errors, rotation, timing mismatches, L misses, 0) with their corrected data codewords, in a canonical order.
// Everything is integer and every reduction is order-free (min / max / add / xor, ballots), so the lists equal the sequential
// definition restated in tests/dm_reference.py.
//
// All stream-ordered kernels, no host round trip:
//   1-3 components_launch (runs.h)      the mask (or the one the caller already has), its run list, the 8-connected components; a run is
//                 its own area and its own four diagonal extremes (run_extremes); every run learns its root, and box, area and
//                 extremes are accumulated there
//   4 dm_candidates  one wave per row, lanes over the row's roots: the box and area filter -> counted, gathered per page
//   5 dm_decode   one wave per (page, candidate): every (size, rotation) try that is in reach (wave-uniform) is scored with lanes
//                 over the modules of its solid and clock rows and columns; for the kept try lane r samples module row r on the
//                 affine grid as one 64-bit word; the quiet rings; lanes gather the codewords through the placement table from the
//                 rows in LDS; per block the decoder of rs.h.  Every loop has a constant bound, every table, LDS and page index
//                 is clamped, and no wave waits for another (a work-group is one wave)
//   5b dm_large   (lumina_ocr_datamatrix_sizes alone, max_size >= 64) a second candidate list (dm_candidates with the sides 64 min_module ..
//                 144 max_module), one wave per (page, candidate): see "stage 2" below; definition: tests/dm_sizes_reference.py
//   6 dm_output   one work-group per page (code_output.h): valid candidates counted, gathered, rank-sorted by (y0, x0, y1, x1, root)
#include "datamatrix.h"
#include "code_output.h"
#include "dm_tables.h"
#include "dm_tables_large.h"
#include "rs.h"
#include "runs.h"
#include <mutex>
#include <vector>

namespace {

typedef unsigned long long u64;
typedef long long i64;

// a candidate's result (code_output.h): y0, x0, y1, x1, root, rows, cols, ndata, errors, rotation, timing, misses, 0, state
constexpr int DM_MAX_TOTAL = 288, DM_MAX_BLOCK = 242, DM_MAX_EC = 68, DM_MAX_NB = 2;
constexpr int DM_RAW = 320, DM_BLK = 256;   // LDS arrays: the codewords of a symbol, of a block (multiples of 64)

// 4: cands [B][max_candidates] = the roots that pass the box (sides lo_side min_module .. hi_side max_module) and area filter
__global__ __launch_bounds__(256) void dm_candidates_kernel(const int* runoff, const int* parent, const int4* box, const int* area, int H, size_t runcap,
                                                            int min_module, int max_module, int lo_side, int hi_side, int max_candidates, int* ncand, int* cands,
                                                            int rows_total) {
    int pg, row, lane;
    if (!row_wave(H, rows_total, pg, row, lane)) return;
    const int* ro = runoff + (size_t)pg * (H + 1);
    const size_t rb = (size_t)pg * runcap;
    for (int id = ro[row] + lane; id < ro[row + 1]; id += 64) {
        if (parent[rb + id] != id) continue;
        const int4 bx = box[rb + id];   // x0, x1, y0, y1
        const int w = bx.y - bx.x + 1, h = bx.w - bx.z + 1;
        if (w < lo_side * min_module || h < lo_side * min_module || w > hi_side * max_module || h > hi_side * max_module) continue;
        if (32 * (i64)area[rb + id] < (i64)w * h) continue;
        const int idx = atomicAdd(&ncand[pg], 1);
        if (idx < max_candidates) cands[(size_t)pg * max_candidates + idx] = id;
    }
}

// the affine grid of a try: O the L's elbow, U up its upright (R rows), V along its foot (C columns), doubled pixel coordinates
struct DmGrid { int ox2, oy2, vxr, vyr, uxc, uyc, R, C; unsigned den; };

// module (row r, col c): the ink at the pixel of its centre; off the page reads clear.  Every term stays below 2^30: the arms of a
// try in reach are at most 2 * 52 * 64 doubled pixels and the page's sides at most 65535.
__device__ __forceinline__ int dm_sample(const u64* mpage, int H, int W, int nw, const DmGrid& g, int r, int c) {
    const int nx = g.ox2 + g.vxr * (2 * c + 1) + g.uxc * (2 * g.R - 2 * r - 1), ny = g.oy2 + g.vyr * (2 * c + 1) + g.uyc * (2 * g.R - 2 * r - 1);
    if (nx < 0 || ny < 0) return 0;
    const int px = (int)((unsigned)nx / g.den), py = (int)((unsigned)ny / g.den);
    if (px >= W || py >= H) return 0;
    return (int)((mpage[(size_t)py * nw + (px >> 6)] >> (px & 63)) & 1ull);
}

struct DmLds {
    u64 rows[64];
    unsigned char raw[DM_RAW];
    RsLds<unsigned char, DM_BLK, DM_MAX_EC, 8> rs;
};

// 5: one wave per (page, candidate): res [B][res_slots][CODE_RES_INTS] (res_slots >= max_candidates), resdata [B][max_candidates][DM_MAX_DATA]
__global__ __launch_bounds__(64) void dm_decode_kernel(const u64* mask, const int* cands, const int* ncand, const u64* ext, int H, int W, int nw, size_t runcap,
                                                       int max_candidates, int min_module, int max_module, int quiet, int timing_max, int solid_max, int res_slots,
                                                       int* res, unsigned char* resdata) {
    __shared__ DmLds s;
    const int pg = blockIdx.y, a = blockIdx.x, lane = threadIdx.x;
    const int nc_page = ncand[pg];
    if (nc_page > max_candidates || a >= nc_page || a >= DM_MAX_CANDIDATES) return;
    const u64* mpage = mask + (size_t)pg * H * nw;
    const int root = clampi(cands[(size_t)pg * max_candidates + a], 0, (int)runcap - 1);
    rs_load_tables(s.rs, DM_EXP, DM_LOG, 8, lane);
    // the outer corners of the four extremes, doubled
    int cx[4], cy[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const u64 e = ext[((size_t)pg * runcap + root) * 4 + j];
        const int x = (int)(e & 0xffffull), yf = (int)((e >> 16) & 0xffffull), y = (j == 0 || j == 3) ? yf : 65535 - yf;
        cx[j] = 2 * (x + ((j == 1 || j == 2) ? 1 : 0));
        cy[j] = 2 * (y + (j >= 2 ? 1 : 0));
    }
    // every (size, rotation) in reach: the smallest (timing mismatches, L misses, R C, k, size)
    i64 best = -1;
    const i64 lo_m = (i64)min_module, hi_m = (i64)max_module;
#pragma unroll 1
    for (int sz = 0; sz < DM_NUM_SIZES; ++sz) {
        const int R = DM_SIZES[sz * 8 + 0], C = DM_SIZES[sz * 8 + 1], nr = clampi(DM_SIZES[sz * 8 + 4], 1, 2), nc = clampi(DM_SIZES[sz * 8 + 5], 1, 2);
        const int RH = R / nr, RW = C / nc;
#pragma unroll 1
        for (int k = 0; k < 4; ++k) {
            const int ox = cx[(k + 3) & 3], oy = cy[(k + 3) & 3];
            const int ux = cx[k] - ox, uy = cy[k] - oy, vx = cx[(k + 2) & 3] - ox, vy = cy[(k + 2) & 3] - oy;
            const i64 lu = (i64)ux * ux + (i64)uy * uy, lv = (i64)vx * vx + (i64)vy * vy;
            const i64 ulo = 2 * R * lo_m, uhi = 2 * R * hi_m, vlo = 2 * C * lo_m, vhi = 2 * C * hi_m;
            if (lu < ulo * ulo || lu > uhi * uhi || lv < vlo * vlo || lv > vhi * vhi) continue;
            const i64 qa = lu * C * C, qb = lv * R * R;
            if (16 * (qa > qb ? qa : qb) > 25 * (qa < qb ? qa : qb)) continue;
            DmGrid g;
            g.R = R; g.C = C; g.den = 4u * R * C;
            g.ox2 = ox * 2 * R * C; g.oy2 = oy * 2 * R * C; g.vxr = vx * R; g.vyr = vy * R; g.uxc = ux * C; g.uyc = uy * C;
            int misses = 0, timing = 0;
            for (int i = 0; i < 4; ++i) {   // the regions' clock rows (even i) and solid rows (odd i)
                if (i >= 2 * nr) break;
                const int r = (i >> 1) * RH + ((i & 1) ? RH - 1 : 0);
                const bool on = lane < C;
                const int v = on ? dm_sample(mpage, H, W, nw, g, r, lane) : 0;
                const int lc = lane >= RW ? lane - RW : lane;
                const bool solid = (i & 1) || lc == 0;
                misses += __popcll(__ballot(on && solid && !v));
                timing += __popcll(__ballot(on && !solid && v != ((lane & 1) ^ 1)));
            }
            for (int j = 0; j < 4; ++j) {   // the regions' solid columns (even j) and clock columns (odd j), without the rows above
                if (j >= 2 * nc) break;
                const int c = (j >> 1) * RW + ((j & 1) ? RW - 1 : 0);
                const int lr = lane >= RH ? lane - RH : lane;
                const bool on = lane < R && lr != 0 && lr != RH - 1;
                const int v = on ? dm_sample(mpage, H, W, nw, g, lane, c) : 0;
                misses += __popcll(__ballot(on && !(j & 1) && !v));
                timing += __popcll(__ballot(on && (j & 1) && v != (lane & 1)));
            }
            const i64 key = ((i64)timing << 32) | ((i64)misses << 20) | ((i64)(R * C) << 8) | (i64)(k << 5) | (i64)sz;
            if (best < 0 || key < best) best = key;
        }
    }
    if (best < 0) return;
    const int timing = (int)(best >> 32), misses = (int)((best >> 20) & 0xfff), k = (int)((best >> 5) & 3), sz = clampi((int)(best & 31), 0, DM_NUM_SIZES - 1);
    if (timing > timing_max || misses > solid_max) return;
    const int R = DM_SIZES[sz * 8 + 0], C = DM_SIZES[sz * 8 + 1], ndata = DM_SIZES[sz * 8 + 2], ncheck = DM_SIZES[sz * 8 + 3];
    const int nb = clampi(DM_SIZES[sz * 8 + 6], 1, DM_MAX_NB), total = ndata + ncheck, ec = ncheck / nb;
    if (total > DM_MAX_TOTAL || ndata > DM_MAX_DATA || ec < 2 || ec > DM_MAX_EC || (ndata + nb - 1) / nb + ec > DM_MAX_BLOCK) return;   // (the tables never say so)
    const int ox = cx[(k + 3) & 3], oy = cy[(k + 3) & 3];
    const int ux = cx[k] - ox, uy = cy[k] - oy, vx = cx[(k + 2) & 3] - ox, vy = cy[(k + 2) & 3] - oy;
    DmGrid g;
    g.R = R; g.C = C; g.den = 4u * R * C;
    g.ox2 = ox * 2 * R * C; g.oy2 = oy * 2 * R * C; g.vxr = vx * R; g.vyr = vy * R; g.uxc = ux * C; g.uyc = uy * C;
    // the quiet rings
    bool dirty = false;
    for (int q = 1; q <= DM_MAX_QUIET; ++q) {
        if (q > quiet) break;
        const int t = lane - q;
        if (t < C + q) dirty = dirty || dm_sample(mpage, H, W, nw, g, -q, t) || dm_sample(mpage, H, W, nw, g, R - 1 + q, t);
        if (t < R + q) dirty = dirty || dm_sample(mpage, H, W, nw, g, t, -q) || dm_sample(mpage, H, W, nw, g, t, C - 1 + q);
    }
    if (__ballot(dirty)) return;
    // lane r samples module row r
    u64 row = 0;
    if (lane < R)
        for (int c = 0; c < 52; ++c)
            if (c < C) row |= (u64)dm_sample(mpage, H, W, nw, g, lane, c) << c;
    s.rows[lane] = row;
    __syncthreads();
    // codewords in placement order
    const int poff = DM_PLACE_OFF[sz];
#pragma unroll 1
    for (int i = lane; i < DM_RAW; i += 64) {
        int val = 0;
        if (i < total) {
            for (int bit = 0; bit < 8; ++bit) {
                const int at = poff + 8 * i + bit;
                const unsigned p = DM_PLACE[at < DM_PLACE_N ? at : DM_PLACE_N - 1];
                val = (val << 1) | (int)((s.rows[(p >> 6) & 63] >> (p & 63)) & 1ull);
            }
        }
        s.raw[i] = (unsigned char)val;
    }
    __syncthreads();
    unsigned char* od = resdata + ((size_t)pg * max_candidates + a) * DM_MAX_DATA;
    int errors = 0;
    for (int blk = 0; blk < DM_MAX_NB; ++blk) {
        if (blk >= nb) break;
        const int nd = (ndata - blk + nb - 1) / nb, len = nd + ec;   // block blk takes every nb-th codeword from blk on
#pragma unroll
        for (int p0 = 0; p0 < DM_BLK; p0 += 64) {
            const int p = p0 + lane;
            if (p < len) s.rs.blk[p] = s.raw[clampi(p < nd ? p * nb + blk : ndata + (p - nd) * nb + blk, 0, DM_RAW - 1)];
        }
        __syncthreads();
        const int got = rs_correct_block(s.rs, len, ec, 1, lane);
        if (got < 0) return;
        errors += got;
#pragma unroll
        for (int p0 = 0; p0 < DM_BLK; p0 += 64) {
            const int p = p0 + lane;
            if (p < nd && p * nb + blk < DM_MAX_DATA) od[p * nb + blk] = s.rs.blk[p];
        }
        __syncthreads();
    }
    if (lane == 0) {
        // the hull: the parallelogram O, O + U, O + V, O + U + V (every coordinate is even)
        int x0 = 0, x1 = 0, y0 = 0, y1 = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int qx = (ox + ((c & 1) ? ux : 0) + ((c & 2) ? vx : 0)) >> 1, qy = (oy + ((c & 1) ? uy : 0) + ((c & 2) ? vy : 0)) >> 1;
            x0 = c == 0 || qx < x0 ? qx : x0; x1 = c == 0 || qx > x1 ? qx : x1;
            y0 = c == 0 || qy < y0 ? qy : y0; y1 = c == 0 || qy > y1 ? qy : y1;
        }
        int* o = res + ((size_t)pg * res_slots + a) * CODE_RES_INTS;
        o[0] = clampi(y0, 0, H - 1); o[1] = clampi(x0, 0, W - 1); o[2] = clampi(y1 - 1, 0, H - 1); o[3] = clampi(x1 - 1, 0, W - 1); o[4] = root;
        o[5] = R; o[6] = C; o[7] = ndata; o[8] = errors; o[9] = k; o[10] = timing; o[11] = misses; o[12] = 0; o[CODE_RES_STATE] = CODE_ROW;
    }
}

// ---- stage 2 of lumina_ocr_datamatrix_sizes: the squares of 64 x 64 .. 144 x 144 (definition: tests/dm_sizes_reference.py) ----
// A module row is three 64-bit words; a symbol has up to 2178 codewords in up to ten blocks of at most 175 + 68 (120 x 120).
constexpr int DML_MAX_SIDE = 144, DML_WORDS = 3, DML_MAX_TOTAL = 2178, DML_RAW = 2240, DML_MAX_NB = 10, DML_MAX_REGIONS = 6, DML_MAX_BLOCK = 243;
static_assert(DML_RAW % 64 == 0 && DML_RAW >= DML_MAX_TOTAL && DM_MAX_DATA_ALL >= 1558, "lanes walk whole chunks of the codewords");
static_assert(DML_MAX_BLOCK <= DM_BLK && DML_MAX_BLOCK <= 255, "a block fits the decoder's array and the field's order");

// The affine grid of dm_sample with the elbow taken out: the doubled elbow (2 X, 2 Y) is even, so the numerator of dm_sample is
// X * den + d with d = vxr (2 c + 1) + uxc (2 R - 2 r - 1), den = 4 R C, and its pixel is X + floor(d / den): negative exactly when the
// numerator is.  The numerator itself passes 2^32 here (a doubled coordinate of up to 131070 times 2 * 144 * 144); d does not pass
// 2^31: an arm in reach has at most 2 * 144 * 64 = 18432 doubled pixels, times the other side (<= 144), times |2 c + 1| or
// |2 R - 2 r - 1| <= 295 (the quiet rings reach four modules out) is at most 7.83e8, and d is two such terms.
struct DmlGrid { int X, Y, vxr, vyr, uxc, uyc, R, den; };

__device__ __forceinline__ int dml_floor_div(int d, int den) {
    const int q = d / den;
    return q - (d - q * den < 0 ? 1 : 0);
}

__device__ __forceinline__ int dml_sample(const u64* mpage, int H, int W, int nw, const DmlGrid& g, int r, int c) {
    const int px = g.X + dml_floor_div(g.vxr * (2 * c + 1) + g.uxc * (2 * g.R - 2 * r - 1), g.den);
    const int py = g.Y + dml_floor_div(g.vyr * (2 * c + 1) + g.uyc * (2 * g.R - 2 * r - 1), g.den);
    if (px < 0 || py < 0 || px >= W || py >= H) return 0;
    return (int)((mpage[(size_t)py * nw + (px >> 6)] >> (px & 63)) & 1ull);
}

struct DmLargeLds {
    u64 rows[DML_MAX_SIDE * DML_WORDS];
    unsigned char raw[DML_RAW];
    RsLds<unsigned char, DM_BLK, DM_MAX_EC, 8> rs;
};

// 5b: one wave per (page, stage-2 candidate).  res [B][2 max_candidates][CODE_RES_INTS]: stage 1's records in a page's first
// max_candidates slots, this stage's behind them; o[14] of a record here is its data row in rowdata [B][max_codes][DM_MAX_DATA_ALL],
// handed out by nrows (a symbol past max_codes has a record and no row: the page's list overflows and is not written).  The score is
// stage 1's rule over all 2 nr rows and 2 nc columns of the regions, lanes over the modules in up to three passes of 64; the grid is
// sampled with lanes over columns and a ballot per word, so that neighbouring lanes read neighbouring pixels and a row of 144 keeps
// 144 of 192 lane slots busy whatever the number of rows; blocks are dealt by stream position (position p belongs to block p mod nb).
__global__ __launch_bounds__(64) void dm_large_kernel(const u64* mask, const int* cands, const int* ncand, const int* ncand1, const u64* ext, int H, int W, int nw,
                                                      size_t runcap, int max_candidates, int max_codes, int min_module, int max_module, int quiet, int timing_max,
                                                      int solid_max, int max_size, int* res, int* nrows, unsigned char* rowdata) {
    __shared__ DmLargeLds s;
    const int pg = blockIdx.y, a = blockIdx.x, lane = threadIdx.x;
    const int nc_page = ncand[pg];
    if (nc_page > max_candidates || a >= nc_page || a >= DM_MAX_CANDIDATES) return;
    const u64* mpage = mask + (size_t)pg * H * nw;
    const int root = clampi(cands[(size_t)pg * max_candidates + a], 0, (int)runcap - 1);
    int* pres = res + (size_t)pg * 2 * max_candidates * CODE_RES_INTS;
    // a root that gave a stage-1 row is skipped
    const int n1 = ncand1[pg];
    bool taken = false;
    if (n1 <= max_candidates)
        for (int a0 = 0; a0 < DM_MAX_CANDIDATES; a0 += 64) {
            if (a0 >= n1) break;
            const int a1 = a0 + lane;
            if (a1 < n1 && a1 < max_candidates) taken = taken || (pres[a1 * CODE_RES_INTS + CODE_RES_STATE] == CODE_ROW && pres[a1 * CODE_RES_INTS + 4] == root);
        }
    if (__ballot(taken)) return;
    rs_load_tables(s.rs, DM_EXP, DM_LOG, 8, lane);
    // the outer corners of the four extremes, doubled
    int cx[4], cy[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const u64 e = ext[((size_t)pg * runcap + root) * 4 + j];
        const int x = (int)(e & 0xffffull), yf = (int)((e >> 16) & 0xffffull), y = (j == 0 || j == 3) ? yf : 65535 - yf;
        cx[j] = 2 * (x + ((j == 1 || j == 2) ? 1 : 0));
        cy[j] = 2 * (y + (j >= 2 ? 1 : 0));
    }
    // every (size <= max_size, rotation) in reach: the smallest (timing mismatches, L misses, size, k); R C grows with the size
    i64 best = -1;
    const i64 lo_m = (i64)min_module, hi_m = (i64)max_module;
#pragma unroll 1
    for (int sz = 0; sz < DML_NUM_SIZES; ++sz) {
        const int R = clampi(DML_SIZES[sz * 8 + 0], 8, DML_MAX_SIDE), C = clampi(DML_SIZES[sz * 8 + 1], 8, DML_MAX_SIDE);
        const int nr = clampi(DML_SIZES[sz * 8 + 4], 1, DML_MAX_REGIONS), nc = clampi(DML_SIZES[sz * 8 + 5], 1, DML_MAX_REGIONS);
        if (R > max_size) continue;
        const int RH = R / nr, RW = C / nc;
#pragma unroll 1
        for (int k = 0; k < 4; ++k) {
            const int ox = cx[(k + 3) & 3], oy = cy[(k + 3) & 3];
            const int ux = cx[k] - ox, uy = cy[k] - oy, vx = cx[(k + 2) & 3] - ox, vy = cy[(k + 2) & 3] - oy;
            const i64 lu = (i64)ux * ux + (i64)uy * uy, lv = (i64)vx * vx + (i64)vy * vy;
            const i64 ulo = 2 * R * lo_m, uhi = 2 * R * hi_m, vlo = 2 * C * lo_m, vhi = 2 * C * hi_m;
            if (lu < ulo * ulo || lu > uhi * uhi || lv < vlo * vlo || lv > vhi * vhi) continue;
            const i64 qa = lu * C * C, qb = lv * R * R;   // (< 2^45)
            if (16 * (qa > qb ? qa : qb) > 25 * (qa < qb ? qa : qb)) continue;
            DmlGrid g;
            g.R = R; g.den = 4 * R * C; g.X = ox >> 1; g.Y = oy >> 1; g.vxr = vx * R; g.vyr = vy * R; g.uxc = ux * C; g.uyc = uy * C;
            int misses = 0, timing = 0;
            for (int i = 0; i < 2 * DML_MAX_REGIONS; ++i) {   // the regions' clock rows (even i) and solid rows (odd i)
                if (i >= 2 * nr) break;
                const int r = (i >> 1) * RH + ((i & 1) ? RH - 1 : 0);
                for (int p = 0; p < DML_WORDS; ++p) {
                    if (p * 64 >= C) break;
                    const int c = p * 64 + lane;
                    const bool on = c < C;
                    const int v = on ? dml_sample(mpage, H, W, nw, g, r, c) : 0;
                    const bool solid = (i & 1) || c % RW == 0;
                    misses += __popcll(__ballot(on && solid && !v));
                    timing += __popcll(__ballot(on && !solid && v != ((c & 1) ^ 1)));
                }
            }
            for (int j = 0; j < 2 * DML_MAX_REGIONS; ++j) {   // the regions' solid columns (even j) and clock columns (odd j), without the rows above
                if (j >= 2 * nc) break;
                const int c = (j >> 1) * RW + ((j & 1) ? RW - 1 : 0);
                for (int p = 0; p < DML_WORDS; ++p) {
                    if (p * 64 >= R) break;
                    const int r = p * 64 + lane, lr = r % RH;
                    const bool on = r < R && lr != 0 && lr != RH - 1;
                    const int v = on ? dml_sample(mpage, H, W, nw, g, r, c) : 0;
                    misses += __popcll(__ballot(on && !(j & 1) && !v));
                    timing += __popcll(__ballot(on && (j & 1) && v != (r & 1)));
                }
            }
            const i64 key = ((i64)timing << 40) | ((i64)misses << 24) | (i64)(sz << 4) | (i64)k;   // (both counts < 2^13)
            if (best < 0 || key < best) best = key;
        }
    }
    if (best < 0) return;
    const int timing = (int)(best >> 40), misses = (int)((best >> 24) & 0xffff), k = (int)(best & 3), sz = clampi((int)((best >> 4) & 15), 0, DML_NUM_SIZES - 1);
    if (timing > timing_max || misses > solid_max) return;
    const int R = clampi(DML_SIZES[sz * 8 + 0], 8, DML_MAX_SIDE), C = clampi(DML_SIZES[sz * 8 + 1], 8, DML_MAX_SIDE);
    const int ndata = DML_SIZES[sz * 8 + 2], ncheck = DML_SIZES[sz * 8 + 3];
    const int nb = clampi(DML_SIZES[sz * 8 + 6], 1, DML_MAX_NB), total = ndata + ncheck, ec = ncheck / nb;
    if (total > DML_MAX_TOTAL || ndata > DM_MAX_DATA_ALL || ec < 2 || ec > DM_MAX_EC || (total + nb - 1) / nb > DML_MAX_BLOCK || total / nb <= ec) return;   // (the tables never say so)
    const int ox = cx[(k + 3) & 3], oy = cy[(k + 3) & 3];
    const int ux = cx[k] - ox, uy = cy[k] - oy, vx = cx[(k + 2) & 3] - ox, vy = cy[(k + 2) & 3] - oy;
    DmlGrid g;
    g.R = R; g.den = 4 * R * C; g.X = ox >> 1; g.Y = oy >> 1; g.vxr = vx * R; g.vyr = vy * R; g.uxc = ux * C; g.uyc = uy * C;
    // the quiet rings
    bool dirty = false;
    for (int q = 1; q <= DM_MAX_QUIET; ++q) {
        if (q > quiet) break;
        for (int p = 0; p < DML_WORDS; ++p) {
            const int t = p * 64 + lane - q;
            if (t < C + q) dirty = dirty || dml_sample(mpage, H, W, nw, g, -q, t) || dml_sample(mpage, H, W, nw, g, R - 1 + q, t);
            if (t < R + q) dirty = dirty || dml_sample(mpage, H, W, nw, g, t, -q) || dml_sample(mpage, H, W, nw, g, t, C - 1 + q);
        }
    }
    if (__ballot(dirty)) return;
    // the module rows: lanes over columns, a ballot per word
    for (int i = lane; i < DML_MAX_SIDE * DML_WORDS; i += 64) s.rows[i] = 0;
    __syncthreads();
#pragma unroll 1
    for (int r = 0; r < DML_MAX_SIDE; ++r) {
        if (r >= R) break;
        for (int p = 0; p < DML_WORDS; ++p) {
            if (p * 64 >= C) break;
            const int c = p * 64 + lane;
            const u64 word = __ballot(c < C && dml_sample(mpage, H, W, nw, g, r, c));
            if (lane == 0) s.rows[r * DML_WORDS + p] = word;
        }
    }
    __syncthreads();
    // codewords in placement order
    const int poff = DML_PLACE_OFF[sz];
#pragma unroll 1
    for (int i = lane; i < DML_RAW; i += 64) {
        int val = 0;
        if (i < total) {
            for (int bit = 0; bit < 8; ++bit) {
                const int at = poff + 8 * i + bit;
                const unsigned p = DML_PLACE[at >= 0 && at < DML_PLACE_N ? at : DML_PLACE_N - 1];
                const int pr = clampi((int)(p >> 8), 0, DML_MAX_SIDE - 1), pc = (int)(p & 255), pw = clampi(pc >> 6, 0, DML_WORDS - 1);
                val = (val << 1) | (int)((s.rows[pr * DML_WORDS + pw] >> (pc & 63)) & 1ull);
            }
        }
        s.raw[i] = (unsigned char)val;
    }
    __syncthreads();
    // block blk is the stream positions blk, blk + nb, ...; its last ec codewords are its check codewords.  The corrected data goes back
    // to its stream positions: raw[0 .. ndata) becomes the symbol's data
    int errors = 0;
    for (int blk = 0; blk < DML_MAX_NB; ++blk) {
        if (blk >= nb) break;
        const int len = (total - blk + nb - 1) / nb, nd = len - ec;
#pragma unroll
        for (int p0 = 0; p0 < DM_BLK; p0 += 64) {
            const int p = p0 + lane;
            if (p < len) s.rs.blk[p] = s.raw[clampi(blk + p * nb, 0, DML_RAW - 1)];
        }
        __syncthreads();
        const int got = rs_correct_block(s.rs, len, ec, 1, lane);
        if (got < 0) return;
        errors += got;
#pragma unroll
        for (int p0 = 0; p0 < DM_BLK; p0 += 64) {
            const int p = p0 + lane;
            if (p < nd) s.raw[clampi(blk + p * nb, 0, DML_RAW - 1)] = s.rs.blk[p];
        }
        __syncthreads();
    }
    int slot = lane == 0 ? atomicAdd(&nrows[pg], 1) : 0;
    slot = __shfl(slot, 0);
    if (slot >= 0 && slot < max_codes) {
        unsigned char* od = rowdata + ((size_t)pg * max_codes + slot) * DM_MAX_DATA_ALL;
        for (int j = lane; j < DM_MAX_DATA_ALL; j += 64) od[j] = j < ndata ? s.raw[j] : (unsigned char)0;
    }
    if (lane == 0) {
        int x0 = 0, x1 = 0, y0 = 0, y1 = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int qx = (ox + ((c & 1) ? ux : 0) + ((c & 2) ? vx : 0)) >> 1, qy = (oy + ((c & 1) ? uy : 0) + ((c & 2) ? vy : 0)) >> 1;
            x0 = c == 0 || qx < x0 ? qx : x0; x1 = c == 0 || qx > x1 ? qx : x1;
            y0 = c == 0 || qy < y0 ? qy : y0; y1 = c == 0 || qy > y1 ? qy : y1;
        }
        int* o = pres + (size_t)(max_candidates + a) * CODE_RES_INTS;
        o[0] = clampi(y0, 0, H - 1); o[1] = clampi(x0, 0, W - 1); o[2] = clampi(y1 - 1, 0, H - 1); o[3] = clampi(x1 - 1, 0, W - 1); o[4] = root;
        o[5] = R; o[6] = C; o[7] = ndata; o[8] = errors; o[9] = k; o[10] = timing; o[11] = misses; o[12] = 0; o[14] = slot; o[CODE_RES_STATE] = CODE_ROW;
    }
}

// 6: tmp [B][max_codes][6] = y0, x0, y1, x1, root, slot
__global__ __launch_bounds__(256) void dm_output_kernel(const int* res_all, const unsigned char* resdata_all, const int* ncand, int max_candidates, int max_codes,
                                                        int* tmp_all, int* counts, int* codes, int* data, int* candidate_counts) {
    __shared__ CodeOutLds<DM_MAX_CODES> s;
    const int pg = blockIdx.x;
    const int* res = res_all + (size_t)pg * max_candidates * CODE_RES_INTS;
    const int n = code_output_rows(s, res, ncand[pg], max_candidates, max_codes, tmp_all + (size_t)pg * max_codes * 6, codes + (size_t)pg * max_codes * 12,
                                   counts + pg, candidate_counts ? candidate_counts + pg : nullptr);
    if (n > max_codes) return;
    const unsigned char* rd = resdata_all + (size_t)pg * max_candidates * DM_MAX_DATA;
    code_output_data(s, n, max_candidates, DM_MAX_DATA, data + (size_t)pg * max_codes * DM_MAX_DATA,
                     [=](int slot, int j) -> int { return j < res[slot * CODE_RES_INTS + 7] ? rd[(size_t)slot * DM_MAX_DATA + j] : 0; });
}

// 6 of lumina_ocr_datamatrix_sizes: both stages' records (2 max_candidates slots a page) through the same output stage; byte rows
__global__ __launch_bounds__(256) void dm_sizes_output_kernel(const int* res_all, const unsigned char* resdata_all, const unsigned char* rowdata_all,
                                                              const int* ncand, int max_candidates, int max_codes, int* tmp_all, int* counts, int* codes,
                                                              unsigned char* data, int* candidate_counts) {
    __shared__ CodeOutLds<DM_MAX_CODES> s;
    const int pg = blockIdx.x, slots = 2 * max_candidates;
    const int* res = res_all + (size_t)pg * slots * CODE_RES_INTS;
    const int n = code_output_rows(s, res, slots, slots, max_codes, tmp_all + (size_t)pg * max_codes * 6, codes + (size_t)pg * max_codes * 12, counts + pg,
                                   (int*)nullptr);
    if (threadIdx.x == 0 && candidate_counts) candidate_counts[pg] = ncand[pg];   // stage 1's
    if (n > max_codes) return;
    const unsigned char* rd = resdata_all + (size_t)pg * max_candidates * DM_MAX_DATA;
    const unsigned char* rows = rowdata_all + (size_t)pg * max_codes * DM_MAX_DATA_ALL;
    code_output_data(s, n, slots, DM_MAX_DATA_ALL, data + (size_t)pg * max_codes * DM_MAX_DATA_ALL, [=](int slot, int j) -> unsigned char {
        const int* r = res + slot * CODE_RES_INTS;
        if (j >= r[7]) return 0;
        if (slot < max_candidates) return j < DM_MAX_DATA ? rd[(size_t)slot * DM_MAX_DATA + j] : (unsigned char)0;
        return rows[(size_t)clampi(r[14], 0, max_codes - 1) * DM_MAX_DATA_ALL + j];
    });
}

}  // namespace

// the workspace's regions: one layout sizes it (datamatrix_workspace_bytes) and carves it (datamatrix_launch)
struct DmWorkspace {
    Components c;   // c.ext: at a root, its component's four diagonal extremes, packed
    int* ncand; int* cands; int* res; unsigned char* resdata; int* tmp;
};
static DmWorkspace datamatrix_layout(Arena& a, int B, int H, int W, int max_candidates, int max_codes) {
    DmWorkspace w;
    w.c = components_layout(a, B, H, W, true);
    w.c.ext = a.take<unsigned long long>((size_t)B * run_cap(H, W) * 4);
    w.ncand = a.take<int>((size_t)B);
    w.cands = a.take<int>((size_t)B * max_candidates);
    w.res = a.take<int>((size_t)B * max_candidates * CODE_RES_INTS);
    w.resdata = a.take<unsigned char>((size_t)B * max_candidates * DM_MAX_DATA);
    w.tmp = a.take<int>((size_t)B * max_codes * 6);
    return w;
}

static bool datamatrix_args_ok(int B, int H, int W, int max_candidates, int max_codes) {
    return page_args_ok(B, H, W) && max_codes >= 1 && max_codes <= DM_MAX_CODES && max_candidates >= 1 && max_candidates <= DM_MAX_CANDIDATES;
}

bool dm_params_ok(int min_module, int max_module, int quiet, int timing_max, int solid_max, int max_candidates, int max_codes) {
    return min_module >= 1 && max_module >= min_module && max_module <= DM_MAX_MODULE && quiet >= 0 && quiet <= DM_MAX_QUIET && timing_max >= 0 &&
           timing_max <= DM_MAX_TIMING && solid_max >= 0 && solid_max <= DM_MAX_TIMING && max_candidates >= 1 && max_candidates <= DM_MAX_CANDIDATES &&
           max_codes >= 1 && max_codes <= DM_MAX_CODES;
}

size_t datamatrix_workspace_bytes(int B, int H, int W, int max_candidates, int max_codes) {
    if (!datamatrix_args_ok(B, H, W, max_candidates, max_codes)) return 0;
    Arena a;
    datamatrix_layout(a, B, H, W, max_candidates, max_codes);
    return a.off;
}

hipError_t datamatrix_launch(const DmParams& p, void* workspace, size_t ws_bytes, hipStream_t st) {
    const int B = p.B, H = p.H, W = p.W;
    if (!datamatrix_args_ok(B, H, W, p.max_candidates, p.max_codes) ||
        !dm_params_ok(p.min_module, p.max_module, p.quiet, p.timing_max, p.solid_max, p.max_candidates, p.max_codes))
        return hipErrorInvalidValue;
    if (!p.rgb || !p.codes || !p.data || !p.counts) return hipErrorInvalidValue;
    Arena a(workspace, ws_bytes);
    DmWorkspace w = datamatrix_layout(a, B, H, W, p.max_candidates, p.max_codes);
    if (a.overflow) return hipErrorOutOfMemory;
    const int nw = (W + 63) / 64;
    const size_t runcap = run_cap(H, W);
    hipError_t e;
    if ((e = hipMemsetAsync(w.ncand, 0, sizeof(int) * (size_t)B, st)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(w.res, 0, sizeof(int) * (size_t)B * p.max_candidates * CODE_RES_INTS, st)) != hipSuccess) return e;
    if ((e = components_launch(w.c, p.rgb, p.mask_in, p.mask_out, B, H, W, p.threshold, st)) != hipSuccess) return e;
    const int rows = B * H;
    hipLaunchKernelGGL(dm_candidates_kernel, row_wave_grid(rows), dim3(256), 0, st, w.c.runoff, w.c.parent, w.c.box, w.c.area, H, runcap, p.min_module, p.max_module,
                       8, 52, p.max_candidates, w.ncand, w.cands, rows);
    hipLaunchKernelGGL(dm_decode_kernel, dim3(p.max_candidates, B), dim3(64), 0, st, w.c.mask, w.cands, w.ncand, w.c.ext, H, W, nw, runcap, p.max_candidates,
                       p.min_module, p.max_module, p.quiet, p.timing_max, p.solid_max, p.max_candidates, w.res, w.resdata);
    hipLaunchKernelGGL(dm_output_kernel, dim3(B), dim3(256), 0, st, w.res, w.resdata, w.ncand, p.max_candidates, p.max_codes, w.tmp, p.counts, p.codes, p.data,
                       p.candidate_counts);
    return hipGetLastError();
}

// ---- lumina_ocr_datamatrix_sizes: stage 1 as above, stage 2 for 64 x 64 .. max_size, one output stage ----
struct DmSizesWorkspace {
    Components c;
    int* ncand; int* cands; int* ncand2; int* cands2; int* nrows; int* res; unsigned char* resdata; unsigned char* rowdata; int* tmp;
};
static DmSizesWorkspace datamatrix_sizes_layout(Arena& a, int B, int H, int W, int max_candidates, int max_codes) {
    DmSizesWorkspace w;
    w.c = components_layout(a, B, H, W, true);
    w.c.ext = a.take<unsigned long long>((size_t)B * run_cap(H, W) * 4);
    w.ncand = a.take<int>((size_t)B * 3);   // ncand, ncand2, nrows: one memset
    w.ncand2 = w.ncand + B;
    w.nrows = w.ncand + 2 * (size_t)B;
    w.cands = a.take<int>((size_t)B * max_candidates);
    w.cands2 = a.take<int>((size_t)B * max_candidates);
    w.res = a.take<int>((size_t)B * 2 * max_candidates * CODE_RES_INTS);
    w.resdata = a.take<unsigned char>((size_t)B * max_candidates * DM_MAX_DATA);
    w.rowdata = a.take<unsigned char>((size_t)B * max_codes * DM_MAX_DATA_ALL);
    w.tmp = a.take<int>((size_t)B * max_codes * 6);
    return w;
}

// The placement of a size's codeword bits, (row << 8 | col) in symbol coordinates, by the standard's walk over the data-region matrix
// (the restatement of utils/datamatrix.py's mapping_placement and to_symbol; tests/test_dm_sizes_tables.py compares the two through
// lumina_ocr_datamatrix_placement) -> the number of entries, 0 when the walk leaves the matrix or visits a module twice.
static int dml_placement(int R, int C, int nr, int nc, unsigned short* out, int cap) {
    if (nr < 1 || nc < 1 || R / nr < 3 || C / nc < 3) return 0;
    const int nrow = R - 2 * nr, ncol = C - 2 * nc, dh = R / nr - 2, dw = C / nc - 2;
    std::vector<unsigned char> seen((size_t)nrow * ncol, 0);
    int n = 0;
    bool bad = false;
    auto inside = [&](int r, int c) { return r >= 0 && r < nrow && c >= 0 && c < ncol; };
    auto put = [&](int r, int c) {
        if (!inside(r, c) || seen[(size_t)r * ncol + c] || n >= cap) { bad = true; return; }
        seen[(size_t)r * ncol + c] = 1;
        out[n++] = (unsigned short)(((r + 1 + 2 * (r / dh)) << 8) | (c + 1 + 2 * (c / dw)));
    };
    auto utah = [&](int row, int col) {
        static const int off[8][2] = {{-2, -2}, {-2, -1}, {-1, -2}, {-1, -1}, {-1, 0}, {0, -2}, {0, -1}, {0, 0}};
        for (int i = 0; i < 8; ++i) {
            int r = row + off[i][0], c = col + off[i][1];
            if (r < 0) { r += nrow; c += 4 - ((nrow + 4) % 8); }
            if (c < 0) { c += ncol; r += 4 - ((ncol + 4) % 8); }
            put(r, c);
        }
    };
    auto corner = [&](int which) {
        const int a = nrow, b = ncol;
        const int cells[4][8][2] = {
            {{a - 1, 0}, {a - 1, 1}, {a - 1, 2}, {0, b - 2}, {0, b - 1}, {1, b - 1}, {2, b - 1}, {3, b - 1}},
            {{a - 3, 0}, {a - 2, 0}, {a - 1, 0}, {0, b - 4}, {0, b - 3}, {0, b - 2}, {0, b - 1}, {1, b - 1}},
            {{a - 3, 0}, {a - 2, 0}, {a - 1, 0}, {0, b - 2}, {0, b - 1}, {1, b - 1}, {2, b - 1}, {3, b - 1}},
            {{a - 1, 0}, {a - 1, b - 1}, {0, b - 3}, {0, b - 2}, {0, b - 1}, {1, b - 3}, {1, b - 2}, {1, b - 1}}};
        for (int i = 0; i < 8; ++i) put(cells[which][i][0], cells[which][i][1]);
    };
    auto fresh = [&](int r, int c) { return !(inside(r, c) && seen[(size_t)r * ncol + c]); };
    int row = 4, col = 0;
    do {
        if (row == nrow && col == 0) corner(0);
        if (row == nrow - 2 && col == 0 && ncol % 4 != 0) corner(1);
        if (row == nrow - 2 && col == 0 && ncol % 8 == 4) corner(2);
        if (row == nrow + 4 && col == 2 && ncol % 8 == 0) corner(3);
        do {   // up and to the right
            if (row < nrow && col >= 0 && fresh(row, col)) utah(row, col);
            row -= 2; col += 2;
        } while (row >= 0 && col < ncol && !bad);
        row += 1; col += 3;
        do {   // down and to the left
            if (row >= 0 && col < ncol && fresh(row, col)) utah(row, col);
            row += 2; col -= 2;
        } while (row < nrow && col >= 0 && !bad);
        row += 3; col += 1;
    } while ((row < nrow || col < ncol) && !bad);
    return bad ? 0 : n;
}

// the nine sizes' placements, built once a process; empty when a walk fails or a size does not fill its part of the table
static const std::vector<unsigned short>& dml_place_table() {
    static const std::vector<unsigned short> table = [] {
        std::vector<unsigned short> t(DML_PLACE_N, 0);
        for (int s = 0; s < DML_NUM_SIZES; ++s) {
            const unsigned short* z = DML_SIZES_HOST + s * 8;
            const int want = DML_PLACE_OFF_HOST[s + 1] - DML_PLACE_OFF_HOST[s];
            if (want != 8 * (z[2] + z[3]) || dml_placement(z[0], z[1], z[4], z[5], t.data() + DML_PLACE_OFF_HOST[s], want) != want) return std::vector<unsigned short>();
        }
        return t;
    }();
    return table;
}

int datamatrix_placement(int side, unsigned short* out, int cap) {
    const std::vector<unsigned short>& t = dml_place_table();
    if (t.empty() || !out) return 0;
    for (int s = 0; s < DML_NUM_SIZES; ++s)
        if (DML_SIZES_HOST[s * 8] == side) {
            const int n = DML_PLACE_OFF_HOST[s + 1] - DML_PLACE_OFF_HOST[s];
            if (n > cap) return 0;
            std::copy(t.begin() + DML_PLACE_OFF_HOST[s], t.begin() + DML_PLACE_OFF_HOST[s + 1], out);
            return n;
        }
    return 0;
}

// DML_PLACE of the current device, copied before the first launch that reads it (a blocking copy under a lock: later launches on any
// stream find it there)
static hipError_t dml_upload_once() {
    static std::mutex lock;
    static bool done[64] = {};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64) return hipErrorInvalidDevice;
    std::lock_guard<std::mutex> guard(lock);
    if (done[dev]) return hipSuccess;
    const std::vector<unsigned short>& t = dml_place_table();
    if (t.empty()) return hipErrorUnknown;
    if ((e = hipMemcpyToSymbol(HIP_SYMBOL(DML_PLACE), t.data(), sizeof(unsigned short) * DML_PLACE_N)) != hipSuccess) return e;
    done[dev] = true;
    return hipSuccess;
}

bool dm_max_size_ok(int max_size) { return max_size >= DM_MIN_MAX_SIZE && max_size <= DM_MAX_MAX_SIZE; }

size_t datamatrix_sizes_workspace_bytes(int B, int H, int W, int max_candidates, int max_codes) {
    if (!datamatrix_args_ok(B, H, W, max_candidates, max_codes)) return 0;
    Arena a;
    datamatrix_sizes_layout(a, B, H, W, max_candidates, max_codes);
    return a.off;
}

hipError_t datamatrix_sizes_launch(const DmSizesParams& p, void* workspace, size_t ws_bytes, hipStream_t st) {
    const int B = p.B, H = p.H, W = p.W;
    if (!datamatrix_args_ok(B, H, W, p.max_candidates, p.max_codes) ||
        !dm_params_ok(p.min_module, p.max_module, p.quiet, p.timing_max, p.solid_max, p.max_candidates, p.max_codes) || !dm_max_size_ok(p.max_size))
        return hipErrorInvalidValue;
    if (!p.rgb || !p.codes || !p.data_all || !p.counts) return hipErrorInvalidValue;
    Arena a(workspace, ws_bytes);
    DmSizesWorkspace w = datamatrix_sizes_layout(a, B, H, W, p.max_candidates, p.max_codes);
    if (a.overflow) return hipErrorOutOfMemory;
    const int nw = (W + 63) / 64;
    const size_t runcap = run_cap(H, W);
    hipError_t e;
    if ((e = hipMemsetAsync(w.ncand, 0, sizeof(int) * (size_t)B * 3, st)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(w.res, 0, sizeof(int) * (size_t)B * 2 * p.max_candidates * CODE_RES_INTS, st)) != hipSuccess) return e;
    if ((e = components_launch(w.c, p.rgb, p.mask_in, p.mask_out, B, H, W, p.threshold, st)) != hipSuccess) return e;
    if (p.max_size >= 64 && (e = dml_upload_once()) != hipSuccess) return e;
    const int rows = B * H;
    hipLaunchKernelGGL(dm_candidates_kernel, row_wave_grid(rows), dim3(256), 0, st, w.c.runoff, w.c.parent, w.c.box, w.c.area, H, runcap, p.min_module, p.max_module,
                       8, 52, p.max_candidates, w.ncand, w.cands, rows);
    hipLaunchKernelGGL(dm_decode_kernel, dim3(p.max_candidates, B), dim3(64), 0, st, w.c.mask, w.cands, w.ncand, w.c.ext, H, W, nw, runcap, p.max_candidates,
                       p.min_module, p.max_module, p.quiet, p.timing_max, p.solid_max, 2 * p.max_candidates, w.res, w.resdata);
    if (p.max_size >= 64) {
        hipLaunchKernelGGL(dm_candidates_kernel, row_wave_grid(rows), dim3(256), 0, st, w.c.runoff, w.c.parent, w.c.box, w.c.area, H, runcap, p.min_module,
                           p.max_module, 64, 144, p.max_candidates, w.ncand2, w.cands2, rows);
        hipLaunchKernelGGL(dm_large_kernel, dim3(p.max_candidates, B), dim3(64), 0, st, w.c.mask, w.cands2, w.ncand2, w.ncand, w.c.ext, H, W, nw, runcap,
                           p.max_candidates, p.max_codes, p.min_module, p.max_module, p.quiet, p.timing_max, p.solid_max, p.max_size, w.res, w.nrows, w.rowdata);
    }
    hipLaunchKernelGGL(dm_sizes_output_kernel, dim3(B), dim3(256), 0, st, w.res, w.resdata, w.rowdata, w.ncand, p.max_candidates, p.max_codes, w.tmp, p.counts,
                       p.codes, p.data_all, p.candidate_counts);
    return hipGetLastError();
}
