// Aztec codes (compact 1-4 layers, full-range 1-11 layers; full-range 12-32 layers behind lumina_ocr_aztec_layers) on the GPU
// (gfx950): the symbols of a page as (x0, y0, x1, y1, layers, compact, codeword width, ndata, errors, rotation, mode-message errors,
// mismatches) with their corrected data codewords, in a canonical order.  Everything is integer and every reduction is order-free
// (min / max / add / xor, ballots), so the lists equal the sequential definition restated in tests/aztec_reference.py
// (tests/aztec_layers_reference.py for the second stage).
//
// All stream-ordered kernels, no host round trip:
//   1-3 components_launch (runs.h)      the mask (or the one the caller already has), its run list, the 8-connected components; a run is
//                 its own area; every run learns its root, and box and area are accumulated there
//   4 az_finders  one wave per row, lanes over the row's roots: a solid square core whose neighbours on its centre row both belong to
//                 one concentric component of five times its side -> counted, gathered per page
//   5 az_decode   one wave per (page, finder).  A frame is the ring's centre, a slope and a pitch; a point of it is a pixel by
//                 64-bit multiplications and shifts.  Frames are scored with lanes over modules: first on the bullseye for either
//                 kind, whose corner marks give the rotation and whose mode message (GF(16)) gives layers and data words; then,
//                 the size known, on the symbol's outline (ink just inside it, none just outside) and the centre reference lines.
//                 Lane r samples module row r as one 64-bit word; lanes gather the codewords through the layer spiral from the
//                 rows in LDS; the one block goes through rs.h.  Every loop has a constant bound, every LDS and page index is
//                 clamped, and no wave waits for another (a work-group is one wave)
//   5b az_layers  (lumina_ocr_aztec_layers alone) one wave per (page, finder): a full-range finder of 12 .. max_layers layers that
//                 az_decode left pending gets a finer frame (slope and pitch in 1024ths), refined outwards along the centre reference
//                 lines and finished on the outline; lane r samples rows r, r + 64, r + 128 as three words each; GF(1024) up to 22
//                 layers, GF(4096) above.  The same rules: constant loop bounds, clamped indices, no wave waits for another
//   6 az_output   one work-group per page (code_output.h): valid finders counted, gathered, rank-sorted by (y0, x0, y1, x1, root)
#include "aztec.h"
#include "code_output.h"
#include "aztec_tables.h"
#include "aztec_tables12.h"
#include "rs.h"
#include "runs.h"

namespace {

typedef unsigned long long u64;
typedef long long i64;

// a finder's result (code_output.h): y0, x0, y1, x1, root, layers, compact, width, ndata, errors, rotation, mode errors, mismatches, state
// (CODE_PENDING: for az_layers, which then finds the bullseye's frame t0, k0 in the last two)
constexpr int AZ_MAX_WORDS = 320, AZ_MAX_EC = 318, AZ_MAX_M = 10, AZ_MAX_LAYERS = 11, AZ_MAX_SIDE = 61;
constexpr int AZL_MAX_WORDS = 1664, AZL_MAX_EC = 1662, AZL_MAX_M = 12, AZL_MAX_LAYERS = 32, AZL_MAX_SIDE = 151, AZL_SPAN = 4, AZL_FRAMES = 81;

// 4: finders [B][max_finders][2] = the core's root, the ring's root
__global__ __launch_bounds__(256) void az_finders_kernel(const int* runoff, const unsigned short* rxs, const unsigned short* rxe, const int* parent, const int4* box,
                                                         const int* area, int H, size_t runcap, int min_module, int max_module, int centre_tol, int ring_tol,
                                                         int max_finders, int* nfind, int* finders, int rows_total) {
    int pg, row, lane;
    if (!row_wave(H, rows_total, pg, row, lane)) return;
    const int* ro = runoff + (size_t)pg * (H + 1);
    const size_t rb = (size_t)pg * runcap;
    for (int id = ro[row] + lane; id < ro[row + 1]; id += 64) {
        if (parent[rb + id] != id) continue;
        const int4 bx = box[rb + id];   // x0, x1, y0, y1
        const int w = bx.y - bx.x + 1, h = bx.w - bx.z + 1;
        if (w < min_module || h < min_module || w > max_module || h > max_module) continue;
        if (4 * iabs(w - h) > (w > h ? w : h) || 4 * area[rb + id] < 3 * w * h) continue;
        const int cy = clampi((bx.z + bx.w) >> 1, 0, H - 1), cx = (bx.x + bx.y) >> 1;
        const int lo = ro[cy], hi = ro[cy + 1];
        // the last run of the centre row that starts at or before cx
        int a = lo, b = hi;   // the answer is in [a, b) when there is one
        for (int it = 0; it < 17; ++it) {
            if (b - a <= 1) break;
            const int mid = (a + b) >> 1;
            if (rxs[rb + mid] <= cx) a = mid; else b = mid;
        }
        if (a >= hi || a - 1 < lo || a + 1 >= hi) continue;
        if (rxs[rb + a] > cx || rxe[rb + a] < cx || uf_find(parent + rb, a) != id) continue;
        const int g = uf_find(parent + rb, a - 1);
        if (g == id || uf_find(parent + rb, a + 1) != g) continue;
        const int4 gx = box[rb + g];
        const int w5 = gx.y - gx.x + 1, h5 = gx.w - gx.z + 1;
        if (16 * iabs(5 * w - w5) > ring_tol * w5 || 16 * iabs(5 * h - h5) > ring_tol * h5) continue;
        if (80 * iabs(gx.x + gx.y - bx.x - bx.y) > 2 * centre_tol * w5 || 80 * iabs(gx.z + gx.w - bx.z - bx.w) > 2 * centre_tol * h5) continue;
        const i64 wh = (i64)w5 * h5, a25 = 25 * (i64)area[rb + g];
        if (12 * wh > a25 || a25 > 20 * wh) continue;
        const int idx = atomicAdd(&nfind[pg], 1);
        if (idx < max_finders) {
            finders[((size_t)pg * max_finders + idx) * 2 + 0] = id;
            finders[((size_t)pg * max_finders + idx) * 2 + 1] = g;
        }
    }
}

// a frame: the ring's centre (doubled pixels << 30), slope t / 128, pitch step k; a point (u, v) in quarter modules from the centre
struct AzFrame { i64 cx, cy, q; int t; };

__device__ __forceinline__ AzFrame az_frame(int cx2, int cy2, int s10, int t, int k) {
    AzFrame f;
    f.cx = (i64)cx2 << 30; f.cy = (i64)cy2 << 30; f.t = t;
    f.q = (((i64)s10 << 20) / (5 * (128 + iabs(t)))) * (256 + 2 * k);
    return f;
}
__device__ __forceinline__ void az_pixel(const AzFrame& f, int u, int v, i64& px, i64& py) {
    px = (f.cx + f.q * (i64)(128 * u - f.t * v)) >> 31;
    py = (f.cy + f.q * (i64)(f.t * u + 128 * v)) >> 31;
}
// the ink at a point; off the page reads clear
__device__ __forceinline__ int az_at(const u64* mpage, int H, int W, int nw, const AzFrame& f, int u, int v) {
    i64 px, py;
    az_pixel(f, u, v, px, py);
    if (px < 0 || py < 0 || px >= W || py >= H) return 0;
    return (int)((mpage[(size_t)py * nw + (size_t)(px >> 6)] >> (px & 63)) & 1ull);
}
// a symbol offset turned clockwise by r quarter turns
__device__ __forceinline__ void az_turn(int x, int y, int r, int& tx, int& ty) {
    tx = r == 0 ? x : r == 1 ? -y : r == 2 ? -x : y;
    ty = r == 0 ? y : r == 1 ? x : r == 2 ? -y : -x;
}

__device__ __forceinline__ int az_width(int layers) { return layers <= 2 ? 6 : layers <= 8 ? 8 : layers <= 22 ? 10 : 12; }
__device__ __forceinline__ int az_total_bits(bool compact, int layers) { return ((compact ? 88 : 112) + 16 * layers) * layers; }
__device__ __forceinline__ int az_modules(bool compact, int layers) {
    const int base = (compact ? 11 : 14) + 4 * layers;
    return compact ? base : base + 1 + 2 * ((base / 2 - 1) / 15);
}
// index of the matrix without the reference grid's lines -> the symbol's coordinate
__device__ __forceinline__ int az_grid(bool compact, int layers, int i) {
    if (compact) return i;
    const int half = 7 + 2 * layers, c = az_modules(false, layers) / 2;
    if (i >= half) { const int j = i - half; return c + j + j / 15 + 1; }
    const int j = half - 1 - i;
    return c - j - j / 15 - 1;
}
// bit b of the symbol's stream -> its module: layer 0 outermost, the left side going down, the bottom going right, the right side
// going up, the top going left; bit 2 j + k of a side is domino j, k modules inwards
template <int MAX_LAYERS, int MAX_COORD>
__device__ __forceinline__ void az_bit_pos(bool compact, int layers, int b, int& x, int& y) {
    int i = 0, row = 0;
    for (i = 0; i < MAX_LAYERS; ++i) {
        row = 4 * (layers - i) + (compact ? 9 : 12);
        if (b < 8 * row || i >= layers - 1) break;
        b -= 8 * row;
    }
    b = clampi(b, 0, 8 * row - 1);
    const int side = b / (2 * row), r = b % (2 * row), j = r >> 1, k = r & 1;
    const int low = 2 * i, high = (compact ? 11 : 14) + 4 * layers - 1 - 2 * i;
    const int mx = side == 0 ? low + k : side == 1 ? low + j : side == 2 ? high - k : high - j;
    const int my = side == 0 ? low + j : side == 1 ? high - k : side == 2 ? high - j : low + k;
    x = clampi(az_grid(compact, layers, mx), 0, MAX_COORD);
    y = clampi(az_grid(compact, layers, my), 0, MAX_COORD);
}

struct AzLds {
    u64 rows[64];
    RsLds<unsigned short, AZ_MAX_WORDS, AZ_MAX_EC, AZ_MAX_M> rs;
};

// ink on the square at d quarter modules, points every `step` quarter modules, corners included on all four sides (d / step * 2 + 1 <= 128 points a side)
__device__ __forceinline__ int az_square(const u64* mpage, int H, int W, int nw, const AzFrame& f, int d, int step, int lane) {
    int n = 0;
    const int cnt = 2 * d / step + 1;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int idx = lane + 64 * j, a = -d + step * idx;
        const bool on = idx < cnt;
        n += __popcll(__ballot(on && az_at(mpage, H, W, nw, f, a, -d))) + __popcll(__ballot(on && az_at(mpage, H, W, nw, f, a, d))) +
             __popcll(__ballot(on && az_at(mpage, H, W, nw, f, -d, a))) + __popcll(__ballot(on && az_at(mpage, H, W, nw, f, d, a)));
    }
    return n;
}

// 5: one wave per (page, finder): res [B][max_finders][CODE_RES_INTS], resdata [B][max_finders][data_stride].  A full-range finder of
// AZ_MAX_LAYERS < layers <= max_layers that ends without a row is left pending
__global__ __launch_bounds__(64) void az_decode_kernel(const u64* mask, const int* finders, const int* nfind, const int4* box, int H, int W, int nw, size_t runcap,
                                                       int max_finders, int quiet, int mark_max, int max_layers, int data_stride, int* res,
                                                       unsigned short* resdata) {
    __shared__ AzLds s;
    const int pg = blockIdx.y, a = blockIdx.x, lane = threadIdx.x;
    const int nf_page = nfind[pg];
    if (nf_page > max_finders || a >= nf_page || a >= AZ_MAX_FINDERS) return;
    const u64* mpage = mask + (size_t)pg * H * nw;
    const int root = clampi(finders[((size_t)pg * max_finders + a) * 2 + 0], 0, (int)runcap - 1);
    const int ring = clampi(finders[((size_t)pg * max_finders + a) * 2 + 1], 0, (int)runcap - 1);
    const int4 gx = box[(size_t)pg * runcap + ring];   // x0, x1, y0, y1
    const int cx2 = gx.x + gx.y + 1, cy2 = gx.z + gx.w + 1, s10 = (gx.y - gx.x + 1) + (gx.w - gx.z + 1);
    rs_load_tables(s.rs, AZ_EXP + AZ_EXP_OFF[0], AZ_LOG + AZ_LOG_OFF[0], 4, lane);
    // either kind: the bullseye's best frame, the rotation, the mode message
    i64 kind_best = -1;
    int pend_layers = 0, pend_ndata = 0, pend_rot = 0, pend_merr = 0, pend_mism = 0, pend_t = 0, pend_k = 0;
#pragma unroll 1
    for (int full = 0; full < 2; ++full) {
        const int sd = full ? 7 : 5, side = 2 * sd - 1;
        int best = -1;
#pragma unroll 1
        for (int k = -12; k <= 12; k += 2) {
#pragma unroll 1
            for (int t = -4; t <= 4; t += 4) {
                const AzFrame f = az_frame(cx2, cy2, s10, t, k);
                int mism = 0;
                for (int j = 0; j < 3; ++j) {
                    const int idx = lane + 64 * j, dx = idx % side - (sd - 1), dy = idx / side - (sd - 1);
                    const bool on = idx < side * side;
                    const int want = ((iabs(dx) > iabs(dy) ? iabs(dx) : iabs(dy)) & 1) ^ 1;
                    mism += __popcll(__ballot(on && az_at(mpage, H, W, nw, f, 4 * dx, 4 * dy) != want));
                }
                const int key = (mism << 16) | (iabs(k) << 12) | (iabs(t) << 9) | ((k + 12) << 4) | (t + 6);
                if (best < 0 || key < best) best = key;
            }
        }
        const int bull = best >> 16;
        const AzFrame f = az_frame(cx2, cy2, s10, (best & 15) - 6, ((best >> 4) & 31) - 12);
        // the twelve corner modules of the mode ring
        const int corner = (lane >> 2) & 3, which = lane & 3;   // lanes 0 .. 15, `which` 3 unused
        const int sx = (corner == 1 || corner == 2) ? 1 : -1, sy = corner >= 2 ? 1 : -1;
        const int mx = sx * (which == 1 ? sd - 1 : sd), my = sy * (which == 2 ? sd - 1 : sd);
        const int dark = corner == 0 || (corner == 1 && which != 1) || (corner == 2 && which == 2);
        int rot = 0, mm = 99;
        for (int r = 0; r < 4; ++r) {
            int tx, ty;
            az_turn(mx, my, r, tx, ty);
            const int got = __popcll(__ballot(lane < 16 && which < 3 && az_at(mpage, H, W, nw, f, 4 * tx, 4 * ty) != dark));
            if (got < mm) { mm = got; rot = r; }
        }
        if (bull + mm > mark_max) continue;
        // the mode message, clockwise from the top side's left end
        const int n = full ? 10 : 7, nwords = n, ecw = full ? 6 : 5;
        int bit = 0;
        if (lane < 4 * n) {
            const int sde = lane / n, jj = lane % n, i = sde < 2 ? jj : n - 1 - jj;
            const int o = full ? -5 + i + i / 5 : -3 + i;
            const int px = sde == 0 ? o : sde == 1 ? sd : sde == 2 ? o : -sd, py = sde == 0 ? -sd : sde == 1 ? o : sde == 2 ? sd : o;
            int tx, ty;
            az_turn(px, py, rot, tx, ty);
            bit = az_at(mpage, H, W, nw, f, 4 * tx, 4 * ty);
        }
        const u64 ball = __ballot(bit);
        __syncthreads();
        if (lane < nwords) {
            const int v = (int)((ball >> (4 * lane)) & 15ull);
            s.rs.blk[lane] = (unsigned short)(((v & 1) << 3) | ((v & 2) << 1) | ((v & 4) >> 1) | ((v & 8) >> 3));
        }
        __syncthreads();
        const int merr = rs_correct_block(s.rs, nwords, ecw, 1, lane);
        if (merr < 0) continue;
        int layers, ndata;
        if (!full) {
            const int v = (s.rs.blk[0] << 4) | s.rs.blk[1];
            layers = (v >> 6) + 1; ndata = (v & 63) + 1;
        } else {
            const int v = (s.rs.blk[0] << 12) | (s.rs.blk[1] << 8) | (s.rs.blk[2] << 4) | s.rs.blk[3];
            layers = (v >> 11) + 1; ndata = (v & 2047) + 1;
            if (layers > AZ_MAX_LAYERS) {
                if (layers <= max_layers && az_total_bits(false, layers) / az_width(layers) - ndata >= 2) {
                    pend_layers = layers; pend_ndata = ndata; pend_rot = rot; pend_merr = merr; pend_mism = bull + mm;
                    pend_t = (best & 15) - 6; pend_k = ((best >> 4) & 31) - 12;
                }
                continue;
            }
        }
        if (az_total_bits(!full, layers) / az_width(layers) - ndata < 2) continue;
        // (mismatches, mode errors, full) | rotation, layers, ndata
        const i64 key = ((i64)(bull + mm) << 40) | ((i64)merr << 32) | ((i64)full << 31) | ((i64)rot << 20) | ((i64)layers << 12) | (i64)ndata;
        if (kind_best < 0 || key < kind_best) kind_best = key;
    }
    if (pend_layers && lane == 0) {   // (a row of this finder overwrites it)
        int* o = res + ((size_t)pg * max_finders + a) * CODE_RES_INTS;
        o[5] = pend_layers; o[8] = pend_ndata; o[10] = pend_rot; o[11] = pend_merr; o[12] = pend_mism; o[CODE_RES_STATE] = CODE_PENDING; o[14] = pend_t; o[15] = pend_k;
    }
    if (kind_best < 0) return;
    const int mism = (int)(kind_best >> 40), merr = (int)((kind_best >> 32) & 255), rot = (int)((kind_best >> 20) & 3);
    const bool compact = !((kind_best >> 31) & 1);
    const int layers = clampi((int)((kind_best >> 12) & 255), 1, compact ? 4 : AZ_MAX_LAYERS), ndata = (int)(kind_best & 4095);
    const int n = az_modules(compact, layers), h = n / 2, width = az_width(layers);
    const int total = az_total_bits(compact, layers) / width, pad = az_total_bits(compact, layers) % width, ec = total - ndata;
    if (n > AZ_MAX_SIDE || total > AZ_MAX_WORDS || ndata < 1 || ndata > AZ_MAX_DATA || ec < 2 || ec > AZ_MAX_EC) return;   // (the formulas never say so)
    // the frame of the whole symbol: nothing just outside its outline, the most ink just inside it, the centre lines alternating
    i64 best = -1;
#pragma unroll 1
    for (int k = -12; k <= 12; ++k) {
#pragma unroll 1
        for (int t = -6; t <= 6; ++t) {
            const AzFrame f = az_frame(cx2, cy2, s10, t, k);
            if (az_square(mpage, H, W, nw, f, 4 * h + 3, 2, lane)) continue;
            const int in = az_square(mpage, H, W, nw, f, 4 * h + 1, 2, lane);
            int ref = 0;
            if (!compact) {
                const int span = h - 7;   // distances 8 .. h
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int idx = lane + 64 * j, d = 8 + idx % span, dir = idx / span;
                    const int u = dir == 0 ? d : dir == 1 ? -d : 0, v = dir == 2 ? d : dir == 3 ? -d : 0;
                    ref += __popcll(__ballot(idx < 4 * span && az_at(mpage, H, W, nw, f, 4 * u, 4 * v) != ((d & 1) ^ 1)));
                }
            }
            const i64 key = ((i64)ref << 26) | ((i64)(1023 - in) << 16) | (iabs(k) << 12) | (iabs(t) << 9) | ((k + 12) << 4) | (t + 6);
            if (best < 0 || key < best) best = key;
        }
    }
    if (best < 0) return;
    const int ref = (int)(best >> 26);
    const AzFrame f = az_frame(cx2, cy2, s10, (int)(best & 15) - 6, (int)((best >> 4) & 31) - 12);
    // the quiet rings, at the modules' centres
    bool dirty = false;
    for (int q = 1; q <= AZ_MAX_QUIET; ++q) {
        if (q > quiet) break;
        if (az_square(mpage, H, W, nw, f, 4 * (h + q), 4, lane)) dirty = true;
    }
    if (dirty) return;
    // lane y samples module row y
    u64 row = 0;
    if (lane < n)
        for (int x = 0; x < AZ_MAX_SIDE; ++x) {
            if (x >= n) break;
            int tx, ty;
            az_turn(x - h, lane - h, rot, tx, ty);
            row |= (u64)az_at(mpage, H, W, nw, f, 4 * tx, 4 * ty) << x;
        }
    __syncthreads();
    s.rows[lane] = row;
    rs_load_tables(s.rs, AZ_EXP + AZ_EXP_OFF[(width - 4) >> 1], AZ_LOG + AZ_LOG_OFF[(width - 4) >> 1], width, lane);
    // codewords through the layer spiral, the pad bits first
#pragma unroll 1
    for (int j = lane; j < AZ_MAX_WORDS; j += 64) {
        int val = 0;
        if (j < total)
            for (int b = 0; b < AZ_MAX_M; ++b) {
                if (b >= width) break;
                int x, y;
                az_bit_pos<AZ_MAX_LAYERS, 63>(compact, layers, pad + j * width + b, x, y);
                val = (val << 1) | (int)((s.rows[y] >> x) & 1ull);
            }
        s.rs.blk[j] = (unsigned short)val;
    }
    __syncthreads();
    const int errors = rs_correct_block(s.rs, total, ec, 1, lane);
    if (errors < 0) return;
    unsigned short* od = resdata + ((size_t)pg * max_finders + a) * data_stride;
    for (int p = lane; p < AZ_MAX_DATA; p += 64)
        if (p < ndata) od[p] = s.rs.blk[p];
    if (lane == 0) {
        // the hull: the box of the outline's four corners
        i64 x0 = 0, x1 = 0, y0 = 0, y1 = 0;
        const int e = 4 * h + 2;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            i64 qx, qy;
            az_pixel(f, (c & 1) ? e : -e, (c & 2) ? e : -e, qx, qy);
            x0 = c == 0 || qx < x0 ? qx : x0; x1 = c == 0 || qx > x1 ? qx : x1;
            y0 = c == 0 || qy < y0 ? qy : y0; y1 = c == 0 || qy > y1 ? qy : y1;
        }
        const auto cl = [](i64 v, int hi) { return (int)(v < 0 ? 0 : v > hi ? hi : v); };
        int* o = res + ((size_t)pg * max_finders + a) * CODE_RES_INTS;
        o[0] = cl(y0, H - 1); o[1] = cl(x0, W - 1); o[2] = cl(y1 - 1, H - 1); o[3] = cl(x1 - 1, W - 1); o[4] = root;
        o[5] = layers; o[6] = compact ? 1 : 0; o[7] = width; o[8] = ndata; o[9] = errors; o[10] = rot; o[11] = merr; o[12] = mism + ref; o[CODE_RES_STATE] = CODE_ROW;
    }
}

// ---- stage 2 of lumina_ocr_aztec_layers: full-range symbols of 12 .. 32 layers (definition: tests/aztec_layers_reference.py) ----
// a finer frame: slope t / 1024, pitch (1024 + k) / 1024 of the ring's, neither in the other's way; a point (u, v) in quarter modules
struct AzFrame2 { i64 cx, cy, q; int t; };

__device__ __forceinline__ AzFrame2 az_frame2(int cx2, int cy2, int s10, int t, int k) {
    AzFrame2 f;
    f.cx = (i64)cx2 << 32; f.cy = (i64)cy2 << 32; f.t = t;
    f.q = (((i64)s10 << 20) / 5120) * (1024 + k);
    return f;
}
__device__ __forceinline__ void az_pixel2(const AzFrame2& f, int u, int v, i64 half, i64& px, i64& py) {
    px = (f.cx + f.q * (i64)(1024 * u - f.t * v) + half) >> 33;
    py = (f.cy + f.q * (i64)(f.t * u + 1024 * v) + half) >> 33;
}
// the ink at a point; off the page reads clear (no branch round the load, so that the loads of neighbouring points overlap)
__device__ __forceinline__ int az_at2(const u64* mpage, int H, int W, int nw, const AzFrame2& f, int u, int v) {
    i64 px, py;
    az_pixel2(f, u, v, 0, px, py);
    const bool on = px >= 0 && py >= 0 && px < W && py < H;
    const int cx = (int)(px < 0 ? 0 : px > W - 1 ? W - 1 : px), cy = (int)(py < 0 ? 0 : py > H - 1 ? H - 1 : py);
    const int bit = (int)((mpage[(size_t)cy * nw + (size_t)(cx >> 6)] >> (cx & 63)) & 1ull);
    return on ? bit : 0;
}
// az_square for the finer frame (d / step * 2 + 1 <= 320 points a side)
__device__ __forceinline__ int az_square2(const u64* mpage, int H, int W, int nw, const AzFrame2& f, int d, int step, int lane) {
    int n = 0;
    const int cnt = 2 * d / step + 1;
#pragma unroll 1
    for (int j = 0; j < 5; ++j) {
        const int idx = lane + 64 * j, a = -d + step * idx;
        const bool on = idx < cnt;
        n += __popcll(__ballot(on && az_at2(mpage, H, W, nw, f, a, -d))) + __popcll(__ballot(on && az_at2(mpage, H, W, nw, f, a, d))) +
             __popcll(__ballot(on && az_at2(mpage, H, W, nw, f, -d, a))) + __popcll(__ballot(on && az_at2(mpage, H, W, nw, f, d, a)));
    }
    return n;
}
// mismatches of the centre row's and column's modules at the distances 8 .. hi on the four arms, each at the offsets (+-off, +-off)
// quarter modules along and across its line (off = 0: the module's centre alone); 16 (hi - 7) <= 1088 points
__device__ __forceinline__ int az_arms2(const u64* mpage, int H, int W, int nw, const AzFrame2& f, int hi, int off, int lane) {
    const int cnt = hi - 7, total = (off ? 16 : 4) * cnt;
    int n = 0;
#pragma unroll 1
    for (int j0 = 0; j0 < 20; j0 += 4) {
        if (j0 * 64 >= total) break;   // (wave-uniform)
        bool bad[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int idx = lane + 64 * (j0 + q);
            const int d = 8 + idx % cnt, r = (idx / cnt) & 15, arm = r & 3;
            const int al = 4 * d + ((r & 8) ? off : -off), ac = (r & 4) ? off : -off;
            const int sx = arm == 0 ? 1 : arm == 1 ? -1 : 0, sy = arm == 2 ? 1 : arm == 3 ? -1 : 0;
            bad[q] = idx < total && az_at2(mpage, H, W, nw, f, sx * al - sy * ac, sy * al + sx * ac) != ((d & 1) ^ 1);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) n += __popcll(__ballot(bad[q]));
    }
    return n;
}

struct AzLds2 {
    u64 rows[192][3];          // module row y: bit x of the 151
    int score[AZL_FRAMES];
    RsLds<unsigned short, AZL_MAX_WORDS, AZL_MAX_EC, AZL_MAX_M> rs;
};

// 5b: one wave per (page, finder); a finder that stage 1 did not leave pending ends at once
__global__ __launch_bounds__(64) void az_layers_kernel(const u64* mask, const int* finders, const int* nfind, const int4* box, int H, int W, int nw,
                                                       size_t runcap, int max_finders, int quiet, int max_layers, int* res, unsigned short* resdata) {
    __shared__ AzLds2 s;
    const int pg = blockIdx.y, a = blockIdx.x, lane = threadIdx.x;
    const int nf_page = nfind[pg];
    if (nf_page > max_finders || a >= nf_page || a >= AZ_MAX_FINDERS) return;
    int* o = res + ((size_t)pg * max_finders + a) * CODE_RES_INTS;
    if (o[CODE_RES_STATE] != CODE_PENDING) return;
    const int layers = clampi(o[5], AZ_MAX_LAYERS + 1, AZL_MAX_LAYERS), ndata = o[8], rot = o[10] & 3, merr = o[11], mism = o[12];
    const int t0 = clampi(o[14], -4, 4), k0 = clampi(o[15], -12, 12);
    __syncthreads();   // (every lane has read the row that lane 0 will write)
    if (layers > max_layers) return;
    const u64* mpage = mask + (size_t)pg * H * nw;
    const int root = clampi(finders[((size_t)pg * max_finders + a) * 2 + 0], 0, (int)runcap - 1);
    const int ring = clampi(finders[((size_t)pg * max_finders + a) * 2 + 1], 0, (int)runcap - 1);
    const int4 gx = box[(size_t)pg * runcap + ring];   // x0, x1, y0, y1
    const int cx2 = gx.x + gx.y + 1, cy2 = gx.z + gx.w + 1, s10 = (gx.y - gx.x + 1) + (gx.w - gx.z + 1);
    const int n = az_modules(false, layers), h = n / 2, width = az_width(layers);
    const int total = az_total_bits(false, layers) / width, pad = az_total_bits(false, layers) % width, ec = total - ndata;
    if (n > AZL_MAX_SIDE || total > AZL_MAX_WORDS || total > (1 << width) - 1 || ndata < 1 || ndata > AZ_MAX_DATA_ALL || ec < 2 || ec > AZL_MAX_EC) return;
    // the frame, coarse to fine along the centre reference lines: at every radius the middle of the frames that fit best
    int t = 8 * t0, k = 8 * (k0 - iabs(t0));
#pragma unroll 1
    for (int level = 0; level < 4; ++level) {
        const int radius = level == 3 ? h : (16 << level) < h ? (16 << level) : h, step = 8 >> level;
#pragma unroll 1
        for (int fi = 0; fi < AZL_FRAMES; ++fi) {
            const int j = fi / 9 - AZL_SPAN, i = fi % 9 - AZL_SPAN;
            const int m = az_arms2(mpage, H, W, nw, az_frame2(cx2, cy2, s10, t + step * i, k + step * j), radius, 1, lane);
            if (lane == 0) s.score[fi] = m;
        }
        __syncthreads();
        int mn = 1 << 30, jlo = 9, jhi = -9, ilo = 9, ihi = -9;
        for (int fi = 0; fi < AZL_FRAMES; ++fi) mn = s.score[fi] < mn ? s.score[fi] : mn;
        for (int fi = 0; fi < AZL_FRAMES; ++fi)
            if (s.score[fi] == mn) {
                const int j = fi / 9 - AZL_SPAN, i = fi % 9 - AZL_SPAN;
                jlo = j < jlo ? j : jlo; jhi = j > jhi ? j : jhi; ilo = i < ilo ? i : ilo; ihi = i > ihi ? i : ihi;
            }
        const int jc = (jlo + jhi) >> 1, ic = (ilo + ihi) >> 1;
        int pick = 1 << 30;
        for (int fi = 0; fi < AZL_FRAMES; ++fi)
            if (s.score[fi] == mn) {
                const int j = fi / 9 - AZL_SPAN, i = fi % 9 - AZL_SPAN;
                const int key = (iabs(j - jc) << 12) | (iabs(i - ic) << 8) | ((j + AZL_SPAN) << 4) | (i + AZL_SPAN);
                pick = key < pick ? key : pick;
            }
        __syncthreads();
        t += step * ((pick & 15) - AZL_SPAN);
        k += step * (((pick >> 4) & 15) - AZL_SPAN);
    }
    // the outline: nothing just outside it, something just inside it; of those the centre lines' fit, then the nearest
    int best = -1;
#pragma unroll 1
    for (int fi = 0; fi < AZL_FRAMES; ++fi) {
        const int j = fi / 9 - AZL_SPAN, i = fi % 9 - AZL_SPAN;
        const AzFrame2 f = az_frame2(cx2, cy2, s10, t + i, k + j);
        if (az_square2(mpage, H, W, nw, f, 4 * h + 3, 2, lane)) continue;
        if (!az_square2(mpage, H, W, nw, f, 4 * h + 1, 2, lane)) continue;
        const int ref = az_arms2(mpage, H, W, nw, f, h, 0, lane);
        const int key = (ref << 16) | (iabs(j) << 12) | (iabs(i) << 8) | ((j + AZL_SPAN) << 4) | (i + AZL_SPAN);
        if (best < 0 || key < best) best = key;
    }
    if (best < 0) return;
    const int ref = best >> 16;
    const AzFrame2 f = az_frame2(cx2, cy2, s10, t + (best & 15) - AZL_SPAN, k + ((best >> 4) & 15) - AZL_SPAN);
    bool dirty = false;
    for (int q = 1; q <= AZ_MAX_QUIET; ++q) {
        if (q > quiet) break;
        if (az_square2(mpage, H, W, nw, f, 4 * (h + q), 4, lane)) dirty = true;
    }
    if (dirty) return;
    // lane r samples module rows r, r + 64, r + 128, three words each
#pragma unroll 1
    for (int c = 0; c < 3; ++c) {
        const int y = lane + 64 * c;
        u64 w0 = 0, w1 = 0, w2 = 0;
        if (y < n)
#pragma unroll 4
            for (int x = 0; x < AZL_MAX_SIDE + 1; ++x) {
                int tx, ty;
                az_turn(x - h, y - h, rot, tx, ty);
                const u64 bit = (u64)(x < n && az_at2(mpage, H, W, nw, f, 4 * tx, 4 * ty)) << (x & 63);
                if (x < 64) w0 |= bit; else if (x < 128) w1 |= bit; else w2 |= bit;
            }
        s.rows[y][0] = w0; s.rows[y][1] = w1; s.rows[y][2] = w2;
    }
    if (width == 12) rs_load_tables(s.rs, AZ12_EXP, AZ12_LOG, 12, lane);
    else rs_load_tables(s.rs, AZ_EXP + AZ_EXP_OFF[3], AZ_LOG + AZ_LOG_OFF[3], 10, lane);
    // codewords through the layer spiral, the pad bits first
#pragma unroll 1
    for (int j = lane; j < AZL_MAX_WORDS; j += 64) {
        int val = 0;
        if (j < total)
            for (int b = 0; b < AZL_MAX_M; ++b) {
                if (b >= width) break;
                int x, y;
                az_bit_pos<AZL_MAX_LAYERS, AZL_MAX_SIDE - 1>(false, layers, pad + j * width + b, x, y);
                val = (val << 1) | (int)((s.rows[y][x >> 6] >> (x & 63)) & 1ull);
            }
        s.rs.blk[j] = (unsigned short)val;
    }
    __syncthreads();
    const int errors = rs_correct_block(s.rs, total, ec, 1, lane);
    if (errors < 0) return;
    unsigned short* od = resdata + ((size_t)pg * max_finders + a) * AZ_MAX_DATA_ALL;
    for (int p = lane; p < AZ_MAX_DATA_ALL; p += 64)
        if (p < ndata) od[p] = s.rs.blk[p];
    if (lane == 0) {
        // the hull: the box of the outline's four corners, each at its nearest pixel
        i64 x0 = 0, x1 = 0, y0 = 0, y1 = 0;
        const int e = 4 * h + 2;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            i64 qx, qy;
            az_pixel2(f, (c & 1) ? e : -e, (c & 2) ? e : -e, 1ll << 32, qx, qy);
            x0 = c == 0 || qx < x0 ? qx : x0; x1 = c == 0 || qx > x1 ? qx : x1;
            y0 = c == 0 || qy < y0 ? qy : y0; y1 = c == 0 || qy > y1 ? qy : y1;
        }
        const auto cl = [](i64 v, int hi) { return (int)(v < 0 ? 0 : v > hi ? hi : v); };
        o[0] = cl(y0, H - 1); o[1] = cl(x0, W - 1); o[2] = cl(y1 - 1, H - 1); o[3] = cl(x1 - 1, W - 1); o[4] = root;
        o[5] = layers; o[6] = 0; o[7] = width; o[8] = ndata; o[9] = errors; o[10] = rot; o[11] = merr; o[12] = mism + ref; o[CODE_RES_STATE] = CODE_ROW;
    }
}

// 6: tmp [B][max_codes][6] = y0, x0, y1, x1, root, slot; data rows of ND words (int of AZ_MAX_DATA, 16-bit of AZ_MAX_DATA_ALL)
template <class T, int ND>
__global__ __launch_bounds__(256) void az_output_kernel(const int* res_all, const unsigned short* resdata_all, const int* nfind, int max_finders, int max_codes,
                                                        int* tmp_all, int* counts, int* codes, T* data, int* finder_counts) {
    __shared__ CodeOutLds<AZ_MAX_CODES> s;
    const int pg = blockIdx.x;
    const int* res = res_all + (size_t)pg * max_finders * CODE_RES_INTS;
    const int n = code_output_rows(s, res, nfind[pg], max_finders, max_codes, tmp_all + (size_t)pg * max_codes * 6, codes + (size_t)pg * max_codes * 12,
                                   counts + pg, finder_counts ? finder_counts + pg : nullptr);
    if (n > max_codes) return;
    const unsigned short* rd = resdata_all + (size_t)pg * max_finders * ND;
    code_output_data(s, n, max_finders, ND, data + (size_t)pg * max_codes * ND,
                     [=](int slot, int j) -> T { return j < res[slot * CODE_RES_INTS + 8] ? (T)rd[(size_t)slot * ND + j] : (T)0; });
}

}  // namespace

// the workspace's regions: one layout sizes it (aztec_workspace_bytes) and carves it (aztec_launch)
struct AzWorkspace {
    Components c;
    int* nfind; int* finders; int* res; unsigned short* resdata; int* tmp;
};
static AzWorkspace aztec_layout(Arena& a, int B, int H, int W, int max_finders, int max_codes, int data_stride = AZ_MAX_DATA) {
    AzWorkspace w;
    w.c = components_layout(a, B, H, W, true);
    w.nfind = a.take<int>((size_t)B);
    w.finders = a.take<int>((size_t)B * max_finders * 2);
    w.res = a.take<int>((size_t)B * max_finders * CODE_RES_INTS);
    w.resdata = a.take<unsigned short>((size_t)B * max_finders * data_stride);
    w.tmp = a.take<int>((size_t)B * max_codes * 6);
    return w;
}

static bool aztec_args_ok(int B, int H, int W, int max_finders, int max_codes) {
    return page_args_ok(B, H, W) && max_codes >= 1 && max_codes <= AZ_MAX_CODES && max_finders >= 1 && max_finders <= AZ_MAX_FINDERS;
}

bool aztec_params_ok(int min_module, int max_module, int quiet, int centre_tol, int ring_tol, int mark_max, int max_finders, int max_codes) {
    return min_module >= 1 && max_module >= min_module && max_module <= AZ_MAX_MODULE && quiet >= 0 && quiet <= AZ_MAX_QUIET && centre_tol >= 0 &&
           centre_tol <= 64 && ring_tol >= 0 && ring_tol <= AZ_MAX_TOL && mark_max >= 0 && mark_max <= AZ_MAX_MARKS && max_finders >= 1 &&
           max_finders <= AZ_MAX_FINDERS && max_codes >= 1 && max_codes <= AZ_MAX_CODES;
}

size_t aztec_workspace_bytes(int B, int H, int W, int max_finders, int max_codes) {
    if (!aztec_args_ok(B, H, W, max_finders, max_codes)) return 0;
    Arena a;
    aztec_layout(a, B, H, W, max_finders, max_codes);
    return a.off;
}

bool aztec_max_layers_ok(int max_layers) { return max_layers >= AZ_MAX_LAYERS && max_layers <= AZL_MAX_LAYERS; }

size_t aztec_layers_workspace_bytes(int B, int H, int W, int max_finders, int max_codes) {
    if (!aztec_args_ok(B, H, W, max_finders, max_codes)) return 0;
    Arena a;
    aztec_layout(a, B, H, W, max_finders, max_codes, AZ_MAX_DATA_ALL);
    return a.off;
}

// both entries: data_all = nullptr is lumina_ocr_aztec (p.data, stage 1 alone), otherwise lumina_ocr_aztec_layers (16-bit rows of AZ_MAX_DATA_ALL)
static hipError_t aztec_run(const AztecParams& p, int max_layers, unsigned short* data_all, void* workspace, size_t ws_bytes, hipStream_t st) {
    const int B = p.B, H = p.H, W = p.W;
    if (!aztec_args_ok(B, H, W, p.max_finders, p.max_codes) ||
        !aztec_params_ok(p.min_module, p.max_module, p.quiet, p.centre_tol, p.ring_tol, p.mark_max, p.max_finders, p.max_codes) ||
        !aztec_max_layers_ok(max_layers))
        return hipErrorInvalidValue;
    if (!p.rgb || !p.codes || !(data_all ? (const void*)data_all : (const void*)p.data) || !p.counts) return hipErrorInvalidValue;
    const int stride = data_all ? AZ_MAX_DATA_ALL : AZ_MAX_DATA;
    Arena a(workspace, ws_bytes);
    AzWorkspace w = aztec_layout(a, B, H, W, p.max_finders, p.max_codes, stride);
    if (a.overflow) return hipErrorOutOfMemory;
    const int nw = (W + 63) / 64;
    const size_t runcap = run_cap(H, W);
    hipError_t e;
    if ((e = hipMemsetAsync(w.nfind, 0, sizeof(int) * (size_t)B, st)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(w.res, 0, sizeof(int) * (size_t)B * p.max_finders * CODE_RES_INTS, st)) != hipSuccess) return e;
    if ((e = components_launch(w.c, p.rgb, p.mask_in, p.mask_out, B, H, W, p.threshold, st)) != hipSuccess) return e;
    const unsigned long long* mask = w.c.mask;
    const int rows = B * H;
    hipLaunchKernelGGL(az_finders_kernel, row_wave_grid(rows), dim3(256), 0, st, w.c.runoff, w.c.rxs, w.c.rxe, w.c.parent, w.c.box, w.c.area, H, runcap,
                       p.min_module, p.max_module, p.centre_tol, p.ring_tol, p.max_finders, w.nfind, w.finders, rows);
    hipLaunchKernelGGL(az_decode_kernel, dim3(p.max_finders, B), dim3(64), 0, st, mask, w.finders, w.nfind, w.c.box, H, W, nw, runcap, p.max_finders, p.quiet,
                       p.mark_max, max_layers, stride, w.res, w.resdata);
    if (!data_all) {
        hipLaunchKernelGGL((az_output_kernel<int, AZ_MAX_DATA>), dim3(B), dim3(256), 0, st, w.res, w.resdata, w.nfind, p.max_finders, p.max_codes, w.tmp, p.counts,
                           p.codes, p.data, p.finder_counts);
        return hipGetLastError();
    }
    if (max_layers > AZ_MAX_LAYERS)
        hipLaunchKernelGGL(az_layers_kernel, dim3(p.max_finders, B), dim3(64), 0, st, mask, w.finders, w.nfind, w.c.box, H, W, nw, runcap, p.max_finders, p.quiet,
                           max_layers, w.res, w.resdata);
    hipLaunchKernelGGL((az_output_kernel<unsigned short, AZ_MAX_DATA_ALL>), dim3(B), dim3(256), 0, st, w.res, w.resdata, w.nfind, p.max_finders, p.max_codes, w.tmp,
                       p.counts, p.codes, data_all, p.finder_counts);
    return hipGetLastError();
}

hipError_t aztec_launch(const AztecParams& p, void* workspace, size_t ws_bytes, hipStream_t st) {
    return aztec_run(p, AZ_MAX_LAYERS, nullptr, workspace, ws_bytes, st);
}

hipError_t aztec_layers_launch(const AztecLayersParams& p, void* workspace, size_t ws_bytes, hipStream_t st) {
    if (!p.data_all) return hipErrorInvalidValue;
    return aztec_run(p, p.max_layers, p.data_all, workspace, ws_bytes, st);
}
