// Selection marks (checkboxes) on the GPU (gfx950): the square frames of a page with the state of their interior, as
// (x0, y0, x1, y1, edge, ink_in, area_in, state) in a canonical order.  Everything is integer and every reduction is order-free
// (min / max / add / or), so the lists equal the sequential definition restated in tests/mark_reference.py.
//
// A box side (14-60 pixels at 200 dpi) is shorter than any rule, so the fixed run slots of tables.hip do not apply: marks need the
// connected components of ALL ink.  A row of a page is a list of runs (a text page: ~100 per row), in raster order, and everything
// up to the candidates works on that list, as dbpost.hip does for the probability map: steps 1-4 are components_launch of runs.h.
//
// All stream-ordered kernels, no host round trip; kernels 2-5 are one wave per (page, row), four rows per work-group:
//   1 ink_mask    ink = L < threshold packed into 64-bit words along x — or the mask the caller already has
//   2 run_count / row_scan / run_fill   mask words -> run list [xs, xe] of the page in raster order; a run is its own parent and box
//   3 run_merge   union-find (atomicMin) over run ids: a run joins the runs of the row above it touches (8-connectivity); the root
//                 of a component is its first run in raster order
//   4 run_accum   every run learns its root; bounding box of every component accumulated at the root (atomicMin / atomicMax,
//                 issued only when the value read would change)
//   5 mk_marks    roots whose box is a candidate (sides in range, nearly square): the row's WAVE takes each one — lane r owns row
//                 y0 + r and builds its 64-bit window from the one or two mask words the box straddles; the frame counts and the
//                 interior ink are wave-wide OR / popcount / add reductions (no LDS, no per-pixel loop) -> counted, gathered
//   6 mk_sort     one work-group per page: rank sort by (y0, x0, y1, x1, root) -> the output
// Round marks (radio buttons; only when MarkParams.rounds is given, definition restated in tests/radio_reference.py):
//   5b mk_rounds  the same roots and candidates, after mk_marks: a candidate that is no frame is read in doubled coordinates about its
//                 box centre.  Lane r owns row y0 + r: the outside / ring / moat / core zones of its row are bit intervals whose ends
//                 come from an integer root of bound - v^2; roundness, the ring's coverage, the empty moat and the core's ink are
//                 wave-wide reductions; the isolation band is a second short pass in which lanes own the band's rows -> counted,
//                 gathered into a list of its own, sorted by mk_sort
#include "marks.h"
#include "runs.h"

namespace {

typedef unsigned long long u64;

__device__ __forceinline__ u64 wave_or(u64 v) {
    unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { lo |= (unsigned)__shfl_xor((int)lo, d); hi |= (unsigned)__shfl_xor((int)hi, d); }
    return ((u64)hi << 32) | lo;
}

// 5: tmp [B][max_marks][9] = y0, x0, y1, x1, root, edge, ink_in, area_in, state
__global__ __launch_bounds__(256) void mk_marks_kernel(const u64* mask, const int* runoff, const int* parent, const int4* box, int H, int nw, size_t runcap,
                                                       int min_side, int max_side, int max_marks, int* counts, int* tmp, int rows_total) {
    int pg, row, lane;
    if (!row_wave(H, rows_total, pg, row, lane)) return;
    const int* ro = runoff + (size_t)pg * (H + 1);
    const int r0 = ro[row], r1 = ro[row + 1];
    const size_t rb = (size_t)pg * runcap;
    const u64* mpage = mask + (size_t)pg * H * nw;
    for (int i0 = r0; i0 < r1; i0 += 64) {   // (wave-uniform bounds: the ballot sees every lane)
        const int id = i0 + lane;
        int4 bx = make_int4(0, 0, 0, 0);
        bool cand = false;
        if (id < r1 && parent[rb + id] == id) {
            bx = box[rb + id];
            const int w = bx.y - bx.x + 1, h = bx.w - bx.z + 1, d = w > h ? w - h : h - w, mn = w < h ? w : h;
            cand = w >= min_side && h >= min_side && w <= max_side && h <= max_side && 4 * d <= mn;
        }
        u64 todo = __ballot(cand);
        while (todo) {   // wave-uniform: every lane works on the candidate of lane `src`
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int x0 = __shfl(bx.x, src), x1 = __shfl(bx.y, src), y0 = __shfl(bx.z, src), y1 = __shfl(bx.w, src);
            const int w = x1 - x0 + 1, h = y1 - y0 + 1, t = 1 + (w < h ? w : h) / 8;
            // lane r: bits x0 .. x1 of row y0 + r (y0 + r <= y1 < H; the second word only when the box reaches into it)
            u64 win = 0;
            if (lane < h) {
                const u64* mr = mpage + (size_t)(y0 + lane) * nw;
                const int wi = x0 >> 6, s = x0 & 63;
                win = mr[wi] >> s;
                if (s && s + w > 64) win |= mr[wi + 1] << (64 - s);
                if (w < 64) win &= (1ull << w) - 1ull;
            }
            const int top = __popcll(wave_or(lane < t ? win : 0ull));
            const int bottom = __popcll(wave_or(lane >= h - t ? win : 0ull));   // (lanes >= h hold 0)
            const int left = __popcll(__ballot((win & ((1ull << t) - 1ull)) != 0ull));
            const int right = __popcll(__ballot((win >> (w - t)) != 0ull));
            const int qx = w / 4, qy = h / 4;
            const u64 cols = (w - 2 * qx < 64 ? (1ull << (w - 2 * qx)) - 1ull : ~0ull) << qx;
            const int ink_in = wave_sum(lane >= qy && lane < h - qy ? __popcll(win & cols) : 0);
            if (top >= w - w / 8 && bottom >= w - w / 8 && left >= h - h / 8 && right >= h - h / 8 && lane == 0) {
                const int area_in = (w - 2 * qx) * (h - 2 * qy);
                const int idx = atomicAdd(&counts[pg], 1);
                if (idx < max_marks) {
                    int* o = tmp + ((size_t)pg * max_marks + idx) * 9;
                    o[0] = y0; o[1] = x0; o[2] = y1; o[3] = x1; o[4] = i0 + src;
                    o[5] = top + bottom + left + right; o[6] = ink_in; o[7] = area_in; o[8] = 16 * ink_in >= area_in ? 1 : 0;
                }
            }
        }
    }
}

// up to 64 bits of row y of a page's mask from any x: bit k = ink at (x + k, y), k < n (1 <= n <= 64); rows and columns off the page
// are clear.  Every shift count is 0..63.
__device__ __forceinline__ u64 mask_bits(const u64* mpage, int H, int W, int nw, int y, int x, int n) {
    if (y < 0 || y >= H) return 0ull;
    const int xa = x > 0 ? x : 0, xb = x + n - 1 < W - 1 ? x + n - 1 : W - 1;
    if (xa > xb) return 0ull;
    const int cnt = xb - xa + 1;   // 1..64
    const u64* mr = mpage + (size_t)y * nw;
    const int wi = xa >> 6, s = xa & 63;
    u64 v = mr[wi] >> s;
    if (s && s + cnt > 64) v |= mr[wi + 1] << (64 - s);   // (xb >= 64 (wi + 1): the word is the row's)
    if (cnt < 64) v &= (1ull << cnt) - 1ull;
    return v << (xa - x);   // (xa - x + cnt <= n <= 64)
}

// bits lo .. hi of a word (0 <= lo, hi <= 63; empty when lo > hi)
__device__ __forceinline__ u64 bit_span(int lo, int hi) {
    if (lo > hi) return 0ull;
    const int n = hi - lo + 1;
    return (n < 64 ? (1ull << n) - 1ull : ~0ull) << lo;
}

// columns c of a w-wide box row with u^2 <= t, u = 2 c - (w - 1): |u| <= m, m the integer root of t (t < 2^15); none when t < 0
__device__ __forceinline__ u64 disc_cols(int t, int w) {
    if (t < 0) return 0ull;
    int m = 0;
#pragma unroll
    for (int b = 128; b >= 1; b >>= 1)
        if ((m + b) * (m + b) <= t) m += b;
    int lo = w - 1 - m, hi = (w - 1 + m) >> 1;
    lo = lo > 0 ? (lo + 1) >> 1 : 0;
    if (hi > w - 1) hi = w - 1;
    return bit_span(lo, hi);
}

// 5b: tmp as in 5.  A frame of 5 is never a round mark.
__global__ __launch_bounds__(256) void mk_rounds_kernel(const u64* mask, const int* runoff, const int* parent, const int4* box, int H, int W, int nw,
                                                        size_t runcap, int min_side, int max_side, int out_max, int ring_div, int band_div, int band_min,
                                                        int max_marks, int* counts, int* tmp, int rows_total) {
    int pg, row, lane;
    if (!row_wave(H, rows_total, pg, row, lane)) return;
    const int* ro = runoff + (size_t)pg * (H + 1);
    const int r0 = ro[row], r1 = ro[row + 1];
    const size_t rb = (size_t)pg * runcap;
    const u64* mpage = mask + (size_t)pg * H * nw;
    for (int i0 = r0; i0 < r1; i0 += 64) {
        const int id = i0 + lane;
        int4 bx = make_int4(0, 0, 0, 0);
        bool cand = false;
        if (id < r1 && parent[rb + id] == id) {
            bx = box[rb + id];
            const int w = bx.y - bx.x + 1, h = bx.w - bx.z + 1, d = w > h ? w - h : h - w, mn = w < h ? w : h;
            cand = w >= min_side && h >= min_side && w <= max_side && h <= max_side && 4 * d <= mn;
        }
        u64 todo = __ballot(cand);
        while (todo) {
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int x0 = __shfl(bx.x, src), x1 = __shfl(bx.y, src), y0 = __shfl(bx.z, src), y1 = __shfl(bx.w, src);
            const int w = x1 - x0 + 1, h = y1 - y0 + 1, mn = w < h ? w : h, D = w > h ? w : h;
            const u64 win = lane < h ? mask_bits(mpage, H, W, nw, y0 + lane, x0, w) : 0ull;
            // the checkboxes' frame test
            const int t = 1 + mn / 8;
            const int ftop = __popcll(wave_or(lane < t ? win : 0ull)), fbottom = __popcll(wave_or(lane >= h - t ? win : 0ull));
            const int fleft = __popcll(__ballot((win & ((1ull << t) - 1ull)) != 0ull)), fright = __popcll(__ballot((win >> (w - t)) != 0ull));
            const bool frame = ftop >= w - w / 8 && fbottom >= w - w / 8 && fleft >= h - h / 8 && fright >= h - h / 8;
            // zones of this lane's row
            const int T = 1 + D / ring_div, di = D - 2 * T > 0 ? D - 2 * T : 0;
            const int b_outer = (D + 1) * (D + 1), b_core = D * D / 4, b_inner = di * di > b_core ? di * di : b_core;
            const int v = 2 * lane - (h - 1), vv = v * v;
            const bool own = lane < h;
            const u64 full = bit_span(0, w - 1);
            const u64 d_outer = own ? disc_cols(b_outer - vv, w) : 0ull, d_inner = own ? disc_cols(b_inner - vv, w) : 0ull;
            const u64 d_core = own ? disc_cols(b_core - vv, w) : 0ull;
            const int outside = wave_sum(__popcll(win & full & ~d_outer));
            const u64 ring = win & d_outer & ~d_inner;
            const int top = __popcll(wave_or(v <= 0 ? ring : 0ull)), bottom = __popcll(wave_or(v >= 0 ? ring : 0ull));   // (lanes >= h hold 0)
            const int left = __popcll(__ballot((ring & bit_span(0, (w - 1) >> 1)) != 0ull));
            const int right = __popcll(__ballot((ring & bit_span(w >> 1, w - 1)) != 0ull));
            const bool moat = __ballot((win & d_inner & ~d_core) != 0ull) != 0ull;
            const int ink_in = wave_sum(__popcll(win & d_core)), area_in = wave_sum(__popcll(d_core));
            // isolation: the band's columns beside the box's rows, then the band's rows over the whole width (up to 64 + 2 * 16 columns)
            const int band = band_min + mn / band_div;   // <= 32 (marks_launch checks the parameters)
            u64 near = 0ull;
            if (own && band > 0) near = mask_bits(mpage, H, W, nw, y0 + lane, x0 - band, band) | mask_bits(mpage, H, W, nw, y0 + lane, x1 + 1, band);
            if (lane < 2 * band) {
                const int y = lane < band ? y0 - band + lane : y1 + 1 + (lane - band);
                const int span = w + 2 * band;   // 1..128
                near |= mask_bits(mpage, H, W, nw, y, x0 - band, span < 64 ? span : 64);
                if (span > 64) near |= mask_bits(mpage, H, W, nw, y, x0 - band + 64, span - 64);
            }
            const bool crowded = __ballot(near != 0ull) != 0ull;
            const bool covered = top >= w - w / 8 && bottom >= w - w / 8 && left >= h - h / 8 && right >= h - h / 8;
            if (!frame && outside <= out_max && covered && !moat && !crowded && lane == 0) {
                const int idx = atomicAdd(&counts[pg], 1);
                if (idx < max_marks) {
                    int* o = tmp + ((size_t)pg * max_marks + idx) * 9;
                    o[0] = y0; o[1] = x0; o[2] = y1; o[3] = x1; o[4] = i0 + src;
                    o[5] = top + bottom + left + right; o[6] = ink_in; o[7] = area_in; o[8] = 16 * ink_in >= area_in ? 1 : 0;
                }
            }
        }
    }
}

// 6: the five key columns in LDS; roots are distinct, so ranks are
__global__ __launch_bounds__(256) void mk_sort_kernel(const int* counts, const int* tmp, int* marks, int max_marks) {
    __shared__ int s_key[MARK_MAX_MARKS * 5];
    const int pg = blockIdx.x;
    const int n = counts[pg];
    if (n > max_marks) return;   // overflow: the count is all that is reported
    const int* t = tmp + (size_t)pg * max_marks * 9;
    int* out = marks + (size_t)pg * max_marks * 8;
    rank_sort<5>(s_key, t, 9, n, [=](int i, int rank, const int (&k)[5]) {
        int* o = out + (size_t)rank * 8;
        o[0] = k[1]; o[1] = k[0]; o[2] = k[3]; o[3] = k[2];
        o[4] = t[i * 9 + 5]; o[5] = t[i * 9 + 6]; o[6] = t[i * 9 + 7]; o[7] = t[i * 9 + 8];
    });
}

}  // namespace

// the workspace's regions: one layout sizes it (marks_workspace_bytes) and carves it (marks_launch)
struct MarkWorkspace {
    Components c;   // (no area)
    int* tmp; int* round_tmp;   // round_tmp: only with the round list
};
static MarkWorkspace marks_layout(Arena& a, int B, int H, int W, int max_marks, bool rounds) {
    MarkWorkspace w;
    w.c = components_layout(a, B, H, W, false);
    w.tmp = a.take<int>((size_t)B * max_marks * 9);
    w.round_tmp = rounds ? a.take<int>((size_t)B * max_marks * 9) : nullptr;
    return w;
}

static bool marks_args_ok(int B, int H, int W, int max_marks) {
    return page_args_ok(B, H, W) && max_marks >= 1 && max_marks <= MARK_MAX_MARKS;
}

bool round_params_ok(int out_max, int ring_div, int band_div, int band_min) {
    return out_max >= 0 && ring_div >= 1 && band_div >= ROUND_MIN_BAND_DIV && band_min >= 0 && band_min <= ROUND_MAX_BAND_MIN;
}

size_t marks_workspace_bytes(int B, int H, int W, int max_marks, bool rounds) {
    if (!marks_args_ok(B, H, W, max_marks)) return 0;
    Arena a;
    marks_layout(a, B, H, W, max_marks, rounds);
    return a.off;
}

hipError_t marks_launch(const MarkParams& p, void* workspace, size_t ws_bytes, hipStream_t st) {
    const int B = p.B, H = p.H, W = p.W;
    if (!marks_args_ok(B, H, W, p.max_marks) || p.min_side < MARK_MIN_SIDE || p.max_side > MARK_MAX_SIDE || p.max_side < p.min_side) return hipErrorInvalidValue;
    if (!p.rgb || !p.marks || !p.counts) return hipErrorInvalidValue;
    const bool rounds = p.rounds != nullptr;
    if (rounds != (p.round_counts != nullptr)) return hipErrorInvalidValue;
    if (rounds && !round_params_ok(p.out_max, p.ring_div, p.band_div, p.band_min)) return hipErrorInvalidValue;
    Arena a(workspace, ws_bytes);
    MarkWorkspace w = marks_layout(a, B, H, W, p.max_marks, rounds);
    if (a.overflow) return hipErrorOutOfMemory;
    const int nw = (W + 63) / 64;
    const size_t runcap = run_cap(H, W);
    hipError_t e = hipMemsetAsync(p.counts, 0, sizeof(int) * (size_t)B, st);
    if (e != hipSuccess) return e;
    if ((e = components_launch(w.c, p.rgb, p.mask_in, p.mask_out, B, H, W, p.threshold, st)) != hipSuccess) return e;
    const unsigned long long* mask = w.c.mask;
    const int rows = B * H;
    const dim3 grows = row_wave_grid(rows);
    hipLaunchKernelGGL(mk_marks_kernel, grows, dim3(256), 0, st, mask, w.c.runoff, w.c.parent, w.c.box, H, nw, runcap, p.min_side, p.max_side, p.max_marks,
                       p.counts, w.tmp, rows);
    hipLaunchKernelGGL(mk_sort_kernel, dim3(B), dim3(256), 0, st, p.counts, w.tmp, p.marks, p.max_marks);
    if (rounds) {
        if ((e = hipMemsetAsync(p.round_counts, 0, sizeof(int) * (size_t)B, st)) != hipSuccess) return e;
        hipLaunchKernelGGL(mk_rounds_kernel, grows, dim3(256), 0, st, mask, w.c.runoff, w.c.parent, w.c.box, H, W, nw, runcap, p.min_side, p.max_side, p.out_max,
                           p.ring_div, p.band_div, p.band_min, p.max_marks, p.round_counts, w.round_tmp, rows);
        hipLaunchKernelGGL(mk_sort_kernel, dim3(B), dim3(256), 0, st, p.round_counts, w.round_tmp, p.rounds, p.max_marks);
    }
    return hipGetLastError();
}
