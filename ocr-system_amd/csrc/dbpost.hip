// DB post-process and recognition crop on the GPU (gfx950), bit-identical by construction to the
// sequential definition in oracle/csrc/dbpost_oracle.c (integer geometry, exact rational area
// comparison, fixed-point score sum, correctly-rounded fp64 corner arithmetic, no fma).
//
// No reference counterpart; output shape = the 4-point quad of
// /root/reference/backend/utils/ocr_postprocessor.py:24 / flat polygon of ocr_service.py:295-301.
//
// Pipeline (all stream-ordered kernels, no host round trip).  Steps 1-7 work on the RUNS of the binarised map, one wave per page row:
//   1 rl_mask / row_scan / run_fill   threshold -> 64-bit masks per row segment -> run list [xs, xe] of the page in raster order
//   2 run_merge     union-find (atomicMin) over run ids: a run joins the runs of the row above it touches (8-connectivity)
//   3 rl_roots      parent = root = the component's first run (starts at its smallest linear pixel index: canonical); roots per row
//   4 row_scan / rl_assign : roots in raster order -> component id k < max_boxes, top row
//   5 rl_extent     atomicMax of the component's bottom row, by the runs that have no run below them
//   6 seg_scan / seg_init   per page: row-extreme segments; 7 rl_extremes: per-row min/max x, reduced per component inside the wave
//                   (atomics only in rows of more than 64 runs)
//   8 live_list / comp_box   the live components (k < min(ncomp, max_boxes)) of the batch as one list, walked by a grid of what is
//                   resident; a work-group per component: hull (monotone chains), rotating calipers over hull
//                   edges (lanes = edges), fixed-point score (lanes = 8-pixel chunks of a row), unclip, corner order
//   9 compact       valid boxes in component order -> boxes / scores / count
// row_scan, run_fill and run_merge are the run-list kernels of runs.hip, shared with the selection marks.
#include "dbpost.h"
#include "runs.h"

namespace {

// ---- 1-7: connected components over RUNS.  A row of the binarised map is a short list of runs (a text page: ~10 per row, 2 %
// of what a per-pixel label image holds), in raster order; everything between the threshold and the per-component row extremes
// works on that list.  All kernels are one wave per (page, row), four rows per work-group (row_wave).

// 1a: threshold -> one 64-bit mask per 64-pixel segment of the row + the number of runs in the row; the row's probabilities are
// requested 8 segments at a time
__global__ __launch_bounds__(256) void rl_mask_kernel(const bf16_t* prob, unsigned long long* mask, int* runcnt, int Hp, int Wp, int nseg, int vh, int vw,
                                                      float thresh, int rows_total) {
    int pg, row, lane;
    if (!row_wave(Hp, rows_total, pg, row, lane)) return;
    const size_t base = ((size_t)pg * Hp + row) * Wp;
    unsigned long long* mrow = mask + ((size_t)pg * Hp + row) * nseg;
    int cnt = 0;
    unsigned long long carry = 0;   // bit 63 of the previous segment
    for (int xb = 0; xb < Wp; xb += 64 * 8) {
        float pv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int x = xb + u * 64 + lane;
            pv[u] = bf16_to_f32(prob[base + (x < Wp ? x : Wp - 1)]);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int x0 = xb + u * 64, x = x0 + lane;
            if (x0 >= Wp) break;
            const unsigned long long m = __ballot(x < vw && row < vh && pv[u] > thresh);
            if (lane == 0) mrow[x0 >> 6] = m;
            cnt += __popcll(run_starts(m, carry));
            carry = m >> 63;
        }
    }
    if (lane == 0) runcnt[(size_t)pg * (Hp + 1) + row] = cnt;
}
// 3 + 4a: every run learns its root; roots per row are counted
__global__ __launch_bounds__(256) void rl_roots_kernel(const int* runoff, int* parent, int* rootcnt, int Hp, size_t runcap, int rows_total) {
    int pg, row, lane;
    if (!row_wave(Hp, rows_total, pg, row, lane)) return;
    const int* ro = runoff + (size_t)pg * (Hp + 1);
    const int r0 = ro[row], r1 = ro[row + 1];
    int* P = parent + (size_t)pg * runcap;
    int cnt = 0;
    for (int i0 = r0; i0 < r1; i0 += 64) {   // (wave-uniform bounds: the ballot sees every lane)
        const int id = i0 + lane;
        bool root = false;
        if (id < r1) {
            const int p = P[id];
            root = p == id;
            if (!root) P[id] = uf_find(P, p);   // concurrent compressions only ever replace a parent by an ancestor
        }
        cnt += __popcll(__ballot(root));
    }
    if (lane == 0) rootcnt[(size_t)pg * (Hp + 1) + row] = cnt;
}
// 4c: roots in raster order -> component id k (or -1 beyond the cap); the root's row IS the component's top row
__global__ __launch_bounds__(256) void rl_assign_kernel(const int* runoff, const int* rootoff, const int* parent, int* cidr, int* ymin, int* ymax, int Hp,
                                                        size_t runcap, int maxc, int rows_total) {
    int pg, row, lane;
    if (!row_wave(Hp, rows_total, pg, row, lane)) return;
    const int* ro = runoff + (size_t)pg * (Hp + 1);
    const int r0 = ro[row], r1 = ro[row + 1];
    const size_t rb = (size_t)pg * runcap;
    int k0 = rootoff[(size_t)pg * (Hp + 1) + row];
    for (int i0 = r0; i0 < r1; i0 += 64) {
        const int id = i0 + lane;
        const bool root = id < r1 && parent[rb + id] == id;
        const unsigned long long m = __ballot(root);
        if (root) {
            const int k = k0 + __popcll(m & ((1ull << lane) - 1ull));
            cidr[rb + id] = k < maxc ? k : -1;
            if (k < maxc) { ymin[(size_t)pg * maxc + k] = row; ymax[(size_t)pg * maxc + k] = row; }
        }
        k0 += __popcll(m);
    }
}
// 5: bottom row of every component.  A run that touches a run of the row below (run_merge's rule, 8-connectivity) is not its
// component's lowest: only the others report their row, so a component costs one atomic per bottom end, not one per run
__global__ __launch_bounds__(256) void rl_extent_kernel(const int* runoff, const unsigned short* rxs, const unsigned short* rxe, const int* parent,
                                                        const int* cidr, int* ymax, int Hp, size_t runcap, int maxc, int rows_total) {
    int pg, row, lane;
    if (!row_wave(Hp, rows_total, pg, row, lane)) return;
    const int* ro = runoff + (size_t)pg * (Hp + 1);
    const size_t rb = (size_t)pg * runcap;
    const int r0 = ro[row], r1 = ro[row + 1];
    if (r0 == r1) return;
    const int b1 = row + 1 < Hp ? ro[row + 2] : r1;   // the row below holds runs [r1, b1)
    for (int id = r0 + lane; id < r1; id += 64) {
        if (r1 < b1) {
            const int xs = rxs[rb + id], xe = rxe[rb + id];
            int lo = r1, hi = b1;   // first run of the row below with xe' + 1 >= xs
            while (lo < hi) { const int mid = (lo + hi) >> 1; if ((int)rxe[rb + mid] + 1 < xs) lo = mid + 1; else hi = mid; }
            if (lo < b1 && (int)rxs[rb + lo] <= xe + 1) continue;
        }
        const int k = cidr[rb + parent[rb + id]];
        if (k >= 0) atomicMax(&ymax[(size_t)pg * maxc + k], row);
    }
}
// ---- 6: per page segment offsets (one wave) + init of the segments in use ----
__global__ __launch_bounds__(64) void seg_scan_kernel(const int* ncomp, const int* ymin, const int* ymax, int* segoff, int maxc) {
    const int pg = blockIdx.x, lane = threadIdx.x;
    const int n = ncomp[pg] < maxc ? ncomp[pg] : maxc;
    int run = 0;
    for (int k0 = 0; k0 < n; k0 += 64) {
        const int k = k0 + lane;
        const int v = k < n ? (ymax[(size_t)pg * maxc + k] - ymin[(size_t)pg * maxc + k] + 1) : 0;
        int inc = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(inc, d); if (lane >= d) inc += t; }
        if (k < n) segoff[(size_t)pg * (maxc + 1) + k] = run + inc - v;
        run += __shfl(inc, 63);
    }
    if (lane == 0) segoff[(size_t)pg * (maxc + 1) + n] = run;
}
__global__ __launch_bounds__(256) void seg_init_kernel(const int* ncomp, const int* segoff, int* rowmin, int* rowmax, int maxc, size_t seg_cap) {
    const int pg = blockIdx.y;
    const int n = ncomp[pg] < maxc ? ncomp[pg] : maxc;
    const int total = segoff[(size_t)pg * (maxc + 1) + n];
    for (int g = blockIdx.x * 256 + threadIdx.x; g < total; g += gridDim.x * 256) { rowmin[(size_t)pg * seg_cap + g] = 0x7fffffff; rowmax[(size_t)pg * seg_cap + g] = -1; }
}
// ---- 7: leftmost / rightmost foreground pixel of every component in every row it covers ----
__global__ __launch_bounds__(256) void rl_extremes_kernel(const int* runoff, const unsigned short* rxs, const unsigned short* rxe, const int* parent,
                                                          const int* cidr, const int* ymin, const int* segoff, int* rowmin, int* rowmax, int Hp,
                                                          size_t runcap, int maxc, size_t seg_cap, int rows_total) {
    int pg, row, lane;
    if (!row_wave(Hp, rows_total, pg, row, lane)) return;
    const int* ro = runoff + (size_t)pg * (Hp + 1);
    const size_t rb = (size_t)pg * runcap;
    const int r0 = ro[row], r1 = ro[row + 1];
    // the runs of a row are in raster order: among the (up to 64) runs the wave holds, a component's leftmost pixel is the start of
    // its first run and its rightmost the end of its last.  A row of at most 64 runs is one batch and those two lanes store; a longer
    // row may split a component over batches, and the same two lanes of every batch fall back to the atomics.
    const bool single = r1 - r0 <= 64;
    for (int i0 = r0; i0 < r1; i0 += 64) {   // (wave-uniform bounds: the ballots see every lane)
        const int id = i0 + lane;
        const int k = id < r1 ? cidr[rb + parent[rb + id]] : -1;
        bool first = false, last = false;
        unsigned long long todo = __ballot(k >= 0);
        while (todo) {
            const int kk = __shfl(k, __ffsll((long long)todo) - 1);
            const unsigned long long m = __ballot(k == kk);
            if (k == kk) { first = lane == __ffsll((long long)m) - 1; last = lane == 63 - __clzll((long long)m); }
            todo &= ~m;
        }
        if (first || last) {
            const size_t sg = (size_t)pg * seg_cap + segoff[(size_t)pg * (maxc + 1) + k] + (row - ymin[(size_t)pg * maxc + k]);
            if (single) {
                if (first) rowmin[sg] = (int)rxs[rb + id];
                if (last) rowmax[sg] = (int)rxe[rb + id];
            } else {
                if (first) atomicMin(&rowmin[sg], (int)rxs[rb + id]);
                if (last) atomicMax(&rowmax[sg], (int)rxe[rb + id]);
            }
        }
    }
}

// ---- 8: one wave per component ----
struct Cand { long long dx, dy, mind, maxd, minn, maxn, L, A; int have; };

__device__ __forceinline__ bool frac_less(unsigned long long a1, unsigned long long l2, unsigned long long a2, unsigned long long l1, bool* eq) {
    // compare a1*l2 vs a2*l1 exactly (128-bit)
    const unsigned long long h1 = __umul64hi(a1, l2), lo1 = a1 * l2, h2 = __umul64hi(a2, l1), lo2 = a2 * l1;
    *eq = (h1 == h2 && lo1 == lo2);
    return h1 < h2 || (h1 == h2 && lo1 < lo2);
}
__device__ __forceinline__ bool cand_better(const Cand& a, const Cand& b) {  // is a strictly better than b
    if (!a.have) return false;
    if (!b.have) return true;
    bool eq;
    const bool less = frac_less((unsigned long long)a.A, (unsigned long long)b.L, (unsigned long long)b.A, (unsigned long long)a.L, &eq);
    if (!eq) return less;
    return a.dx < b.dx || (a.dx == b.dx && a.dy < b.dy);
}
__device__ __forceinline__ long long gcdll(long long a, long long b) {
    a = a < 0 ? -a : a; b = b < 0 ? -b : b;
    while (b) { const long long t = a % b; a = b; b = t; }
    return a;
}
__device__ __forceinline__ long long shfl_ll(long long v, int src) {
    const int lo = __shfl((int)(v & 0xffffffffll), src), hi = __shfl((int)(v >> 32), src);
    return ((long long)hi << 32) | (unsigned int)lo;
}
__device__ __forceinline__ long long shfl_xor_ll(long long v, int m) {
    const int lo = __shfl_xor((int)(v & 0xffffffffll), m), hi = __shfl_xor((int)(v >> 32), m);
    return ((long long)hi << 32) | (unsigned int)lo;
}

constexpr int HULL_LDS = 4096;  // hull points kept in LDS (taller components fall back to the global scratch)

// one live component (page pg, id k) by the whole work-group; every path out of it sets the component's valid flag
__device__ __forceinline__ void comp_box_item(const int pg, const int k, const bf16_t* prob, const int* ymin, const int* ymax, const int* segoff,
                                              const int* rowmin, const int* rowmax, int2* hullbuf, int* box_tmp, float* score_tmp,
                                              int* valid_tmp, int Hp, int Wp, int vh, int vw, int maxc, size_t seg_cap,
                                              float box_thresh, float unclip_ratio, int min_size) {
    __shared__ int2 s_hull[HULL_LDS];
    __shared__ int s_ext[HULL_LDS];  // row minima [0, HULL_LDS/2) and maxima [HULL_LDS/2, HULL_LDS) of the component
    __shared__ Cand s_cand[4];
    __shared__ unsigned long long s_sum[4], s_cnt[4];
    __shared__ int s_nl, s_nr, s_nh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int* vflag = valid_tmp + (size_t)pg * maxc + k;
    const int y0 = ymin[(size_t)pg * maxc + k], y1 = ymax[(size_t)pg * maxc + k];
    const size_t seg = (size_t)pg * seg_cap + segoff[(size_t)pg * (maxc + 1) + k];
    const int* rmin = rowmin + seg;
    const int* rmax = rowmax + seg;
    const int rows = y1 - y0 + 1;
    int2* hull = (2 * rows <= HULL_LDS) ? s_hull : hullbuf + 2 * seg;
    // the per-row extremes are fetched by the whole workgroup (coalesced, one latency) so that the two serial chain builders
    // below walk LDS, not global memory (one dependent global load per row otherwise)
    const bool ext_lds = rows <= HULL_LDS / 2;
    if (ext_lds)
        for (int r = tid; r < rows; r += 256) { s_ext[r] = rmin[r]; s_ext[HULL_LDS / 2 + r] = rmax[r]; }
    __syncthreads();
    // ---- hull: thread 0 builds the left chain in hull[0..], thread 64 (another wave) the right chain in hull[rows..] ----
    if (tid == 0 || tid == 64) {
        const bool left = tid == 0;
        int2* ch = hull + (left ? 0 : rows);
        int nc = 0;
        for (int t = 0; t < rows; ++t) {
            const int r = left ? t : rows - 1 - t;
            const int ex = ext_lds ? s_ext[(left ? 0 : HULL_LDS / 2) + r] : (left ? rmin[r] : rmax[r]);
            const int2 p = make_int2(ex, y0 + r);
            while (nc >= 2) {
                const int2 o = ch[nc - 2], a = ch[nc - 1];
                const long long cr = (long long)(a.x - o.x) * (p.y - o.y) - (long long)(a.y - o.y) * (p.x - o.x);
                if (cr >= 0) --nc; else break;
            }
            ch[nc++] = p;
        }
        if (left) s_nl = nc; else s_nr = nc;
    }
    __syncthreads();
    if (tid == 0) {  // splice: left chain then right chain, dropping duplicated joints
        int nh = s_nl;
        const int2* rc = hull + rows;
        for (int t = 0; t < s_nr; ++t) {
            const int2 p = rc[t];
            if (nh && hull[nh - 1].x == p.x && hull[nh - 1].y == p.y) continue;
            hull[nh++] = p;
        }
        if (nh > 1 && hull[0].x == hull[nh - 1].x && hull[0].y == hull[nh - 1].y) --nh;
        s_nh = nh;
    }
    __syncthreads();
    const int nh = s_nh;
    if (nh < 2) { if (tid == 0) *vflag = 0; return; }
    // ---- calipers: threads = edges ----
    Cand best; best.have = 0; best.dx = best.dy = best.mind = best.maxd = best.minn = best.maxn = 0; best.L = 1; best.A = 0;
    for (int e = tid; e < nh; e += 256) {
        const int2 a = hull[e], b = hull[(e + 1) % nh];
        long long dx = b.x - a.x, dy = b.y - a.y;
        if (dx == 0 && dy == 0) continue;
        const long long g = gcdll(dx, dy);
        dx /= g; dy /= g;
        if (dx < 0 || (dx == 0 && dy < 0)) { dx = -dx; dy = -dy; }
        long long mind = 0x7fffffffffffffffll, maxd = -0x7fffffffffffffffll - 1, minn = mind, maxn = maxd;
        for (int t = 0; t < nh; ++t) {
            const int2 q = hull[t];
            const long long pd = (long long)q.x * dx + (long long)q.y * dy, pn = -(long long)q.x * dy + (long long)q.y * dx;
            mind = pd < mind ? pd : mind; maxd = pd > maxd ? pd : maxd;
            minn = pn < minn ? pn : minn; maxn = pn > maxn ? pn : maxn;
        }
        Cand c; c.have = 1; c.dx = dx; c.dy = dy; c.mind = mind; c.maxd = maxd; c.minn = minn; c.maxn = maxn;
        c.L = dx * dx + dy * dy; c.A = (maxd - mind) * (maxn - minn);
        if (cand_better(c, best)) best = c;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        Cand o;
        o.have = __shfl_xor(best.have, m);
        o.dx = shfl_xor_ll(best.dx, m); o.dy = shfl_xor_ll(best.dy, m);
        o.mind = shfl_xor_ll(best.mind, m); o.maxd = shfl_xor_ll(best.maxd, m);
        o.minn = shfl_xor_ll(best.minn, m); o.maxn = shfl_xor_ll(best.maxn, m);
        o.L = shfl_xor_ll(best.L, m); o.A = shfl_xor_ll(best.A, m);
        if (cand_better(o, best)) best = o;
    }
    if (lane == 0) s_cand[wave] = best;
    __syncthreads();
    best = s_cand[0];
#pragma unroll
    for (int wv = 1; wv < 4; ++wv) { const Cand o = s_cand[wv]; if (cand_better(o, best)) best = o; }
    if (!best.have) { if (tid == 0) *vflag = 0; return; }
    const long long wd = best.maxd - best.mind, wn = best.maxn - best.minn;
    const double sqL = __dsqrt_rn((double)best.L);
    const double sside = (double)(wd < wn ? wd : wn) / sqL;
    if (sside < (double)min_size) { if (tid == 0) *vflag = 0; return; }
    // ---- score: integer pixels inside the closed rectangle (exact integer sum: order-free) ----
    double fx0, fx1, fy0, fy1;
    {
        const long long as[4] = {best.mind, best.maxd, best.maxd, best.mind}, bs[4] = {best.minn, best.minn, best.maxn, best.maxn};
        double cx[4], cy[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            cx[t] = (double)(as[t] * best.dx - bs[t] * best.dy) / (double)best.L;
            cy[t] = (double)(as[t] * best.dy + bs[t] * best.dx) / (double)best.L;
        }
        fx0 = fx1 = cx[0]; fy0 = fy1 = cy[0];
#pragma unroll
        for (int t = 1; t < 4; ++t) { fx0 = fmin(fx0, cx[t]); fx1 = fmax(fx1, cx[t]); fy0 = fmin(fy0, cy[t]); fy1 = fmax(fy1, cy[t]); }
    }
    int bx0 = (int)floor(fx0) - 1, bx1 = (int)ceil(fx1) + 1, by0 = (int)floor(fy0) - 1, by1 = (int)ceil(fy1) + 1;
    bx0 = bx0 < 0 ? 0 : bx0; by0 = by0 < 0 ? 0 : by0; bx1 = bx1 > vw - 1 ? vw - 1 : bx1; by1 = by1 > vh - 1 ? vh - 1 : by1;
    unsigned long long sum = 0, cnt = 0;
    const int bh = by1 - by0 + 1;
    const bf16_t* pp = prob + (size_t)pg * Hp * Wp;
    // all 256 threads sweep the bounding span in chunks of 8 pixels of a row, consecutive threads on consecutive chunks.  The two
    // projections are affine in x: a chunk forms them once (the only 64-bit products) and steps them by (dx, -dy) per pixel.  Where
    // every row of the map starts on a 16-byte boundary a chunk is one 16-byte load (the span's left edge moved down to a multiple
    // of 8; pixels outside [bx0, bx1] are masked); two chunks per thread are requested before the first inside-test.
    const bool vec = (Wp & 7) == 0 && (reinterpret_cast<uintptr_t>(prob) & 15) == 0;
    const int xa = vec ? bx0 & ~7 : bx0;
    if (bx1 < bx0 || bh <= 0) { if (tid == 0) *vflag = 0; return; }   // (no pixel: the count below would be 0)
    const int nch = ((bx1 - xa) >> 3) + 1, ntot = nch * bh;
    for (int i0 = 0; i0 < ntot; i0 += 256 * 2) {
        uint4 raw[2];
        int cx[2], cy[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int i = i0 + u * 256 + tid;
            const int ic = i < ntot ? i : 0;
            const int ry = ic / nch;
            cy[u] = i < ntot ? by0 + ry : -1;
            cx[u] = xa + ((ic - ry * nch) << 3);
            const bf16_t* src = pp + (size_t)(by0 + ry) * Wp + cx[u];
            if (vec) raw[u] = *reinterpret_cast<const uint4*>(src);
            else {
                unsigned int h[8];
#pragma unroll
                for (int t = 0; t < 8; ++t) h[t] = cx[u] + t <= bx1 ? src[t] : 0u;
                raw[u] = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
            }
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            long long pd = (long long)cx[u] * best.dx + (long long)cy[u] * best.dy, pn = -(long long)cx[u] * best.dy + (long long)cy[u] * best.dx;
            const unsigned int w[4] = {raw[u].x, raw[u].y, raw[u].z, raw[u].w};
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const int x = cx[u] + t;
                const float pv = __uint_as_float((t & 1) ? (w[t >> 1] & 0xffff0000u) : (w[t >> 1] << 16));
                const bool in = cy[u] >= 0 && x >= bx0 && x <= bx1 && pd >= best.mind && pd <= best.maxd && pn >= best.minn && pn <= best.maxn;
                sum += in ? (unsigned long long)(pv * 16777216.0f) : 0ull;
                cnt += in ? 1ull : 0ull;
                pd += best.dx; pn -= best.dy;
            }
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { sum += (unsigned long long)shfl_xor_ll((long long)sum, m); cnt += (unsigned long long)shfl_xor_ll((long long)cnt, m); }
    if (lane == 0) { s_sum[wave] = sum; s_cnt[wave] = cnt; }
    __syncthreads();
    if (tid != 0) return;
    sum = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
    cnt = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    if (!cnt) { *vflag = 0; return; }
    const double score = ((double)sum / (double)cnt) / 16777216.0;
    if (score < (double)box_thresh) { *vflag = 0; return; }
    // ---- unclip + corners ----
    const double E = ((double)unclip_ratio * (double)(wd * wn)) / (double)(2 * (wd + wn));
    const double sside2 = ((double)(wd < wn ? wd : wn) + 2.0 * E) / sqL;
    if (sside2 < (double)(min_size + 2)) { *vflag = 0; return; }
    const double a0 = (double)best.mind - E, a1 = (double)best.maxd + E, b0 = (double)best.minn - E, b1 = (double)best.maxn + E;
    double qx[4], qy[4];
    {
        const double as[4] = {a0, a1, a1, a0}, bs[4] = {b0, b0, b1, b1};
        const double ddx = (double)best.dx, ddy = (double)best.dy, dL = (double)best.L;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const double t1 = __dmul_rn(as[t], ddx), t2 = __dmul_rn(bs[t], ddy), t3 = __dmul_rn(as[t], ddy), t4 = __dmul_rn(bs[t], ddx);
            qx[t] = __ddiv_rn(__dsub_rn(t1, t2), dL);
            qy[t] = __ddiv_rn(__dadd_rn(t3, t4), dL);
        }
    }
    for (int i = 1; i < 4; ++i)
        for (int j = i; j > 0; --j) {
            const bool lt = qx[j] < qx[j - 1] || (qx[j] == qx[j - 1] && qy[j] < qy[j - 1]);
            if (!lt) break;
            const double tx = qx[j], ty = qy[j]; qx[j] = qx[j - 1]; qy[j] = qy[j - 1]; qx[j - 1] = tx; qy[j - 1] = ty;
        }
    double ox[4], oy[4];  // TL, TR, BR, BL
    if (qy[0] <= qy[1]) { ox[0] = qx[0]; oy[0] = qy[0]; ox[3] = qx[1]; oy[3] = qy[1]; } else { ox[0] = qx[1]; oy[0] = qy[1]; ox[3] = qx[0]; oy[3] = qy[0]; }
    if (qy[2] <= qy[3]) { ox[1] = qx[2]; oy[1] = qy[2]; ox[2] = qx[3]; oy[2] = qy[3]; } else { ox[1] = qx[3]; oy[1] = qy[3]; ox[2] = qx[2]; oy[2] = qy[2]; }
    int out[8];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        double rx = rint(ox[t]), ry = rint(oy[t]);
        rx = rx < 0 ? 0 : rx; rx = rx > vw ? vw : rx; ry = ry < 0 ? 0 : ry; ry = ry > vh ? vh : ry;
        out[2 * t] = (int)rx; out[2 * t + 1] = (int)ry;
    }
    {
        const double wx = (double)(out[0] - out[2]), wy = (double)(out[1] - out[3]);
        const double hx = (double)(out[0] - out[6]), hy = (double)(out[1] - out[7]);
        const int rw = (int)sqrt(__dadd_rn(__dmul_rn(wx, wx), __dmul_rn(wy, wy))), rh = (int)sqrt(__dadd_rn(__dmul_rn(hx, hx), __dmul_rn(hy, hy)));
        if (rw <= 3 || rh <= 3) { *vflag = 0; return; }
    }
    int* bo = box_tmp + ((size_t)pg * maxc + k) * 8;
#pragma unroll
    for (int t = 0; t < 8; ++t) bo[t] = out[t];
    score_tmp[(size_t)pg * maxc + k] = (float)score;
    *vflag = 1;
}

// 8a: the live components of the batch as one list, page by page in component order: live[i] = pg * maxc + k for k < min(ncomp, maxc),
// live[B * maxc] = their number.  One work-group per page; it sums the kept counts of the pages before its own.
__global__ __launch_bounds__(256) void live_list_kernel(const int* ncomp, int* live, int B, int maxc) {
    __shared__ int s_part[4];
    const int pg = blockIdx.x, tid = threadIdx.x;
    int before = 0;
    for (int q = tid; q < pg; q += 256) before += ncomp[q] < maxc ? ncomp[q] : maxc;
    before = wave_sum(before);
    if ((tid & 63) == 0) s_part[tid >> 6] = before;
    __syncthreads();
    const int off = s_part[0] + s_part[1] + s_part[2] + s_part[3];
    const int n = ncomp[pg] < maxc ? ncomp[pg] : maxc;
    for (int k = tid; k < n; k += 256) live[off + k] = pg * maxc + k;
    if (pg == B - 1 && tid == 0) live[(size_t)B * maxc] = off + n;
}
// 8b: a grid of what is resident; work-group g takes the live components g, g + gridDim.x, ...
__global__ __launch_bounds__(256) void comp_box_kernel(const bf16_t* prob, const int* live, int items_cap, const int* ymin, const int* ymax,
                                                       const int* segoff, const int* rowmin, const int* rowmax, int2* hullbuf, int* box_tmp,
                                                       float* score_tmp, int* valid_tmp, int Hp, int Wp, int vh, int vw, int maxc, size_t seg_cap,
                                                       float box_thresh, float unclip_ratio, int min_size) {
    int items = live[items_cap];
    items = items < items_cap ? items : items_cap;
    for (int it = blockIdx.x; it < items; it += gridDim.x) {
        const int code = live[it];
        comp_box_item(code / maxc, code % maxc, prob, ymin, ymax, segoff, rowmin, rowmax, hullbuf, box_tmp, score_tmp, valid_tmp, Hp, Wp, vh, vw, maxc,
                      seg_cap, box_thresh, unclip_ratio, min_size);
        __syncthreads();   // the item's LDS is free for the next one
    }
}

// ---- 9: slots at and past min(ncomp, maxc) hold no component (and no flag: comp_box only visits the live ones) ----
__global__ __launch_bounds__(64) void compact_kernel(const int* ncomp, const int* box_tmp, const float* score_tmp, const int* valid_tmp, int* boxes,
                                                     float* scores, int* counts, int maxc) {
    const int pg = blockIdx.x, lane = threadIdx.x;
    const int n = ncomp[pg] < maxc ? ncomp[pg] : maxc;
    int run = 0;
    for (int k0 = 0; k0 < n; k0 += 64) {
        const int k = k0 + lane;
        const bool v = k < n && valid_tmp[(size_t)pg * maxc + k] != 0;
        const unsigned long long m = __ballot(v);
        if (v) {
            const int pos = run + __popcll(m & ((1ull << lane) - 1ull));
#pragma unroll
            for (int t = 0; t < 8; ++t) boxes[((size_t)pg * maxc + pos) * 8 + t] = box_tmp[((size_t)pg * maxc + k) * 8 + t];
            scores[(size_t)pg * maxc + pos] = score_tmp[(size_t)pg * maxc + k];
        }
        run += __popcll(m);
    }
    if (lane == 0) counts[pg] = run;
}

// ---- crops: one block per crop, threads over (row, col).  CH x CW = 32 x 320 (recogniser) or 48 x 192 (orientation classifier).
// flip (optional): a crop whose flag is set is the 180-degree turn of the unflagged crop within its valid width — output (i, j) samples
// the source position of (CH-1-i, wc-1-j) with the same operations, so it equals the turned crop byte for byte ----
template <int CH, int CW>
__global__ __launch_bounds__(256) void crop_kernel(const uint8_t* pages, int H, int W, const int* quads, const int* page_idx, const int* flip,
                                                   uint8_t* crops, int* widths) {
    const int ci = blockIdx.x, tid = threadIdx.x;
    long long p[4][2];
#pragma unroll
    for (int t = 0; t < 4; ++t) { p[t][0] = quads[(size_t)ci * 8 + 2 * t]; p[t][1] = quads[(size_t)ci * 8 + 2 * t + 1]; }
#define D2(a, b) ((p[a][0] - p[b][0]) * (p[a][0] - p[b][0]) + (p[a][1] - p[b][1]) * (p[a][1] - p[b][1]))
    long long cw2 = D2(1, 0) > D2(2, 3) ? D2(1, 0) : D2(2, 3);
    long long ch2 = D2(3, 0) > D2(2, 1) ? D2(3, 0) : D2(2, 1);
#undef D2
    if (4 * ch2 >= 9 * cw2) {
        const long long t0 = p[0][0], t1 = p[0][1];
        p[0][0] = p[1][0]; p[0][1] = p[1][1]; p[1][0] = p[2][0]; p[1][1] = p[2][1];
        p[2][0] = p[3][0]; p[2][1] = p[3][1]; p[3][0] = t0; p[3][1] = t1;
        const long long t = cw2; cw2 = ch2; ch2 = t;
    }
    uint8_t* out = crops + (size_t)ci * CH * CW * 3;
    int wc = 0;
    if (ch2 != 0 && cw2 != 0) {
        const double ratio = sqrt(__ddiv_rn((double)cw2, (double)ch2));
        wc = (int)ceil(__dmul_rn((double)CH, ratio));
        wc = wc < 1 ? 1 : (wc > CW ? CW : wc);
    }
    if (tid == 0) widths[ci] = wc;
    const bool turn = flip != nullptr && flip[ci] != 0;
    const uint8_t* page = pages + (size_t)page_idx[ci] * H * W * 3;
    const float tlx = (float)p[0][0], tly = (float)p[0][1];
    const float ex = (float)(p[1][0] - p[0][0]), ey = (float)(p[1][1] - p[0][1]);
    const float fx = (float)(p[3][0] - p[0][0]), fy = (float)(p[3][1] - p[0][1]);
    // a thread owns 4 consecutive output columns of a row: 12 bytes, stored as three dwords (a crop row is CW * 3 bytes, a multiple
    // of 4).  The row terms (v and its products) are formed once for the four; every pixel keeps its own operations and their order.
    static_assert(CW % 4 == 0, "four columns per thread");
    const bool dword_out = (reinterpret_cast<uintptr_t>(crops) & 3) == 0;
    for (int t = tid; t < CH * (CW / 4); t += 256) {
        const int i = t / (CW / 4), j0 = (t - i * (CW / 4)) * 4;
        const int si = turn ? CH - 1 - i : i;
        const float v = __fdiv_rn((float)si + 0.5f, (float)CH);
        const float t2 = __fmul_rn(v, fx), t4 = __fmul_rn(v, fy);
        uint32_t px[4] = {0, 0, 0, 0};   // r | g << 8 | b << 16 of the four pixels
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = j0 + q;
            if (j >= wc) continue;
            const int sj = turn ? wc - 1 - j : j;
            const float u = __fdiv_rn((float)sj + 0.5f, (float)wc);
            const float t1 = __fmul_rn(u, ex), t3 = __fmul_rn(u, ey);
            const float sx = __fadd_rn(__fadd_rn(tlx, t1), t2), sy = __fadd_rn(__fadd_rn(tly, t3), t4);
            const float x0f = floorf(sx), y0f = floorf(sy);
            const float ax = __fsub_rn(sx, x0f), ay = __fsub_rn(sy, y0f);
            int x0 = (int)x0f, y0 = (int)y0f, x1 = x0 + 1, y1 = y0 + 1;
            x0 = x0 < 0 ? 0 : (x0 > W - 1 ? W - 1 : x0); x1 = x1 < 0 ? 0 : (x1 > W - 1 ? W - 1 : x1);
            y0 = y0 < 0 ? 0 : (y0 > H - 1 ? H - 1 : y0); y1 = y1 < 0 ? 0 : (y1 > H - 1 ? H - 1 : y1);
            const float bx = __fsub_rn(1.0f, ax), by = __fsub_rn(1.0f, ay);
            // the two taps of a page row are 6 adjacent bytes unless the clamp folded them onto one pixel: fetched as 4 + 2
            const uint8_t* r0 = page + ((size_t)y0 * W + x0) * 3;
            const uint8_t* r1 = page + ((size_t)y1 * W + x0) * 3;
            uint32_t a0, a1, b0, b1;   // bytes 0-3 (r g b r') and 4-5 (g' b') of the pair, per page row
            if (x1 == x0 + 1) {
                uint16_t h0, h1;
                __builtin_memcpy(&a0, r0, 4); __builtin_memcpy(&h0, r0 + 4, 2); __builtin_memcpy(&b0, r1, 4); __builtin_memcpy(&h1, r1 + 4, 2);
                a1 = h0; b1 = h1;
            } else {   // x1 == x0
                a0 = r0[0] | (r0[1] << 8) | (r0[2] << 16); b0 = r1[0] | (r1[1] << 8) | (r1[2] << 16);
                a1 = a0 >> 8; a0 |= a0 << 24; b1 = b0 >> 8; b0 |= b0 << 24;
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float p00 = (float)((a0 >> (8 * c)) & 255u), p10 = (float)((b0 >> (8 * c)) & 255u);
                const float p01 = (float)(c == 0 ? a0 >> 24 : (a1 >> (8 * (c - 1))) & 255u), p11 = (float)(c == 0 ? b0 >> 24 : (b1 >> (8 * (c - 1))) & 255u);
                const float top = __fadd_rn(__fmul_rn(bx, p00), __fmul_rn(ax, p01)), bot = __fadd_rn(__fmul_rn(bx, p10), __fmul_rn(ax, p11));
                float val = rintf(__fadd_rn(__fmul_rn(by, top), __fmul_rn(ay, bot)));
                val = val < 0.f ? 0.f : (val > 255.f ? 255.f : val);
                px[q] |= (uint32_t)val << (8 * c);
            }
        }
        uint8_t* o = out + (size_t)t * 12;
        const uint32_t w0 = px[0] | (px[1] << 24), w1 = (px[1] >> 8) | (px[2] << 16), w2 = (px[2] >> 16) | (px[3] << 8);
        if (dword_out) {
            uint32_t* od = reinterpret_cast<uint32_t*>(o);
            od[0] = w0; od[1] = w1; od[2] = w2;
        } else {
#pragma unroll
            for (int b = 0; b < 4; ++b) { o[b] = (uint8_t)(w0 >> (8 * b)); o[4 + b] = (uint8_t)(w1 >> (8 * b)); o[8 + b] = (uint8_t)(w2 >> (8 * b)); }
        }
    }
}

}  // namespace

// the workspace's regions: one layout sizes it (dbpost_workspace_bytes) and carves it (dbpost_launch)
struct DbWorkspace {
    unsigned long long* mask; int *runoff, *rootoff, *nruns, *ncomp; unsigned short *rxs, *rxe;
    int *parent, *cidr, *ymin, *ymax, *segoff, *rowmin, *rowmax; int2* hull; int* box_tmp; float* score_tmp; int* valid_tmp; int* live;
};
static DbWorkspace dbpost_layout(Arena& a, int B, int Hp, int Wp, int maxc) {
    const size_t seg_cap = (size_t)maxc * Hp;  // worst case: every candidate spans the page height
    const size_t runcap = run_cap(Hp, Wp), nseg = (Wp + 63) / 64;
    DbWorkspace w;
    w.mask = a.take<unsigned long long>((size_t)B * Hp * nseg);
    w.runoff = a.take<int>((size_t)B * (Hp + 1)); w.rootoff = a.take<int>((size_t)B * (Hp + 1));   // run / root counts -> offsets
    w.nruns = a.take<int>(B); w.ncomp = a.take<int>(B);
    w.rxs = a.take<unsigned short>((size_t)B * runcap); w.rxe = a.take<unsigned short>((size_t)B * runcap);
    w.parent = a.take<int>((size_t)B * runcap); w.cidr = a.take<int>((size_t)B * runcap);   // (component id of root runs)
    w.ymin = a.take<int>((size_t)B * maxc); w.ymax = a.take<int>((size_t)B * maxc);
    w.segoff = a.take<int>((size_t)B * (maxc + 1));
    w.rowmin = a.take<int>((size_t)B * seg_cap); w.rowmax = a.take<int>((size_t)B * seg_cap);
    w.hull = a.take<int2>((size_t)B * seg_cap * 2);
    w.box_tmp = a.take<int>((size_t)B * maxc * 8); w.score_tmp = a.take<float>((size_t)B * maxc); w.valid_tmp = a.take<int>((size_t)B * maxc);
    w.live = a.take<int>((size_t)B * maxc + 1);   // live components (page * maxc + id) + their number
    return w;
}

size_t dbpost_workspace_bytes(int B, int Hp, int Wp, int maxc) {
    Arena a;
    dbpost_layout(a, B, Hp, Wp, maxc);
    return a.off;
}

hipError_t dbpost_launch(const DbPostParams& p, void* workspace, size_t ws_bytes, hipStream_t st) {
    const int B = p.B, Hp = p.Hp, Wp = p.Wp, maxc = p.max_boxes;
    if (B <= 0 || Hp <= 0 || Wp <= 0 || Wp > 65535 || maxc <= 0 || (size_t)B * Hp >= (1ull << 31) || (size_t)B * maxc >= (1ull << 31) || run_cap(Hp, Wp) >= (1ull << 31)) return hipErrorInvalidValue;
    const size_t seg_cap = (size_t)maxc * Hp, runcap = run_cap(Hp, Wp);
    const int nseg = (Wp + 63) / 64;
    Arena a(workspace, ws_bytes);
    const DbWorkspace w = dbpost_layout(a, B, Hp, Wp, maxc);
    if (a.overflow) return hipErrorOutOfMemory;
    int dev = 0, cus = 0;
    { hipError_t e = hipGetDevice(&dev); if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev); if (e != hipSuccess) return e; }

    const int rows = B * Hp;
    const dim3 grows = row_wave_grid(rows);
    hipLaunchKernelGGL(rl_mask_kernel, grows, dim3(256), 0, st, p.prob, w.mask, w.runoff, Hp, Wp, nseg, p.valid_h, p.valid_w, p.thresh, rows);
    row_scan_launch(w.runoff, w.nruns, B, Hp, st);
    run_fill_launch(w.mask, w.runoff, w.rxs, w.rxe, w.parent, nullptr, B, Hp, nseg, runcap, st);
    run_merge_launch(w.runoff, w.rxs, w.rxe, w.parent, B, Hp, runcap, st);
    hipLaunchKernelGGL(rl_roots_kernel, grows, dim3(256), 0, st, w.runoff, w.parent, w.rootoff, Hp, runcap, rows);
    row_scan_launch(w.rootoff, w.ncomp, B, Hp, st);
    hipLaunchKernelGGL(rl_assign_kernel, grows, dim3(256), 0, st, w.runoff, w.rootoff, w.parent, w.cidr, w.ymin, w.ymax, Hp, runcap, maxc, rows);
    hipLaunchKernelGGL(rl_extent_kernel, grows, dim3(256), 0, st, w.runoff, w.rxs, w.rxe, w.parent, w.cidr, w.ymax, Hp, runcap, maxc, rows);
    hipLaunchKernelGGL(seg_scan_kernel, dim3(B), dim3(64), 0, st, w.ncomp, w.ymin, w.ymax, w.segoff, maxc);
    hipLaunchKernelGGL(seg_init_kernel, dim3(64, B), dim3(256), 0, st, w.ncomp, w.segoff, w.rowmin, w.rowmax, maxc, seg_cap);
    hipLaunchKernelGGL(rl_extremes_kernel, grows, dim3(256), 0, st, w.runoff, w.rxs, w.rxe, w.parent, w.cidr, w.ymin, w.segoff, w.rowmin, w.rowmax, Hp, runcap, maxc, seg_cap, rows);
    hipLaunchKernelGGL(live_list_kernel, dim3(B), dim3(256), 0, st, w.ncomp, w.live, B, maxc);
    // comp_box holds 48 KB of LDS: three work-groups are resident on a compute unit
    const int resident = cus * 3 < B * maxc ? cus * 3 : B * maxc;
    hipLaunchKernelGGL(comp_box_kernel, dim3(resident), dim3(256), 0, st, p.prob, w.live, B * maxc, w.ymin, w.ymax, w.segoff, w.rowmin, w.rowmax, w.hull, w.box_tmp,
                       w.score_tmp, w.valid_tmp, Hp, Wp, p.valid_h, p.valid_w, maxc, seg_cap, p.box_thresh, p.unclip_ratio, p.min_size);
    hipLaunchKernelGGL(compact_kernel, dim3(B), dim3(64), 0, st, w.ncomp, w.box_tmp, w.score_tmp, w.valid_tmp, p.boxes, p.scores, p.counts, maxc);
    return hipGetLastError();
}

hipError_t rec_crop_launch(const uint8_t* pages, int H, int W, const int* quads, const int* page_idx, int n, uint8_t* crops, int* widths,
                           hipStream_t st, const int* flip) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL((crop_kernel<32, 320>), dim3(n), dim3(256), 0, st, pages, H, W, quads, page_idx, flip, crops, widths);
    return hipGetLastError();
}

hipError_t cls_crop_launch(const uint8_t* pages, int H, int W, const int* quads, const int* page_idx, int n, uint8_t* crops, int* widths,
                           hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL((crop_kernel<48, 192>), dim3(n), dim3(256), 0, st, pages, H, W, quads, page_idx, nullptr, crops, widths);
    return hipGetLastError();
}
