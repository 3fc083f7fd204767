// The kernels the page-analysis passes share (gfx950), each written once: the ink mask of a page and its bit transpose, and the run
// list of a batch of row masks — count, scan, fill, 8-connected merge — and, behind components_launch, the components of all ink with
// box, area and extremes at their roots.  Their users are dbpost.hip (runs of the binarised probability map), marks.hip, qrcodes.hip,
// datamatrix.hip and aztec.hip (components of all ink), tables.hip and orient.hip (mask and transpose).  Everything is integer.
#include "runs.h"

namespace {

typedef unsigned long long u64;

// ---- ink mask: one wave per page row, four rows per work-group; four 64-pixel segments are requested at a time ----
__global__ __launch_bounds__(256) void ink_mask_kernel(const uint8_t* rgb, u64* mask, int W, int nw, int threshold, long long rows_total) {
    const long long wrow = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (wrow >= rows_total) return;
    const uint8_t* rp = rgb + (size_t)wrow * W * 3;
    u64* mrow = mask + (size_t)wrow * nw;
    for (int s0 = 0; s0 < nw; s0 += 4) {
        int l[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int x = (s0 + u) * 64 + lane;
            const uint8_t* s = rp + (size_t)(x < W ? x : W - 1) * 3;
            l[u] = (int)((19595u * s[0] + 38470u * s[1] + 7471u * s[2] + 0x8000u) >> 16);
        }
        u64 mine = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const u64 m = __ballot((s0 + u) * 64 + lane < W && l[u] < threshold);
            if (lane == u) mine = m;
        }
        if (lane < 4 && s0 + lane < nw) mrow[s0 + lane] = mine;
    }
}

// ---- bit transpose: one wave per 64 x 64 bit block: lane r holds row r's word, ballot c is column c's word ----
__global__ __launch_bounds__(256) void ink_transpose_kernel(const u64* hmask, u64* vmask, int H, int W, int nw, int nhw, long long blocks_total) {
    const long long wb = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (wb >= blocks_total) return;
    const int cb = (int)(wb % nw), rb = (int)((wb / nw) % nhw), pg = (int)(wb / ((long long)nw * nhw));
    const int row = rb * 64 + lane;
    const u64 w = row < H ? hmask[((size_t)pg * H + row) * nw + cb] : 0ull;
    u64 mine = 0;
#pragma unroll 8
    for (int c = 0; c < 64; ++c) {
        const u64 v = __ballot((w >> c) & 1ull);
        if (lane == c) mine = v;
    }
    const int col = cb * 64 + lane;
    if (col < W) vmask[((size_t)pg * W + col) * nhw + rb] = mine;
}

// ---- run list.  A row of a mask is a short list of runs (a probability map: ~10 per row, all ink of a text page: ~100), in raster
// order.  These kernels are one wave per (page, row), four rows per work-group (row_wave). ----
// number of runs in the row; lanes = words
__global__ __launch_bounds__(256) void run_count_kernel(const u64* mask, int* runcnt, int H, int nw, int rows_total) {
    int pg, row, lane;
    if (!row_wave(H, rows_total, pg, row, lane)) return;
    const u64* mrow = mask + ((size_t)pg * H + row) * nw;
    int cnt = 0;
    u64 carry = 0;
    for (int s0 = 0; s0 < nw; s0 += 64) {
        const int sg = s0 + lane;
        const u64 m = sg < nw ? mrow[sg] : 0ull;
        u64 prev = (u64)(unsigned)__shfl_up((int)(m >> 63), 1);
        if (lane == 0) prev = carry;
        cnt += __popcll(run_starts(m, prev));
        carry = (u64)(unsigned)__shfl((int)(m >> 63), 63);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d);
    if (lane == 0) runcnt[(size_t)pg * (H + 1) + row] = cnt;
}
// exclusive scan of a page's H row counts (one wave, chunked): cnt[r] -> offset of row r, cnt[H] = total (also -> total_out)
__global__ __launch_bounds__(64) void row_scan_kernel(int* cnt, int* total_out, int H) {
    const int pg = blockIdx.x, lane = threadIdx.x;
    int* rc = cnt + (size_t)pg * (H + 1);
    int run = 0;
    for (int r0 = 0; r0 < H; r0 += 64) {
        const int r = r0 + lane;
        const int v = r < H ? rc[r] : 0;
        int inc = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(inc, d); if (lane >= d) inc += t; }
        if (r < H) rc[r] = run + inc - v;
        run += __shfl(inc, 63);
    }
    if (lane == 0) { rc[H] = run; if (total_out) total_out[pg] = run; }
}
// masks -> runs [xs, xe] of the row at its offset in the page's run list; a run is its own union-find parent.  Lanes = words: the
// j-th run start of the row pairs with the j-th run end (a run may span words), so starts and ends are ranked separately.
// BOX: the run is also its own bounding box (x0, x1, y0, y1), which a component later accumulates at its root.
template <bool BOX>
__global__ __launch_bounds__(256) void run_fill_kernel(const u64* mask, const int* runoff, unsigned short* rxs, unsigned short* rxe, int* parent, int4* box,
                                                       int H, int nw, size_t runcap, int rows_total) {
    int pg, row, lane;
    if (!row_wave(H, rows_total, pg, row, lane)) return;
    const u64* mrow = mask + ((size_t)pg * H + row) * nw;
    const size_t rb = (size_t)pg * runcap;
    int sbase = runoff[(size_t)pg * (H + 1) + row], ebase = sbase;
    u64 carry = 0;
    for (int s0 = 0; s0 < nw; s0 += 64) {
        const int sg = s0 + lane;
        const u64 m = sg < nw ? mrow[sg] : 0ull;
        u64 prev = (u64)__shfl_up((int)(m >> 63), 1);            // bit 63 of the word to the left
        if (lane == 0) prev = carry;
        u64 next = (u64)(__shfl_down((int)(m & 1ull), 1) & 1);    // bit 0 of the word to the right
        if (lane == 63) next = s0 + 64 < nw ? (mrow[s0 + 64] & 1ull) : 0ull;
        u64 st = run_starts(m, prev), en = m & ~((m >> 1) | (next << 63));
        int si = __popcll(st), ei = __popcll(en);
        const int ns = si, ne = ei;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int a = __shfl_up(si, d), b = __shfl_up(ei, d);
            if (lane >= d) { si += a; ei += b; }
        }
        int sp = sbase + si - ns, ep = ebase + ei - ne;   // exclusive ranks
        while (st) {
            const int x = sg * 64 + (__ffsll((long long)st) - 1);
            st &= st - 1;
            rxs[rb + sp] = (unsigned short)x; parent[rb + sp] = sp;
            if (BOX) { int* b = reinterpret_cast<int*>(box + rb + sp); b[0] = x; b[2] = row; b[3] = row; }
            ++sp;
        }
        while (en) {
            const int x = sg * 64 + (__ffsll((long long)en) - 1);
            en &= en - 1;
            rxe[rb + ep] = (unsigned short)x;
            if (BOX) reinterpret_cast<int*>(box + rb + ep)[1] = x;
            ++ep;
        }
        sbase += __shfl(si, 63); ebase += __shfl(ei, 63);
        carry = (u64)__shfl((int)(m >> 63), 63);
    }
}
// a run joins every run of the row above that it touches (8-connectivity: [xs - 1, xe + 1] overlaps [xs', xe']).  Run ids grow in
// raster order and the union keeps the smaller root, so a component's root is its first run — the one that starts at the
// component's smallest linear pixel index, the canonical root of the per-pixel definition.
__global__ __launch_bounds__(256) void run_merge_kernel(const int* runoff, const unsigned short* rxs, const unsigned short* rxe, int* parent, int H,
                                                        size_t runcap, int rows_total) {
    int pg, row, lane;
    if (!row_wave(H, rows_total, pg, row, lane)) return;
    if (row == 0) return;
    const int* ro = runoff + (size_t)pg * (H + 1);
    const int u0 = ro[row - 1], r0 = ro[row], r1 = ro[row + 1];
    if (u0 == r0) return;
    const size_t rb = (size_t)pg * runcap;
    int* P = parent + rb;
    for (int id = r0 + lane; id < r1; id += 64) {
        const int xs = rxs[rb + id], xe = rxe[rb + id];
        int lo = u0, hi = r0;   // first run of the row above with xe' + 1 >= xs
        while (lo < hi) { const int mid = (lo + hi) >> 1; if ((int)rxe[rb + mid] + 1 < xs) lo = mid + 1; else hi = mid; }
        for (int t = lo; t < r0 && (int)rxs[rb + t] <= xe + 1; ++t) uf_union(P, id, t);
    }
}

// ---- components: a run's own length (and extremes) is the start of its component's ----
template <bool EXT>
__global__ __launch_bounds__(256) void run_area_kernel(const int* runoff, const unsigned short* rxs, const unsigned short* rxe, int* area, u64* ext, int H,
                                                       size_t runcap, int rows_total) {
    int pg, row, lane;
    if (!row_wave(H, rows_total, pg, row, lane)) return;
    const int* ro = runoff + (size_t)pg * (H + 1);
    const size_t rb = (size_t)pg * runcap;
    for (int id = ro[row] + lane; id < ro[row + 1]; id += 64) {
        const int xs = rxs[rb + id], xe = rxe[rb + id];
        area[rb + id] = xe - xs + 1;
        if (EXT) {
            u64 e[4];
            run_extremes(xs, xe, row, e);
#pragma unroll
            for (int j = 0; j < 4; ++j) ext[(rb + id) * 4 + j] = e[j];
        }
    }
}

// parent = root; the root's box grows to the component's (run_join_root), its area by every other run's length (AREA), its extremes to
// the component's (EXT; as for the box, an atomic is issued only when the value read before it would change)
template <bool AREA, bool EXT>
__global__ __launch_bounds__(256) void run_accum_kernel(const int* runoff, const unsigned short* rxs, const unsigned short* rxe, int* parent, int4* box, int* area,
                                                        u64* ext, int H, size_t runcap, int rows_total) {
    int pg, row, lane;
    if (!row_wave(H, rows_total, pg, row, lane)) return;
    const int* ro = runoff + (size_t)pg * (H + 1);
    const size_t rb = (size_t)pg * runcap;
    for (int id = ro[row] + lane; id < ro[row + 1]; id += 64) {
        int xs, xe;
        const int root = run_join_root(parent + rb, rxs + rb, rxe + rb, box + rb, id, row, xs, xe);
        if (root < 0) continue;
        if (AREA) atomicAdd(area + rb + root, xe - xs + 1);
        if (EXT) {
            u64 e[4];
            run_extremes(xs, xe, row, e);
            u64* x = ext + (rb + root) * 4;
            if (e[0] < __atomic_load_n(x + 0, __ATOMIC_RELAXED)) atomicMin(x + 0, e[0]);
            if (e[1] > __atomic_load_n(x + 1, __ATOMIC_RELAXED)) atomicMax(x + 1, e[1]);
            if (e[2] > __atomic_load_n(x + 2, __ATOMIC_RELAXED)) atomicMax(x + 2, e[2]);
            if (e[3] < __atomic_load_n(x + 3, __ATOMIC_RELAXED)) atomicMin(x + 3, e[3]);
        }
    }
}

}  // namespace

hipError_t ink_mask_launch(const uint8_t* rgb, unsigned long long* mask, int B, int H, int W, int threshold, hipStream_t st) {
    if (!rgb || !mask || B <= 0 || H <= 0 || W <= 0 || (size_t)B * H >= (1ull << 31)) return hipErrorInvalidValue;
    const long long rows = (long long)B * H;
    hipLaunchKernelGGL(ink_mask_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, rgb, mask, W, (W + 63) / 64, threshold, rows);
    return hipGetLastError();
}

hipError_t ink_transpose_launch(const unsigned long long* hmask, unsigned long long* vmask, int B, int H, int W, hipStream_t st) {
    if (!hmask || !vmask || B <= 0 || H <= 0 || W <= 0) return hipErrorInvalidValue;
    const int nw = (W + 63) / 64, nhw = (H + 63) / 64;
    const long long blocks = (long long)B * nw * nhw;
    if (blocks >= (1ll << 33)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ink_transpose_kernel, dim3((unsigned)((blocks + 3) / 4)), dim3(256), 0, st, hmask, vmask, H, W, nw, nhw, blocks);
    return hipGetLastError();
}

hipError_t ink_mask_resolve(const uint8_t* rgb, const unsigned long long* mask_in, unsigned long long* mask_out, unsigned long long* scratch,
                            int B, int H, int W, int threshold, hipStream_t st, const unsigned long long** mask) {
    *mask = mask_in ? mask_in : (mask_out ? mask_out : scratch);
    if (!mask_in) return ink_mask_launch(rgb, mask_out ? mask_out : scratch, B, H, W, threshold, st);
    if (!mask_out) return hipSuccess;
    return hipMemcpyAsync(mask_out, mask_in, sizeof(unsigned long long) * (size_t)B * H * ((W + 63) / 64), hipMemcpyDeviceToDevice, st);
}

void run_count_launch(const unsigned long long* mask, int* runcnt, int B, int H, int nw, hipStream_t st) {
    hipLaunchKernelGGL(run_count_kernel, row_wave_grid(B * H), dim3(256), 0, st, mask, runcnt, H, nw, B * H);
}
void row_scan_launch(int* cnt, int* total_out, int B, int H, hipStream_t st) {
    hipLaunchKernelGGL(row_scan_kernel, dim3(B), dim3(64), 0, st, cnt, total_out, H);
}
void run_fill_launch(const unsigned long long* mask, const int* runoff, unsigned short* rxs, unsigned short* rxe, int* parent, int4* box, int B,
                     int H, int nw, size_t runcap, hipStream_t st) {
    if (box) hipLaunchKernelGGL(run_fill_kernel<true>, row_wave_grid(B * H), dim3(256), 0, st, mask, runoff, rxs, rxe, parent, box, H, nw, runcap, B * H);
    else hipLaunchKernelGGL(run_fill_kernel<false>, row_wave_grid(B * H), dim3(256), 0, st, mask, runoff, rxs, rxe, parent, box, H, nw, runcap, B * H);
}
void run_merge_launch(const int* runoff, const unsigned short* rxs, const unsigned short* rxe, int* parent, int B, int H, size_t runcap,
                      hipStream_t st) {
    hipLaunchKernelGGL(run_merge_kernel, row_wave_grid(B * H), dim3(256), 0, st, runoff, rxs, rxe, parent, H, runcap, B * H);
}

Components components_layout(Arena& a, int B, int H, int W, bool area) {
    const size_t runcap = run_cap(H, W), nw = (W + 63) / 64;
    Components c{};
    c.mask_buf = a.take<u64>((size_t)B * H * nw);
    c.runoff = a.take<int>((size_t)B * (H + 1));
    c.rxs = a.take<unsigned short>((size_t)B * runcap); c.rxe = a.take<unsigned short>((size_t)B * runcap);
    c.parent = a.take<int>((size_t)B * runcap);
    c.box = a.take<int4>((size_t)B * runcap);
    c.area = area ? a.take<int>((size_t)B * runcap) : nullptr;
    return c;
}

bool page_args_ok(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0 || H > 65535 || W > 65535) return false;
    return (size_t)B * H < (1ull << 31) && run_cap(H, W) < (1ull << 31);
}

hipError_t components_launch(Components& c, const uint8_t* rgb, const unsigned long long* mask_in, unsigned long long* mask_out, int B, int H, int W,
                             int threshold, hipStream_t st) {
    if (c.ext && !c.area) return hipErrorInvalidValue;
    const hipError_t e = ink_mask_resolve(rgb, mask_in, mask_out, c.mask_buf, B, H, W, threshold, st, &c.mask);
    if (e != hipSuccess) return e;
    const int nw = (W + 63) / 64, rows = B * H;
    const size_t runcap = run_cap(H, W);
    const dim3 grows = row_wave_grid(rows);
    run_count_launch(c.mask, c.runoff, B, H, nw, st);
    row_scan_launch(c.runoff, nullptr, B, H, st);
    run_fill_launch(c.mask, c.runoff, c.rxs, c.rxe, c.parent, c.box, B, H, nw, runcap, st);
    run_merge_launch(c.runoff, c.rxs, c.rxe, c.parent, B, H, runcap, st);
    const auto area = c.ext ? run_area_kernel<true> : run_area_kernel<false>;
    const auto accum = c.ext ? run_accum_kernel<true, true> : c.area ? run_accum_kernel<true, false> : run_accum_kernel<false, false>;
    if (c.area) hipLaunchKernelGGL(area, grows, dim3(256), 0, st, c.runoff, c.rxs, c.rxe, c.area, c.ext, H, runcap, rows);
    hipLaunchKernelGGL(accum, grows, dim3(256), 0, st, c.runoff, c.rxs, c.rxe, c.parent, c.box, c.area, c.ext, H, runcap, rows);
    return hipSuccess;
}
