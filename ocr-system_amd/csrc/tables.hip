// Rule extraction for ruled ("lattice") tables on the GPU (gfx950): the long thin ink lines of a page, horizontal and vertical, as
// (x0, y0, x1, y1, area) in a canonical order.  Everything is integer and every reduction is order-free (min / max / add), so the
// lists equal the sequential definition restated in tests/table_reference.py.
//
// All stream-ordered kernels, no host round trip:
//   1 ink_mask       (runs.hip) ink = L < threshold packed into 64-bit words along x, one wave ballot per 64 pixels (the page is read once)
//   2 ink_transpose  (runs.hip) the same mask with x and y exchanged (64 x 64 bit blocks, 64 ballots each): the vertical pass below is the
//                    horizontal pass on it.  From here on a "line" is a row (horizontal) or a column (vertical) and a "position"
//                    runs along it; kernels 3-6 take both directions in one launch, one thread per line (a line holds few runs)
//   3 tb_fill        maximal ink runs of the line, merged across gaps <= gap, kept when >= min_len long -> the line's slots.
//                    Kept runs are >= min_len long and > gap apart, so a line has at most (C + gap + 1) / (min_len + gap + 1)
//                    of them: slots are at fixed places (line * cap + k), which grow in raster order
//   4 tb_merge       union-find (atomicMin) over slots: a run joins the runs of the line before it whose intervals overlap its own;
//                    the root of a component is its first slot in raster order
//   5 tb_accum       bounding box and area of every component, accumulated at its root (integer atomics)
//   6 tb_select      roots that are rules (length >= min_len, area <= max_thick * length) -> counted, gathered in arrival order
//   7 tb_sort        one work-group per (page, direction): rank sort by (line0, pos0, line1, pos1, area, slot) -> the output
#include "tables.h"
#include "runs.h"

namespace {

typedef unsigned long long u64;

// one direction of the pass: R lines of C positions per page
struct TDir {
    const u64* mask;   // [B][R][nw]
    int R, C, nw, cap; // cap: slots per line
    unsigned* runs;    // [B][R][cap] start | end << 16
    int* parent;       // [B][R][cap] union-find over the page's slots (line * cap + k)
    int4* stat;        // [B][R][cap] at a root: min start, max end, last line, area of its component
    int* nrun;         // [B][R]
};
struct TDirs { TDir d[2]; int B; };

// thread -> (direction, page, line); horizontal lines first
#define LINE_DECODE                                                          \
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;          \
    const long long nh = (long long)D.B * D.d[0].R;                           \
    if (gid >= nh + (long long)D.B * D.d[1].R) return;                        \
    const int dir = gid >= nh;                                                \
    const TDir& d = D.d[dir];                                                 \
    const long long lg = dir ? gid - nh : gid;                                \
    const int pg = (int)(lg / d.R), line = (int)(lg % d.R);                   \
    const size_t lb = (size_t)pg * d.R + line, sb = lb * d.cap, pb = (size_t)pg * d.R * d.cap;

// 3
struct RunAcc { int cs, ce, k; };
__device__ __forceinline__ void tb_emit(const TDir& d, size_t sb, int line, RunAcc& a, int min_len) {
    if (a.cs >= 0 && a.ce - a.cs + 1 >= min_len && a.k < d.cap) {
        const size_t i = sb + a.k;
        d.runs[i] = (unsigned)a.cs | ((unsigned)a.ce << 16);
        d.parent[i] = line * d.cap + a.k;
        d.stat[i] = make_int4(a.cs, a.ce, line, 0);
        ++a.k;
    }
}
__device__ __forceinline__ void tb_raw_run(const TDir& d, size_t sb, int line, RunAcc& a, int rs, int re, int gap, int min_len) {
    if (a.cs >= 0 && rs - a.ce - 1 <= gap) { a.ce = re; return; }
    tb_emit(d, sb, line, a, min_len);
    a.cs = rs; a.ce = re;
}
__global__ __launch_bounds__(256) void tb_fill_kernel(TDirs D, int gap, int min_len) {
    LINE_DECODE
    (void)pb;
    const u64* m = d.mask + lb * d.nw;
    RunAcc a; a.cs = -1; a.ce = 0; a.k = 0;
    bool in = false;
    int s = 0;
    for (int wi = 0; wi < d.nw; ++wi) {
        const u64 w = m[wi];
        if (!in && w == 0ull) continue;
        int bit = 0;
        while (bit < 64) {
            const u64 rest = (in ? ~w : w) >> bit;
            if (rest == 0ull) break;
            const int b = bit + __ffsll((long long)rest) - 1;
            if (!in) { s = wi * 64 + b; in = true; }
            else { in = false; tb_raw_run(d, sb, line, a, s, wi * 64 + b - 1, gap, min_len); }
            bit = b;
        }
    }
    if (in) tb_raw_run(d, sb, line, a, s, d.C - 1, gap, min_len);   // (only when C is a multiple of 64: bits past C are 0)
    tb_emit(d, sb, line, a, min_len);
    d.nrun[lb] = a.k;
}

// 4: both lists are sorted and disjoint, so the first candidate of the line before only moves forward
__global__ __launch_bounds__(256) void tb_merge_kernel(TDirs D) {
    LINE_DECODE
    if (line == 0) return;
    const int n1 = d.nrun[lb], n0 = d.nrun[lb - 1];
    if (n1 == 0 || n0 == 0) return;
    int* P = d.parent + pb;
    const unsigned* cur = d.runs + sb;
    const unsigned* prev = d.runs + sb - d.cap;
    int j = 0;
    for (int i = 0; i < n1; ++i) {
        const int xs = (int)(cur[i] & 0xffffu), xe = (int)(cur[i] >> 16);
        while (j < n0 && (int)(prev[j] >> 16) < xs) ++j;
        for (int t = j; t < n0 && (int)(prev[t] & 0xffffu) <= xe; ++t) uf_union(P, line * d.cap + i, (line - 1) * d.cap + t);
    }
}

// 5
__global__ __launch_bounds__(256) void tb_accum_kernel(TDirs D) {
    LINE_DECODE
    const int n1 = d.nrun[lb];
    const int* P = d.parent + pb;
    for (int i = 0; i < n1; ++i) {
        const unsigned r = d.runs[sb + i];
        const int xs = (int)(r & 0xffffu), xe = (int)(r >> 16);
        const int root = uf_find(P, line * d.cap + i);
        int* st = reinterpret_cast<int*>(d.stat + pb + root);
        if (root != line * d.cap + i) { atomicMin(st + 0, xs); atomicMax(st + 1, xe); atomicMax(st + 2, line); }
        atomicAdd(st + 3, xe - xs + 1);
    }
}

// 6: tmp [B][2][max_rules][6] = line0, pos0, line1, pos1, area, slot
__global__ __launch_bounds__(256) void tb_select_kernel(TDirs D, int min_len, int max_thick, int max_rules, int* counts, int* tmp) {
    LINE_DECODE
    (void)sb;
    const int n1 = d.nrun[lb];
    const int* P = d.parent + pb;
    for (int i = 0; i < n1; ++i) {
        const int id = line * d.cap + i;
        if (P[id] != id) continue;
        const int4 st = d.stat[pb + id];
        const int length = st.y - st.x + 1;
        if (length < min_len || (long long)st.w > (long long)max_thick * length) continue;
        const int idx = atomicAdd(&counts[pg * 2 + dir], 1);
        if (idx < max_rules) {
            int* t = tmp + (((size_t)pg * 2 + dir) * max_rules + idx) * 6;
            t[0] = line; t[1] = st.x; t[2] = st.z; t[3] = st.y; t[4] = st.w; t[5] = id;
        }
    }
}

// 7
__global__ __launch_bounds__(256) void tb_sort_kernel(const int* counts, const int* tmp, int* hrules, int* vrules, int max_rules) {
    __shared__ int s_key[TABLE_MAX_RULES * 6];
    const int pg = blockIdx.x >> 1, dir = blockIdx.x & 1;
    const int n = counts[pg * 2 + dir];
    if (n > max_rules) return;   // overflow: the count is all that is reported
    int* out = (dir ? vrules : hrules) + (size_t)pg * max_rules * 5;
    rank_sort<6>(s_key, tmp + ((size_t)pg * 2 + dir) * max_rules * 6, 6, n, [=](int, int rank, const int (&k)[6]) {
        int* o = out + (size_t)rank * 5;
        if (dir == 0) { o[0] = k[1]; o[1] = k[0]; o[2] = k[3]; o[3] = k[2]; }   // line = y, position = x
        else          { o[0] = k[0]; o[1] = k[1]; o[2] = k[2]; o[3] = k[3]; }   // line = x, position = y
        o[4] = k[4];
    });
}

}  // namespace

static int table_cap(int C, int gap, int min_len) {
    const int c = (C + gap + 1) / (min_len + gap + 1);
    return c < 1 ? 1 : c;
}

// the workspace's regions: one layout sizes it (table_workspace_bytes) and carves it (table_rules_launch)
struct TableWorkspace {
    unsigned long long *hmask, *vmask;
    unsigned* runs[2]; int* parent[2]; int4* stat[2]; int* nrun[2];
    int* tmp;
};
static TableWorkspace table_layout(Arena& a, int B, int H, int W, int gap, int min_len, int max_rules) {
    const size_t nw = (W + 63) / 64, nhw = (H + 63) / 64;
    const int R[2] = {H, W}, C[2] = {W, H};
    TableWorkspace w;
    w.hmask = a.take<unsigned long long>((size_t)B * H * nw);
    w.vmask = a.take<unsigned long long>((size_t)B * W * nhw);
    for (int k = 0; k < 2; ++k) {
        const size_t slots = (size_t)B * R[k] * table_cap(C[k], gap, min_len);
        w.runs[k] = a.take<unsigned>(slots); w.parent[k] = a.take<int>(slots); w.stat[k] = a.take<int4>(slots);
        w.nrun[k] = a.take<int>((size_t)B * R[k]);
    }
    w.tmp = a.take<int>((size_t)B * 2 * max_rules * 6);
    return w;
}

static bool table_args_ok(int B, int H, int W, int gap, int min_len, int max_rules) {
    if (B <= 0 || H <= 0 || W <= 0 || H > 65535 || W > 65535 || gap < 0 || gap > 65535 || min_len < 1 || min_len > 65535) return false;
    if (max_rules < 1 || max_rules > TABLE_MAX_RULES) return false;
    if ((size_t)B * ((size_t)H + W) >= (1ull << 31) || (size_t)H * W >= (1ull << 31)) return false;
    return (size_t)H * table_cap(W, gap, min_len) < (1ull << 31) && (size_t)W * table_cap(H, gap, min_len) < (1ull << 31);
}

size_t table_workspace_bytes(int B, int H, int W, int gap, int min_len, int max_rules) {
    if (!table_args_ok(B, H, W, gap, min_len, max_rules)) return 0;
    Arena a;
    table_layout(a, B, H, W, gap, min_len, max_rules);
    return a.off;
}

hipError_t table_rules_launch(const TableParams& p, void* workspace, size_t ws_bytes, hipStream_t st) {
    const int B = p.B, H = p.H, W = p.W;
    if (!table_args_ok(B, H, W, p.gap, p.min_len, p.max_rules) || p.max_thick < 0 || !p.rgb || !p.hrules || !p.vrules || !p.counts) return hipErrorInvalidValue;
    Arena a(workspace, ws_bytes);
    const TableWorkspace w = table_layout(a, B, H, W, p.gap, p.min_len, p.max_rules);
    if (a.overflow) return hipErrorOutOfMemory;
    const int nw = (W + 63) / 64, nhw = (H + 63) / 64;
    const unsigned long long* hmask;
    hipError_t e = hipMemsetAsync(p.counts, 0, sizeof(int) * 2 * (size_t)B, st);
    if (e != hipSuccess) return e;
    if ((e = ink_mask_resolve(p.rgb, p.hmask_in, p.hmask_out, w.hmask, B, H, W, p.threshold, st, &hmask)) != hipSuccess) return e;
    if ((e = ink_transpose_launch(hmask, w.vmask, B, H, W, st)) != hipSuccess) return e;
    TDirs D;
    D.B = B;
    for (int k = 0; k < 2; ++k) {
        TDir& d = D.d[k];
        d.mask = k ? w.vmask : hmask;
        d.R = k ? W : H; d.C = k ? H : W; d.nw = k ? nhw : nw; d.cap = table_cap(d.C, p.gap, p.min_len);
        d.runs = w.runs[k]; d.parent = w.parent[k]; d.stat = w.stat[k]; d.nrun = w.nrun[k];
    }
    const dim3 glines((unsigned)(((long long)B * (H + W) + 255) / 256));
    hipLaunchKernelGGL(tb_fill_kernel, glines, dim3(256), 0, st, D, p.gap, p.min_len);
    hipLaunchKernelGGL(tb_merge_kernel, glines, dim3(256), 0, st, D);
    hipLaunchKernelGGL(tb_accum_kernel, glines, dim3(256), 0, st, D);
    hipLaunchKernelGGL(tb_select_kernel, glines, dim3(256), 0, st, D, p.min_len, p.max_thick, p.max_rules, p.counts, w.tmp);
    hipLaunchKernelGGL(tb_sort_kernel, dim3(2 * B), dim3(256), 0, st, p.counts, w.tmp, p.hrules, p.vrules, p.max_rules);
    return hipGetLastError();
}
