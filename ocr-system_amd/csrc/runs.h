#pragma once
#include "common.h"

// What the page-analysis passes share (DB post-process, de-skew, tables, selection marks, matrix codes, page orientation): the lock-free
// union-find, the ink mask of a page and its bit transpose, the run list of a batch of row masks with its 8-connected merge, the
// components of all ink built from them (Components, at the end), and a rank sort of a few integer key columns in LDS.  Device helpers are defined here; the kernels live in runs.hip behind the host
// launchers below (every kernel of the library sits in the anonymous namespace of its own file).

// ---- min-label union-find (parents only ever decrease: the root of a set is its smallest index); on LDS tiles and on pages ----
__device__ __forceinline__ int uf_find(const int* L, int i) {
    int p = L[i];
    while (p != i) { i = p; p = L[i]; }
    return i;
}
__device__ __forceinline__ void uf_union(int* L, int a, int b) {
    bool done = false;
    while (!done) {
        a = uf_find(L, a); b = uf_find(L, b);
        if (a < b) { const int old = atomicMin(&L[b], a); done = (old == b); b = old; }
        else if (b < a) { const int old = atomicMin(&L[a], b); done = (old == a); a = old; }
        else done = true;
    }
}

// ---- one wave per (page, row), four rows per work-group (256 threads): false when the wave has no row ----
__device__ __forceinline__ bool row_wave(int H, int rows_total, int& pg, int& row, int& lane) {
    const int wrow = blockIdx.x * 4 + (threadIdx.x >> 6);
    lane = threadIdx.x & 63;
    if (wrow >= rows_total) return false;
    row = wrow % H; pg = wrow / H;
    return true;
}
inline dim3 row_wave_grid(int rows_total) { return dim3(((unsigned)rows_total + 3u) / 4u); }

// bits of mask word m that start a run: ink whose left neighbour (prev = bit 63 of the word to the left) is not ink
__device__ __forceinline__ unsigned long long run_starts(unsigned long long m, unsigned long long prev) { return m & ~((m << 1) | prev); }

// ---- after run_merge: run id (of `row`, [xs, xe] read here) learns its root -> the root, or -1 when the run is a root itself.  Its parent
// is compressed to the root (concurrent compressions only ever replace a parent by an ancestor) and the root's box (x0, x1, y0, y1)
// grows over the run.  The box only ever moves one way, so a value read before the atomic that already covers this run makes the atomic
// unnecessary (most runs of a component lie inside what earlier ones reported).  P, rxs, rxe, box are the page's. ----
__device__ __forceinline__ int run_join_root(int* P, const unsigned short* rxs, const unsigned short* rxe, int4* box, int id, int row, int& xs, int& xe) {
    const int p = P[id];
    if (p == id) return -1;
    const int root = uf_find(P, p);
    if (root != p) P[id] = root;
    xs = rxs[id]; xe = rxe[id];
    int* b = reinterpret_cast<int*>(box + root);
    if (xs < __atomic_load_n(b + 0, __ATOMIC_RELAXED)) atomicMin(b + 0, xs);
    if (xe > __atomic_load_n(b + 1, __ATOMIC_RELAXED)) atomicMax(b + 1, xe);
    if (row > __atomic_load_n(b + 3, __ATOMIC_RELAXED)) atomicMax(b + 3, row);
    return root;
}

// ---- the four diagonal extremes of one run (min x + y, max x - y, max x + y, min x - y) as packed words (key, y, x): min types hold y,
// max types 65535 - y below the key, so that one atomic min / max keeps the tie rule (the smaller y) exact ----
__device__ __forceinline__ void run_extremes(int xs, int xe, int y, unsigned long long (&e)[4]) {
    typedef unsigned long long u64;
    e[0] = ((u64)(unsigned)(xs + y) << 32) | ((u64)y << 16) | (u64)xs;
    e[1] = ((u64)(unsigned)(xe - y + 65536) << 32) | ((u64)(65535 - y) << 16) | (u64)xe;
    e[2] = ((u64)(unsigned)(xe + y) << 32) | ((u64)(65535 - y) << 16) | (u64)xe;
    e[3] = ((u64)(unsigned)(xs - y + 65536) << 32) | ((u64)y << 16) | (u64)xs;
}

// ---- rank sort of n <= cap rows of NC integer key columns, by one 256-thread work-group: the keys (the first NC of every `stride`
// ints of t) go to LDS (s_key, NC * cap ints), every row is ranked lexicographically against all others, and emit(i, rank, key)
// writes it out.  Rows are distinct (the last column is an id), so ranks are. ----
template <int NC, class Emit>
__device__ __forceinline__ void rank_sort(int* s_key, const int* t, int stride, int n, Emit emit) {
    const int tid = threadIdx.x;
    for (int i = tid; i < n * NC; i += 256) s_key[i] = t[(i / NC) * stride + i % NC];
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
        int k[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) k[c] = s_key[i * NC + c];
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            bool less = false, decided = false;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const int v = s_key[j * NC + c];
                if (!decided && v != k[c]) { less = v < k[c]; decided = true; }
            }
            rank += less ? 1 : 0;
        }
        emit(i, rank, k);
    }
}

// ---- ink mask ----
// ink = L < threshold (L = Pillow's convert('L')) packed into 64-bit words along x: [B][H][ceil(W / 64)], bit x % 64 of word x / 64
hipError_t ink_mask_launch(const uint8_t* rgb, unsigned long long* mask, int B, int H, int W, int threshold, hipStream_t st);
// the mask with x and y exchanged, [B][W][ceil(H / 64)]
hipError_t ink_transpose_launch(const unsigned long long* hmask, unsigned long long* vmask, int B, int H, int W, hipStream_t st);
// the mask a pass works on, returned in *mask: mask_in when given (copied to the parity hook mask_out when that is asked for too),
// otherwise computed here into mask_out or, without a hook, into scratch
hipError_t ink_mask_resolve(const uint8_t* rgb, const unsigned long long* mask_in, unsigned long long* mask_out, unsigned long long* scratch,
                            int B, int H, int W, int threshold, hipStream_t st, const unsigned long long** mask);

// ---- run list of a batch of row masks ([B][H][nw] words), page by page in raster order.  B * H < 2^31 and run_cap < 2^31 are the
// caller's to check; runoff is [B][H + 1], rxs / rxe / parent / box are [B][runcap]. ----
// worst case of a page: every other pixel of every row starts a run
inline size_t run_cap(int H, int W) { return (size_t)H * ((W + 1) / 2); }
// runs per row -> runcnt[pg][row] (for a mask that is already there; the DB post-process counts while it thresholds)
void run_count_launch(const unsigned long long* mask, int* runcnt, int B, int H, int nw, hipStream_t st);
// exclusive scan of every page's H row counts: cnt[pg][r] -> offset of row r, cnt[pg][H] = total (also -> total_out[pg] when given)
void row_scan_launch(int* cnt, int* total_out, int B, int H, hipStream_t st);
// masks -> runs [xs, xe] at the row's offset; a run is its own union-find parent and, when box is given, its own box (x0, x1, y0, y1)
void run_fill_launch(const unsigned long long* mask, const int* runoff, unsigned short* rxs, unsigned short* rxe, int* parent, int4* box, int B,
                     int H, int nw, size_t runcap, hipStream_t st);
// union-find over run ids: a run joins every run of the row above that it touches (8-connectivity)
void run_merge_launch(const int* runoff, const unsigned short* rxs, const unsigned short* rxe, int* parent, int B, int H, size_t runcap,
                      hipStream_t st);

// ---- the components of all ink of a batch of pages: what the matrix-code readers and the selection marks open with.  The regions come
// first in a pass's workspace, in this order; a pass's own regions follow.  After components_launch every run's parent is its root (the
// component's first run in raster order) and a root holds its component's box (x0, x1, y0, y1), its ink when there is an area region,
// and its four packed diagonal extremes (run_extremes) when the caller has set ext to a region of [B][runcap][4] words. ----
struct Components {
    const unsigned long long* mask;   // the mask in use, set by components_launch: the caller's mask_in, its mask_out, or mask_buf
    unsigned long long* mask_buf;     // [B][H][ceil(W / 64)]
    int* runoff;                      // [B][H + 1]: run counts -> offsets
    unsigned short *rxs, *rxe;        // [B][runcap]
    int* parent;                      // [B][runcap]
    int4* box;                        // [B][runcap]
    int* area;                        // [B][runcap], or nullptr
    unsigned long long* ext;          // the caller's, or nullptr (needs the area)
};
Components components_layout(Arena& a, int B, int H, int W, bool area);
// sides 1 .. 65535 (run ends are 16-bit), B * H and the run capacity below 2^31
bool page_args_ok(int B, int H, int W);
// ink_mask_resolve, run_count, row_scan, run_fill, run_merge, then (with an area) every run's own area and extremes, then the
// accumulation at the roots
hipError_t components_launch(Components& c, const uint8_t* rgb, const unsigned long long* mask_in, unsigned long long* mask_out, int B, int H, int W,
                             int threshold, hipStream_t st);
