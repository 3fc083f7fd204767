// Page orientation on the GPU (gfx950): is a page sideways, pages turned by quarter turns, the per-page vote of the line classifier.
// Everything is integer and every reduction is an order-free add, so the results equal the sequential definition restated in
// tests/page_orient_reference.py.
//
// Sideways or not (quarter_launch), all stream-ordered, no host round trip:
//   1 ink_mask / ink_transpose (runs.hip)   ink = L < threshold packed along x, and the same mask with x and y exchanged: the page
//                    bytes are read once, everything after works on 1/24 of them
//   2 or_profile     ink count of every row (mask) and every column (transposed mask): 16 lanes per line, popcounts of its words
//   3 or_energy      E = sum of (p[i + 1] - p[i])^2 per (page, direction) in 64 bits: wave sums, one atomic per wave
//   4 or_flags       sideways = E_c > ratio * E_r
// Turning (page_turn_launch): t = 0 / 2 keep the lines of a page, one thread per pixel; t = 1 / 3 exchange x and y: a 64 x 64 pixel
// tile goes through LDS so that the reads and the writes are both whole 192-byte pieces of a line.
#include "orient.h"
#include "runs.h"

namespace {

typedef unsigned long long u64;

// 2: prof = [B][H] row counts, then [B][W] column counts
__global__ __launch_bounds__(256) void or_profile_kernel(const u64* hmask, const u64* vmask, int* prof, int B, int H, int W, int nw, int nhw) {
    const long long line = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
    const int sub = threadIdx.x & 15;
    const long long nh = (long long)B * H, total = nh + (long long)B * W;
    const bool valid = line < total;
    int c = 0;
    if (valid) {
        const bool col = line >= nh;
        const int n = col ? nhw : nw;
        const u64* m = col ? vmask + (size_t)(line - nh) * nhw : hmask + (size_t)line * nw;
        for (int i = sub; i < n; i += 16) c += __popcll(m[i]);
    }
#pragma unroll
    for (int d = 8; d >= 1; d >>= 1) c += __shfl_xor(c, d);
    if (valid && sub == 0) prof[line] = c;
}

// 3: blockIdx.y = page * 2 + direction
__global__ __launch_bounds__(256) void or_energy_kernel(const int* prof, u64* energies, int B, int H, int W) {
    const int pg = blockIdx.y >> 1, dir = blockIdx.y & 1;
    const int R = dir ? W : H;
    if ((long long)blockIdx.x * 256 >= R - 1) return;
    const int* p = prof + (dir ? (size_t)B * H + (size_t)pg * W : (size_t)pg * H);
    const int i = blockIdx.x * 256 + threadIdx.x;
    u64 e = 0;
    if (i + 1 < R) {
        const long long d = (long long)p[i + 1] - p[i];
        e = (u64)(d * d);
    }
    unsigned lo = (unsigned)e, hi = (unsigned)(e >> 32);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const u64 o = ((u64)(unsigned)__shfl_xor((int)hi, d) << 32) | (unsigned)__shfl_xor((int)lo, d);
        e += o;
        lo = (unsigned)e; hi = (unsigned)(e >> 32);
    }
    if ((threadIdx.x & 63) == 0 && e) atomicAdd(&energies[(size_t)pg * 2 + dir], e);
}

// 4
__global__ __launch_bounds__(256) void or_flags_kernel(const u64* energies, int* sideways, int B, int ratio) {
    const int pg = blockIdx.x * 256 + threadIdx.x;
    if (pg >= B) return;
    sideways[pg] = energies[(size_t)pg * 2 + 1] > (u64)ratio * energies[(size_t)pg * 2] ? 1 : 0;
}

// t = 0 / 2: out (y, x) <- in (y, x) or in (H - 1 - y, W - 1 - x); a wave writes 192 consecutive bytes and reads 192 consecutive bytes
__global__ __launch_bounds__(256) void pt_straight_kernel(const uint8_t* pages, int n, int H, int W, const int* idx, int t, uint8_t* out) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int src = idx[blockIdx.z];
    if (x >= W || y >= H || src < 0 || src >= n) return;
    const int sy = t ? H - 1 - y : y, sx = t ? W - 1 - x : x;
    const uint8_t* s = pages + (((size_t)src * H + sy) * W + sx) * 3;
    uint8_t* d = out + (((size_t)blockIdx.z * H + y) * W + x) * 3;
    d[0] = s[0]; d[1] = s[1]; d[2] = s[2];
}

// t = 1 / 3: out is [W][H].  t = 1: in (y, x) -> out (W - 1 - x, y); t = 3: in (y, x) -> out (x, H - 1 - y).  The block's input tile is
// rows y0 .. y0 + 63, columns x0 .. x0 + 63; in LDS a tile row is 196 bytes (49 words: the column walk of the write phase changes bank
// with every row).  Both phases run over the tile's 64 x 192 bytes with consecutive threads on consecutive bytes of a line.
constexpr int PT_TILE = 64, PT_ROWB = PT_TILE * 3, PT_PITCH = PT_ROWB + 4;
__global__ __launch_bounds__(256) void pt_quarter_kernel(const uint8_t* pages, int n, int H, int W, const int* idx, int t, uint8_t* out) {
    __shared__ uint8_t tile[PT_TILE * PT_PITCH];
    const int src = idx[blockIdx.z];
    if (src < 0 || src >= n) return;
    const int x0 = blockIdx.x * PT_TILE, y0 = blockIdx.y * PT_TILE;
    const uint8_t* in = pages + (size_t)src * H * W * 3;
    for (int e = threadIdx.x; e < PT_TILE * PT_ROWB; e += 256) {
        const int r = e / PT_ROWB, b = e - r * PT_ROWB;
        if (y0 + r < H && x0 + b / 3 < W) tile[r * PT_PITCH + b] = in[((size_t)(y0 + r) * W + x0) * 3 + b];
    }
    __syncthreads();
    uint8_t* o = out + (size_t)blockIdx.z * H * W * 3;
    const int jbase = t == 1 ? y0 : H - PT_TILE - y0;   // first output column of the tile (t = 3: may lie left of the page)
    for (int e = threadIdx.x; e < PT_TILE * PT_ROWB; e += 256) {
        const int a = e / PT_ROWB, ob = e - a * PT_ROWB;   // a: the tile's input column = one output line
        const int q = ob / 3, ch = ob - q * 3;
        const int r = t == 1 ? q : PT_TILE - 1 - q;        // the tile's input row
        const int j = jbase + q;
        if (x0 + a >= W || y0 + r >= H || j < 0) continue;
        const int i = t == 1 ? W - 1 - (x0 + a) : x0 + a;
        o[((size_t)i * H + j) * 3 + ch] = tile[r * PT_PITCH + a * 3 + ch];
    }
}

__global__ __launch_bounds__(256) void pv_vote_kernel(const int* flip, const int* page_idx, int n, int B, int* counts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int pg = page_idx[i];
    if (pg < 0 || pg >= B) return;
    atomicAdd(&counts[pg * 2], 1);
    if (flip[i]) atomicAdd(&counts[pg * 2 + 1], 1);
}

}  // namespace

// the workspace's regions: one layout sizes it (quarter_workspace_bytes) and carves it (quarter_launch)
struct QuarterWorkspace { unsigned long long *hmask, *vmask; int* prof; };
static QuarterWorkspace quarter_layout(Arena& a, int B, int H, int W) {
    const size_t nw = (W + 63) / 64, nhw = (H + 63) / 64;
    QuarterWorkspace w;
    w.hmask = a.take<unsigned long long>((size_t)B * H * nw);
    w.vmask = a.take<unsigned long long>((size_t)B * W * nhw);
    w.prof = a.take<int>((size_t)B * ((size_t)H + W));
    return w;
}

static bool quarter_args_ok(int B, int H, int W) {
    if (B <= 0 || B > 32767 || H <= 0 || W <= 0 || H > 65535 || W > 65535) return false;
    return (size_t)B * ((size_t)H + W) < (1ull << 31);
}

size_t quarter_workspace_bytes(int B, int H, int W) {
    if (!quarter_args_ok(B, H, W)) return 0;
    Arena a;
    quarter_layout(a, B, H, W);
    return a.off;
}

hipError_t quarter_launch(const QuarterParams& p, void* workspace, size_t ws_bytes, hipStream_t st) {
    const int B = p.B, H = p.H, W = p.W;
    if (!quarter_args_ok(B, H, W) || p.ratio < 1 || p.ratio > QUARTER_MAX_RATIO || !p.rgb || !p.energies || !p.sideways) return hipErrorInvalidValue;
    Arena a(workspace, ws_bytes);
    const QuarterWorkspace w = quarter_layout(a, B, H, W);
    if (a.overflow) return hipErrorOutOfMemory;
    const int nw = (W + 63) / 64, nhw = (H + 63) / 64;
    u64* energies = reinterpret_cast<u64*>(p.energies);
    hipError_t e = hipMemsetAsync(p.energies, 0, sizeof(long long) * 2 * (size_t)B, st);
    if (e != hipSuccess) return e;
    if ((e = ink_mask_launch(p.rgb, w.hmask, B, H, W, p.threshold, st)) != hipSuccess) return e;
    if ((e = ink_transpose_launch(w.hmask, w.vmask, B, H, W, st)) != hipSuccess) return e;
    const long long lines = (long long)B * ((long long)H + W);
    hipLaunchKernelGGL(or_profile_kernel, dim3((unsigned)((lines + 15) / 16)), dim3(256), 0, st, w.hmask, w.vmask, w.prof, B, H, W, nw, nhw);
    const int longest = H > W ? H : W;
    if (longest > 1)
        hipLaunchKernelGGL(or_energy_kernel, dim3((unsigned)((longest - 1 + 255) / 256), (unsigned)(2 * B)), dim3(256), 0, st, w.prof, energies, B, H, W);
    hipLaunchKernelGGL(or_flags_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, energies, p.sideways, B, p.ratio);
    return hipGetLastError();
}

hipError_t page_turn_launch(const uint8_t* pages, int n, int H, int W, const int* idx, int m, int t, uint8_t* out, hipStream_t st) {
    if (!pages || !idx || !out || n <= 0 || m <= 0 || m > 65535 || H <= 0 || W <= 0 || H > 65535 || W > 65535 || t < 0 || t > 3 || pages == out)
        return hipErrorInvalidValue;
    if (t & 1)
        hipLaunchKernelGGL(pt_quarter_kernel, dim3((W + PT_TILE - 1) / PT_TILE, (H + PT_TILE - 1) / PT_TILE, m), dim3(256), 0, st, pages, n, H, W, idx, t, out);
    else
        hipLaunchKernelGGL(pt_straight_kernel, dim3((W + 63) / 64, (H + 3) / 4, m), dim3(256), 0, st, pages, n, H, W, idx, t, out);
    return hipGetLastError();
}

hipError_t page_vote_launch(const int* flip, const int* page_idx, int n, int B, int* counts, hipStream_t st) {
    if (!counts || B <= 0 || n < 0 || (n > 0 && (!flip || !page_idx))) return hipErrorInvalidValue;
    const hipError_t e = hipMemsetAsync(counts, 0, sizeof(int) * 2 * (size_t)B, st);
    if (e != hipSuccess || n == 0) return e;
    hipLaunchKernelGGL(pv_vote_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, flip, page_idx, n, B, counts);
    return hipGetLastError();
}
