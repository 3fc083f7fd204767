// Bandwidth-bound helper kernels (NHWC bf16), the LSTM recurrence and the CTC tail for gfx950.
// No reference counterpart exists; semantics are defined by oracle/nets.py.
#include "ops.h"
#include "../../include/lumina_ocr.h"   // LUMINA_MAX_WORDS

#include <type_traits>

#include <cstdlib>

namespace {

__device__ __forceinline__ void unpack8(const uint4 v, float* f) {
    f[0] = __uint_as_float(v.x << 16); f[1] = __uint_as_float(v.x & 0xFFFF0000u);
    f[2] = __uint_as_float(v.y << 16); f[3] = __uint_as_float(v.y & 0xFFFF0000u);
    f[4] = __uint_as_float(v.z << 16); f[5] = __uint_as_float(v.z & 0xFFFF0000u);
    f[6] = __uint_as_float(v.w << 16); f[7] = __uint_as_float(v.w & 0xFFFF0000u);
}
__device__ __forceinline__ uint4 pack8(const float* f) {
    uint4 v;
    v.x = pack_bf16x2(f[0], f[1]); v.y = pack_bf16x2(f[2], f[3]);
    v.z = pack_bf16x2(f[4], f[5]); v.w = pack_bf16x2(f[6], f[7]);
    return v;
}

// ------------------------------------------------------------------ max pool
__global__ void maxpool_kernel(const bf16_t* x, bf16_t* y, int N, int H, int W, int C, int k, int s, int pad, int Ho, int Wo) {
    const int cg = C >> 3;
    const size_t total = (size_t)N * Ho * Wo * cg;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c8 = (int)(i % cg);
        size_t t = i / cg;
        const int ox = (int)(t % Wo); t /= Wo;
        const int oy = (int)(t % Ho);
        const int n = (int)(t / Ho);
        float m[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) m[j] = -3.0e38f;
        for (int dy = 0; dy < k; ++dy) {
            const int iy = oy * s - pad + dy;
            if (iy < 0 || iy >= H) continue;
            for (int dx = 0; dx < k; ++dx) {
                const int ix = ox * s - pad + dx;
                if (ix < 0 || ix >= W) continue;
                float f[8];
                unpack8(*reinterpret_cast<const uint4*>(x + (((size_t)n * H + iy) * W + ix) * C + c8 * 8), f);
#pragma unroll
                for (int j = 0; j < 8; ++j) m[j] = fmaxf(m[j], f[j]);
            }
        }
        *reinterpret_cast<uint4*>(y + i * 8) = pack8(m);
    }
}

// ------------------------------------------------------------------ depthwise conv
// One thread = 4 consecutive output pixels x 8 channels: per kernel row the K+3 input vectors are loaded once (branch-free:
// clamped address + select; a guarded load per tap serialises one memory latency per tap) and re-used by the 4 sliding
// windows; fp32 FMA accumulation in tap order (kh, kw).  The layer's weights and bias are converted to fp32 once per
// workgroup and live in LDS ([tap][half][C/8][4] floats: a tap is two conflict-free ds_read_b128 across lanes), the
// activation is a template parameter, index arithmetic is 32-bit.  VALU-bound (PMC: VALU busy ~75 % of the kernel time,
// ~2.3 k vector instructions per wave for 4 x 8 outputs x K*K taps).
template <int K, int ACT>
__global__ __launch_bounds__(256) void dwconv_kernel(const bf16_t* x, const bf16_t* w, const float* bias, bf16_t* y, int N, int H, int W, int C,
                                                     int sh, int Ho) {
    constexpr int PAD = K / 2, XG = 4;
    extern __shared__ float wl[];  // [K*K][2][cg][4] weights, then bias [C]
    const int cg = C >> 3, wg = (W + XG - 1) / XG;
    for (int i = threadIdx.x; i < K * K * C; i += 256) {
        const int tap = i / C, c = i - tap * C;
        wl[((tap * 2 + ((c >> 2) & 1)) * cg + (c >> 3)) * 4 + (c & 3)] = bf16_to_f32(w[i]);
    }
    float* bl = wl + K * K * C;
    for (int i = threadIdx.x; i < C; i += 256) bl[i] = bias[i];
    __syncthreads();
    const unsigned total = (unsigned)N * Ho * wg * cg;  // < 2^31 (checked by the launcher)
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
        const int c8 = (int)(i % (unsigned)cg);
        unsigned t = i / (unsigned)cg;
        const int xg = (int)(t % (unsigned)wg); t /= (unsigned)wg;
        const int oy = (int)(t % (unsigned)Ho);
        const int n = (int)(t / (unsigned)Ho);
        const int ox0 = xg * XG;
        float a[XG][8];
#pragma unroll
        for (int o = 0; o < XG; ++o)
#pragma unroll
            for (int j = 0; j < 8; ++j) a[o][j] = 0.f;
#pragma unroll
        for (int kh = 0; kh < K; ++kh) {
            const int iy = oy * sh - PAD + kh;
            if (iy < 0 || iy >= H) continue;
            float in[K + XG - 1][8];
            const bf16_t* row = x + ((size_t)(n * H + iy) * W) * C + c8 * 8;
#pragma unroll
            for (int j = 0; j < K + XG - 1; ++j) {
                const int ix = ox0 - PAD + j;
                const int ixc = ix < 0 ? 0 : (ix >= W ? W - 1 : ix);
                uint4 v = *reinterpret_cast<const uint4*>(row + ixc * C);
                if (ix != ixc) v = make_uint4(0, 0, 0, 0);
                unpack8(v, in[j]);
            }
#pragma unroll
            for (int kw = 0; kw < K; ++kw) {
                const float4 g0 = *reinterpret_cast<const float4*>(wl + (((kh * K + kw) * 2 + 0) * cg + c8) * 4);
                const float4 g1 = *reinterpret_cast<const float4*>(wl + (((kh * K + kw) * 2 + 1) * cg + c8) * 4);
                const float g[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
#pragma unroll
                for (int o = 0; o < XG; ++o)
#pragma unroll
                    for (int j = 0; j < 8; ++j) a[o][j] = __builtin_fmaf(in[o + kw][j], g[j], a[o][j]);
            }
        }
        float bb[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) bb[j] = bl[c8 * 8 + j];
        bf16_t* yrow = y + ((size_t)(n * Ho + oy) * W + ox0) * C + c8 * 8;
#pragma unroll
        for (int o = 0; o < XG; ++o) {
            if (ox0 + o >= W) break;
#pragma unroll
            for (int j = 0; j < 8; ++j) a[o][j] = apply_act(a[o][j] + bb[j], ACT);
            *reinterpret_cast<uint4*>(yrow + o * C) = pack8(a[o]);
        }
    }
}

// ------------------------------------------------------------------ squeeze-excite gate from the pooled sums (one block per crop)
// pool [N][strips][C]: per-strip sums of the depthwise output, written by the fused expand + depthwise kernel's epilogue (mbconv.hip) or by
// se_pool_kernel — the tensor itself is not read again (the nine full passes over it per recogniser forward were 0.9 ms of a 64-page step).
__global__ __launch_bounds__(256) void se_fc_kernel(const float* pool, int strips, const bf16_t* w1, const float* b1, const bf16_t* w2,
                                                    const float* b2, bf16_t* gate, int HW, int C, int mid) {
    extern __shared__ float sm[];  // mean[C], hid[mid]
    const int n = blockIdx.x, tid = threadIdx.x;
    float* mean = sm;
    float* hid = mean + C;
    for (int c = tid; c < C; c += 256) {
        float s = 0.f;
        for (int g = 0; g < strips; ++g) s += pool[((size_t)n * strips + g) * C + c];
        mean[c] = bf16_to_f32(f32_to_bf16(s / (float)HW));
    }
    __syncthreads();
    for (int m = tid; m < mid; m += 256) {
        float s = 0.f;
        for (int c = 0; c < C; ++c) s = s + bf16_to_f32(w1[(size_t)m * C + c]) * mean[c];
        hid[m] = bf16_to_f32(f32_to_bf16(fmaxf(s + b1[m], 0.f)));
    }
    __syncthreads();
    for (int c = tid; c < C; c += 256) {
        float s = 0.f;
        for (int m = 0; m < mid; ++m) s = s + bf16_to_f32(w2[(size_t)c * mid + m]) * hid[m];
        gate[(size_t)n * C + c] = f32_to_bf16(apply_act(s + b2[c], ACT_HSIGMOID));
    }
}

__global__ void se_scale_kernel(const bf16_t* x, const bf16_t* gate, bf16_t* y, int N, int HW, int C) {
    const int cg = C >> 3;
    const size_t total = (size_t)N * HW * cg;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c8 = (int)(i % cg);
        const int n = (int)(i / ((size_t)HW * cg));
        float f[8], g[8];
        unpack8(*reinterpret_cast<const uint4*>(x + i * 8), f);
        unpack8(*reinterpret_cast<const uint4*>(gate + (size_t)n * C + c8 * 8), g);
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = f[j] * g[j];
        *reinterpret_cast<uint4*>(y + i * 8) = pack8(f);
    }
}

// ------------------------------------------------------------------ LSTM recurrence on the matrix cores
// The three-wave kernel (option lstm_waves = 3, kept for comparison).  One workgroup = 32 sequences x one direction, 3 waves; wave u owns hidden units [32u, 32u+32).  Per time step
//   gates[4][32 units][32 seqs] = W_hh (A operand, resident in registers for all 80 steps) * h_{t-1} (B operand, LDS)
// with the accumulators initialised from the stored x-projection.  The four gate tiles of a (unit, sequence) pair
// land in the same lane / register slot, so the cell update is register-local; h_t goes to LDS (next step's operand)
// and to HBM (layer output) as packed 8-byte quads.  c stays fp32 in registers, h is bf16 (oracle/nets.py lstm_dir).
constexpr int LH = 96, LSEQ = 32, LPITCH = 208;  // bytes per sequence row of the h buffer (192 + 16: conflict-free b128 reads)

__device__ __forceinline__ float fast_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-1.4426950408889634f * x)); }
__device__ __forceinline__ float fast_tanh(float x) { return 2.f * fast_sigmoid(2.f * x) - 1.f; }

__global__ __launch_bounds__(192) void lstm3_kernel(const bf16_t* xproj, const bf16_t* whh, bf16_t* out, int N, int T) {
    __shared__ __attribute__((aligned(16))) unsigned char hbuf[2][LSEQ * LPITCH];
    const int tid = threadIdx.x, lane = tid & 63, u = tid >> 6, r = lane & 31, h = lane >> 5;
    const int dir = blockIdx.x & 1, n0 = (blockIdx.x >> 1) * LSEQ;
    const int seq = n0 + r;
    const bool valid = seq < N;
    const int sq = valid ? seq : N - 1;  // clamp loads of the ragged last group
    bf16x8_t afr[4][6];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int ks = 0; ks < 6; ++ks)
            afr[g][ks] = *reinterpret_cast<const bf16x8_t*>(whh + ((size_t)dir * 4 * LH + g * LH + 32 * u + r) * LH + ks * 16 + h * 8);
    for (int i = tid; i < 2 * LSEQ * LPITCH / 16; i += 192) reinterpret_cast<uint4*>(&hbuf[0][0])[i] = make_uint4(0, 0, 0, 0);
    float c[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) c[j] = 0.f;
    const size_t xrow = (size_t)sq * T;
    const int xcol = dir * 4 * LH + 32 * u + 4 * h;
    uint2 xq[4][4];
    {
        const int t = dir ? T - 1 : 0;
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int q = 0; q < 4; ++q) xq[g][q] = *reinterpret_cast<const uint2*>(xproj + (xrow + t) * (8 * LH) + xcol + g * LH + 8 * q);
    }
    __syncthreads();
    int cur = 0;
    for (int step = 0; step < T; ++step) {
        const int t = dir ? (T - 1 - step) : step;
        f32x16_t acc[4];
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                acc[g][4 * q + 0] = __uint_as_float(xq[g][q].x << 16); acc[g][4 * q + 1] = __uint_as_float(xq[g][q].x & 0xFFFF0000u);
                acc[g][4 * q + 2] = __uint_as_float(xq[g][q].y << 16); acc[g][4 * q + 3] = __uint_as_float(xq[g][q].y & 0xFFFF0000u);
            }
        if (step + 1 < T) {  // prefetch the next step's x-projection under this step's MFMAs
            const int tn = dir ? (t - 1) : (t + 1);
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int q = 0; q < 4; ++q) xq[g][q] = *reinterpret_cast<const uint2*>(xproj + (xrow + tn) * (8 * LH) + xcol + g * LH + 8 * q);
        }
#pragma unroll
        for (int ks = 0; ks < 6; ++ks) {
            const bf16x8_t bfr = *reinterpret_cast<const bf16x8_t*>(&hbuf[cur][r * LPITCH + (ks * 16 + h * 8) * 2]);
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(afr[g][ks], bfr, acc[g], 0, 0, 0);
        }
        bf16_t* orow = out + ((size_t)sq * T + t) * (2 * LH) + dir * LH + 32 * u + 4 * h;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float hn[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int j = 4 * q + e;
                const float ig = fast_sigmoid(acc[0][j]), fg = fast_sigmoid(acc[1][j]), gg = fast_tanh(acc[2][j]), og = fast_sigmoid(acc[3][j]);
                c[j] = fg * c[j] + ig * gg;
                hn[e] = og * fast_tanh(c[j]);
            }
            uint2 o;
            o.x = pack_bf16x2(hn[0], hn[1]);
            o.y = pack_bf16x2(hn[2], hn[3]);
            *reinterpret_cast<uint2*>(&hbuf[cur ^ 1][r * LPITCH + (32 * u + 8 * q + 4 * h) * 2]) = o;
            if (valid) *reinterpret_cast<uint2*>(orow + 8 * q) = o;
        }
        __syncthreads();
        cur ^= 1;
    }
}

// The same recurrence on twelve waves (the default).  Wave w owns hidden
// units [8w, 8w+8) and runs ONE 32x32 tile per step whose A rows are ordered row = 8 * gate + unit_local: with the 32x32x16 output
// layout (accumulator entry 4q + e is row 8q + 4h + e) a lane holds gates q = 0..3 of units 8w + 4h + e, e = 0..3, of its sequence, so
// the cell update stays register-local on four (unit, sequence) pairs per lane instead of sixteen.  Six MFMAs per wave and step instead
// of 24 (the same total), and the gate arithmetic (ten transcendentals per pair, the critical path) spreads over all four SIMDs with
// three waves each.  Per element nothing changes: accumulator initialised from the bf16 x-projection, six k steps ascending, the same
// gate expressions, c in fp32, h rounded to bf16.
__global__ __launch_bounds__(768) void lstm_kernel(const bf16_t* xproj, const bf16_t* whh, bf16_t* out, int N, int T) {
    __shared__ __attribute__((aligned(16))) unsigned char hbuf[2][LSEQ * LPITCH];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
    const int dir = blockIdx.x & 1, n0 = (blockIdx.x >> 1) * LSEQ;
    const int seq = n0 + r;
    const bool valid = seq < N;
    const int sq = valid ? seq : N - 1;  // clamp loads of the ragged last group
    bf16x8_t afr[6];   // A row r of this wave's tile: w_hh row gate * 96 + 8w + (r & 7), gate = r >> 3
#pragma unroll
    for (int ks = 0; ks < 6; ++ks)
        afr[ks] = *reinterpret_cast<const bf16x8_t*>(whh + ((size_t)dir * 4 * LH + (r >> 3) * LH + 8 * w + (r & 7)) * LH + ks * 16 + h * 8);
    for (int i = tid; i < 2 * LSEQ * LPITCH / 16; i += 768) reinterpret_cast<uint4*>(&hbuf[0][0])[i] = make_uint4(0, 0, 0, 0);
    float c[4] = {0.f, 0.f, 0.f, 0.f};
    const size_t xrow = (size_t)sq * T;
    const int xcol = dir * 4 * LH + 8 * w + 4 * h;
    uint2 xq[4];
    {
        const int t = dir ? T - 1 : 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) xq[q] = *reinterpret_cast<const uint2*>(xproj + (xrow + t) * (8 * LH) + xcol + q * LH);
    }
    __syncthreads();
    int cur = 0;
    for (int step = 0; step < T; ++step) {
        const int t = dir ? (T - 1 - step) : step;
        f32x16_t acc;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            acc[4 * q + 0] = __uint_as_float(xq[q].x << 16); acc[4 * q + 1] = __uint_as_float(xq[q].x & 0xFFFF0000u);
            acc[4 * q + 2] = __uint_as_float(xq[q].y << 16); acc[4 * q + 3] = __uint_as_float(xq[q].y & 0xFFFF0000u);
        }
        if (step + 1 < T) {  // prefetch the next step's x-projection under this step's MFMAs
            const int tn = dir ? (t - 1) : (t + 1);
#pragma unroll
            for (int q = 0; q < 4; ++q) xq[q] = *reinterpret_cast<const uint2*>(xproj + (xrow + tn) * (8 * LH) + xcol + q * LH);
        }
#pragma unroll
        for (int ks = 0; ks < 6; ++ks) {
            const bf16x8_t bfr = *reinterpret_cast<const bf16x8_t*>(&hbuf[cur][r * LPITCH + (ks * 16 + h * 8) * 2]);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(afr[ks], bfr, acc, 0, 0, 0);
        }
        float hn[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float ig = fast_sigmoid(acc[e]), fg = fast_sigmoid(acc[4 + e]), gg = fast_tanh(acc[8 + e]), og = fast_sigmoid(acc[12 + e]);
            c[e] = fg * c[e] + ig * gg;
            hn[e] = og * fast_tanh(c[e]);
        }
        uint2 o;
        o.x = pack_bf16x2(hn[0], hn[1]);
        o.y = pack_bf16x2(hn[2], hn[3]);
        *reinterpret_cast<uint2*>(&hbuf[cur ^ 1][r * LPITCH + (8 * w + 4 * h) * 2]) = o;
        if (valid) *reinterpret_cast<uint2*>(out + ((size_t)sq * T + t) * (2 * LH) + dir * LH + 8 * w + 4 * h) = o;
        __syncthreads();
        cur ^= 1;
    }
}

// ------------------------------------------------------------------ CTC head: fused FC + argmax + softmax-max
// A-stationary MFMA GEMM for K = 192 (both recognisers).  A wave keeps its 32 sequence rows in registers (12 fragments) for the whole
// launch; the 64-class weight tiles stream through two LDS buffers (LDS-DMA), their 64 biases through a ring of four slots, both one
// tile ahead, so one barrier per tile is enough.  Two accumulator sets: while the MFMAs of tile t fill one, the soft-max
// and arg-max work of tile t - 1 reads the other (the vector instructions issue in the MFMAs' shadow).  The running (max, argmax,
// sum-exp) stay in registers, the [M, C] logits never exist in memory.
// What defines the bits: logit = K sum + bias in fp32; exp2((v - tm) * log2e) as a subtraction, then a multiplication; the tile's sum
// over (nt, j) ascending, then the partner half-wave's; the two rescale forms of the running sum.  The maximum is exact in any order,
// so it is taken with max3 and the class index is derived only when a tile's maximum beats the running one.
constexpr int CT_NT = 2;                                   // per wave: 32 rows x CT_NT x 32 classes per weight tile
constexpr int CT_ROWS = 4 * 32, CT_BN = 32 * CT_NT, CT_K = 192, CT_KSTEPS = CT_K / 16;
constexpr int CT_W_ITEMS = CT_BN * (CT_K / 8);             // 16-byte items of a weight tile: 1536 = 6 per thread, no remainder
constexpr int CT_WIT = CT_W_ITEMS / 256, CT_WBYTES = CT_W_ITEMS * 16;
constexpr int CT_BIAS_SLOTS = 4;                           // tile t + 1 is written while t - 1 (epilogue) and t are still read
constexpr size_t CT_LDS = 2 * (size_t)CT_WBYTES;          // dynamic; + 1 KB of bias slots (static) = 50 176 B: two work-groups per CU
static_assert(CT_W_ITEMS % 256 == 0 && CT_BN * sizeof(float) / 16 <= 64, "the staging below has no remainder loop");

typedef _Float16 ctc_f16x8_t __attribute__((ext_vector_type(8)));
template <int DT>   // storage type of the sequence and the weights: 0 bf16, 1 fp16 (SVTR fp16 mode)
__global__ __launch_bounds__(256, 2) void ctc_fc_argmax_kernel(const CtcFcParams p) {
    typedef typename std::conditional<DT == 1, ctc_f16x8_t, bf16x8_t>::type frag_t;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // the bias ring is an LDS object of its own: the compiler then knows that the weight DMA cannot write what the epilogue reads
    __shared__ __attribute__((aligned(16))) float sB[CT_BIAS_SLOTS * CT_BN];
    unsigned char* sW = smem;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int row0 = blockIdx.x * CT_ROWS;
    const int last = p.ntiles - 1;
    constexpr float LOG2E = 1.4426950408889634f;

    // this lane's part of its row: the B operand of every K step (rows past M are zero and are not written at the end)
    frag_t arow[CT_KSTEPS];
    {
        const int row = row0 + wave * 32 + r;
        const frag_t* src = reinterpret_cast<const frag_t*>(p.seq + (size_t)row * CT_K) + h;
#pragma unroll
        for (int kc = 0; kc < CT_KSTEPS; ++kc) {
            frag_t v = {};
            if (row < p.M) v = src[2 * kc];
            arow[kc] = v;
        }
    }

    // weight tile `tile` -> LDS buffer slot & 1 by LDS-DMA (no register round trip): six 1 KB pieces per wave, lane-linear, which is
    // the packed tile's own order.  Its 64 biases travel through a register of 16 lanes into bias slot slot & 3 (landed): a DMA
    // into a slot the compiler cannot tell from the one the epilogue reads would put a vmcnt(0) in front of that read.  No guards:
    // 1536 items are 6 x 256, and a request past the last tile repeats the last tile into a buffer nobody reads any more.
    uint4 breg = make_uint4(0, 0, 0, 0);
    auto stage = [&](int tile, int slot) {
        const uint4* src = reinterpret_cast<const uint4*>(p.wpk) + (size_t)tile * CT_W_ITEMS + tid;
        unsigned char* dst = sW + (slot & 1) * CT_WBYTES + (tid - lane) * 16;
#pragma unroll
        for (int it = 0; it < CT_WIT; ++it)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + 256 * it),
                                             (__attribute__((address_space(3))) void*)(dst + 256 * it * 16), 16, 0, 0);
        if (tid < CT_BN / 4) breg = reinterpret_cast<const uint4*>(p.bias + (size_t)tile * CT_BN)[tid];
    };
    // the requests of this wave have landed; the barrier then makes every wave's part visible
    auto landed = [&](int slot) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (tid < CT_BN / 4) reinterpret_cast<uint4*>(sB + (slot & (CT_BIAS_SLOTS - 1)) * CT_BN)[tid] = breg;
        __syncthreads();
    };

    float run_m = -3.0e38f, run_s = 0.f;
    int run_i = 0;

    // tile t: request tile t + 1 into the other buffer, 24 MFMAs from buffer t & 1 (the fragments of K step k + 1 are requested
    // before the MFMAs of step k; the first step's C operand is zero)
    auto mma = [&](f32x16_t (&acc)[CT_NT], int t) {
        stage(min(t + 1, last), t + 1);
        const unsigned char* w = sW + (t & 1) * CT_WBYTES + (h * CT_BN + r) * 16;
        frag_t wf[2][CT_NT];
#pragma unroll
        for (int nt = 0; nt < CT_NT; ++nt) wf[0][nt] = *reinterpret_cast<const frag_t*>(w + nt * 32 * 16);
#pragma unroll
        for (int kc = 0; kc < CT_KSTEPS; ++kc) {
            if (kc + 1 < CT_KSTEPS) {
#pragma unroll
                for (int nt = 0; nt < CT_NT; ++nt)
                    wf[(kc + 1) & 1][nt] = *reinterpret_cast<const frag_t*>(w + (2 * (kc + 1) * CT_BN + nt * 32) * 16);
            }
#pragma unroll
            for (int nt = 0; nt < CT_NT; ++nt) {
                const f32x16_t c = kc == 0 ? f32x16_t{} : acc[nt];
                if constexpr (DT == 1) acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[kc & 1][nt], arow[kc], c, 0, 0, 0);
                else acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[kc & 1][nt], arow[kc], c, 0, 0, 0);
            }
        }
    };
    // tile t's logits (in place), its maximum over this lane's 32 classes and the partner's, its sum of exponentials
    auto tile_sum = [&](f32x16_t (&acc)[CT_NT], int t, float& tm, float& ts) {
        const float* bt = sB + (t & (CT_BIAS_SLOTS - 1)) * CT_BN + 4 * h;
#pragma unroll
        for (int nt = 0; nt < CT_NT; ++nt)
#pragma unroll
            for (int q = 0; q < 4; ++q) {   // classes nt * 32 + 8 * q + 4 * h + (0 .. 3) are accumulator entries 4 * q + (0 .. 3)
                // (read as a fragment and re-typed: hipcc puts s_waitcnt vmcnt(0), a wait for the weight tile just requested, in front
                // of a float4 read of LDS while an LDS-DMA is pending, and none in front of the fragment reads; check the ISA after edits)
                typedef float ctc_f32x4_t __attribute__((ext_vector_type(4)));
                const ctc_f32x4_t b = __builtin_bit_cast(ctc_f32x4_t, *reinterpret_cast<const frag_t*>(bt + nt * 32 + 8 * q));
                acc[nt][4 * q + 0] = acc[nt][4 * q + 0] + b[0]; acc[nt][4 * q + 1] = acc[nt][4 * q + 1] + b[1];
                acc[nt][4 * q + 2] = acc[nt][4 * q + 2] + b[2]; acc[nt][4 * q + 3] = acc[nt][4 * q + 3] + b[3];
            }
        float m = -3.0e38f;
#pragma unroll
        for (int nt = 0; nt < CT_NT; ++nt)
#pragma unroll
            for (int j = 0; j < 16; j += 2) m = __builtin_fmaxf(__builtin_fmaxf(m, acc[nt][j]), acc[nt][j + 1]);
        tm = __builtin_fmaxf(m, __shfl_xor(m, 32));
        float s = 0.f;
#pragma unroll
        for (int nt = 0; nt < CT_NT; ++nt)
#pragma unroll
            for (int j = 0; j < 16; ++j) s += __builtin_amdgcn_exp2f((acc[nt][j] - tm) * LOG2E);
        ts = s + __shfl_xor(s, 32);
    };
    // the running state.  Only a tile whose maximum is strictly above the running one changes the class (an equal one loses to the
    // earlier tile): then the index is the lowest class that holds the maximum, in this lane or its partner (both take this branch
    // together: they hold the same row)
    auto update = [&](const f32x16_t (&acc)[CT_NT], int t, float tm, float ts) {
        if (tm > run_m) {
            int ti = CT_BN;
#pragma unroll
            for (int nt = CT_NT - 1; nt >= 0; --nt)
#pragma unroll
                for (int j = 15; j >= 0; --j)
                    if (acc[nt][j] == tm) ti = nt * 32 + (j & 3) + 8 * (j >> 2) + 4 * h;
            ti = min(ti, __shfl_xor(ti, 32));
            run_s = run_s * __builtin_amdgcn_exp2f((run_m - tm) * LOG2E) + ts;
            run_m = tm;
            run_i = t * CT_BN + ti;
        } else {
            run_s += ts * __builtin_amdgcn_exp2f((tm - run_m) * LOG2E);
        }
    };
    // MFMAs of tile t into accc, beside them the vector work of tile t - 1 on acce; one barrier: after it buffer (t + 1) & 1 and
    // bias slot (t + 1) & 3 are complete, and buffer t & 1 and slot (t - 1) & 3 are free for the requests of step t + 1
    auto step = [&](f32x16_t (&accc)[CT_NT], f32x16_t (&acce)[CT_NT], int t) {
        float tm, ts;
        mma(accc, t);
        tile_sum(acce, t - 1, tm, ts);
        update(acce, t - 1, tm, ts);
        landed(t + 1);
    };

    stage(0, 0);
    landed(0);
    f32x16_t acc0[CT_NT], acc1[CT_NT];
    mma(acc0, 0);            // prologue: tile 0 has no epilogue beside it
    landed(1);
    int t = 1;
    for (; t + 1 < p.ntiles; t += 2) {
        step(acc1, acc0, t);
        step(acc0, acc1, t + 1);
    }
    float tm, ts;
    if (t < p.ntiles) {      // an even number of tiles: one more step, then drain acc1
        step(acc1, acc0, t);
        tile_sum(acc1, t, tm, ts);
        update(acc1, t, tm, ts);
    } else {                 // drain acc0
        tile_sum(acc0, last, tm, ts);
        update(acc0, last, tm, ts);
    }
    if (h == 0) {
        const int row = row0 + wave * 32 + r;
        if (row < p.M) { p.out_idx[row] = run_i; p.out_prob[row] = 1.f / run_s; }
    }
}

// ------------------------------------------------------------------ CTC greedy collapse (one wave per sequence)
// The collapse of one row by one wave: kept classes -> text (-1 padded), kept probabilities -> kept_p (LDS, 128 floats), -> their count.
// kept_t (LDS, optional): the step of every kept character.  Both kernels below run exactly this.
__device__ __forceinline__ int ctc_collapse_row(const int* idx, const float* prob, int* text, float* kept_p, int* kept_t, int n, int T, int lane) {
    int base = 0;
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        const int cur = t < T ? idx[(size_t)n * T + t] : 0;
        int prev = __shfl_up(cur, 1);
        if (lane == 0) prev = t0 > 0 ? idx[(size_t)n * T + t0 - 1] : -1;
        const bool keep = t < T && cur != 0 && cur != prev;
        const unsigned long long mask = __ballot(keep);
        const int pos = base + __popcll(mask & ((1ull << lane) - 1ull));
        if (keep) {
            text[(size_t)n * T + pos] = cur; kept_p[pos] = prob[(size_t)n * T + t];
            if (kept_t) kept_t[pos] = t;
        }
        base += __popcll(mask);
    }
    for (int t = base + lane; t < T; t += 64) text[(size_t)n * T + t] = -1;
    return base;
}

__global__ __launch_bounds__(64) void ctc_collapse_kernel(const int* idx, const float* prob, int* text, int* len, float* score, int T) {
    __shared__ float kept_p[128];
    const int n = blockIdx.x, lane = threadIdx.x;
    const int base = ctc_collapse_row(idx, prob, text, kept_p, nullptr, n, T, lane);
    __syncthreads();
    if (lane == 0) {
        float s = 0.f;
        for (int k = 0; k < base; ++k) s = s + kept_p[k];  // time order, fp32 (oracle/nets.py ctc_greedy)
        len[n] = base;
        score[n] = base ? s / (float)base : 0.f;
    }
}

// round-half-away-from-zero of a * c / wc (wc > 0, c >= 0): the one rounding rule of the word quads (include/lumina_ocr.h)
__device__ __forceinline__ long long word_round_div(long long a, long long c, long long wc) {
    const long long num = a * c, mag = ((num < 0 ? -num : num) * 2 + wc) / (2 * wc);
    return num < 0 ? -mag : mag;
}

// ---- CTC collapse + the line's words (lumina_ocr_ctc_decode_words): one wave per line.  text / len / score as ctc_collapse_kernel;
// a lane that holds the first character of a word walks the word: its end, its fp32 score in time order, its columns, its quad ----
__global__ __launch_bounds__(64) void ctc_words_kernel(const int* idx, const float* prob, const int* quads, const int* widths, const int* flip,
                                                       int space_id, int* text, int* len, float* score, int* word_quads, int* word_span,
                                                       float* word_score, int* word_count, int T) {
    __shared__ float kept_p[128];
    __shared__ int kept_t[128];
    const int n = blockIdx.x, lane = threadIdx.x;
    const int base = ctc_collapse_row(idx, prob, text, kept_p, kept_t, n, T, lane);
    __syncthreads();
    if (lane == 0) {
        float s = 0.f;
        for (int k = 0; k < base; ++k) s = s + kept_p[k];
        len[n] = base;
        score[n] = base ? s / (float)base : 0.f;
    }
    const int* row = idx + (size_t)n * T;
    const int wc = widths[n];
    // the line quad's corners in the order the crop used them (crop_kernel, dbpost.hip: same test, same 64-bit integers)
    long long p[4][2];
#pragma unroll
    for (int t = 0; t < 4; ++t) { p[t][0] = quads[(size_t)n * 8 + 2 * t]; p[t][1] = quads[(size_t)n * 8 + 2 * t + 1]; }
#define D2(a, b) ((p[a][0] - p[b][0]) * (p[a][0] - p[b][0]) + (p[a][1] - p[b][1]) * (p[a][1] - p[b][1]))
    const long long cw2 = D2(1, 0) > D2(2, 3) ? D2(1, 0) : D2(2, 3);
    const long long ch2 = D2(3, 0) > D2(2, 1) ? D2(3, 0) : D2(2, 1);
#undef D2
    const int rot = 4 * ch2 >= 9 * cw2 ? 1 : 0;   // crop corner k is line corner (k + rot) & 3
    const bool turn = flip != nullptr && flip[n] != 0;
    int nwords = 0;
    for (int k0 = 0; k0 < base; k0 += 64) {
        const int k = k0 + lane;
        const bool inw = k < base && (space_id < 0 || row[kept_t[k]] != space_id);
        const bool start = inw && (k == 0 || (space_id >= 0 && row[kept_t[k - 1]] == space_id));
        const unsigned long long mask = __ballot(start);
        const int w = nwords + __popcll(mask & ((1ull << lane) - 1ull));
        nwords += __popcll(mask);
        if (!start || w >= LUMINA_MAX_WORDS || wc <= 0) continue;   // (uniform trip count: the lanes meet again at the next ballot)
        int e = k;   // last character of the word
        float s = 0.f + kept_p[k];
        while (e + 1 < base && (space_id < 0 || row[kept_t[e + 1]] != space_id)) { ++e; s = s + kept_p[e]; }
        int te = kept_t[e];   // last step of the last character's run
        const int cls = row[te];
        while (te + 1 < T && row[te + 1] == cls) ++te;
        int c0 = 4 * kept_t[k], c1 = 4 * (te + 1);
        c0 = c0 < wc ? c0 : wc; c1 = c1 < wc ? c1 : wc; c1 = c1 > c0 ? c1 : c0;
        const int s0 = turn ? wc - c1 : c0, s1 = turn ? wc - c0 : c1;
        const int cs[4] = {s0, s1, s1, s0};   // crop corner k of the word: top edge P0 -> P1 at s0, s1; bottom edge P3 -> P2 at s1, s0
        int* q = word_quads + ((size_t)n * LUMINA_MAX_WORDS + w) * 8;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int a = (c < 2 ? 0 : 3), b = (c < 2 ? 1 : 2);   // edge a -> b in crop corners
            const long long ax = p[(a + rot) & 3][0], ay = p[(a + rot) & 3][1], bx = p[(b + rot) & 3][0], by = p[(b + rot) & 3][1];
            const int j = (c + rot) & 3;   // the line's own corner on whose side this point lies
            q[2 * j] = (int)(ax + word_round_div(bx - ax, cs[c], wc));
            q[2 * j + 1] = (int)(ay + word_round_div(by - ay, cs[c], wc));
        }
        word_span[((size_t)n * LUMINA_MAX_WORDS + w) * 2] = k;
        word_span[((size_t)n * LUMINA_MAX_WORDS + w) * 2 + 1] = e - k + 1;
        word_score[(size_t)n * LUMINA_MAX_WORDS + w] = __fdiv_rn(s, (float)(e - k + 1));
    }
    if (lane == 0) word_count[n] = wc <= 0 ? 0 : (nwords < LUMINA_MAX_WORDS ? nwords : LUMINA_MAX_WORDS);
}

int grid_for(size_t total) {
    size_t g = (total + 255) / 256;
    return (int)(g > 256 * 64 ? 256 * 64 : (g ? g : 1));
}

// ---- orientation-classifier head: one wave per crop ----
__global__ __launch_bounds__(64) void cls_head_kernel(const bf16_t* __restrict__ feat, const float* __restrict__ w, const float* __restrict__ b, int P,
                                                      int C, int Cs, float thresh, int* label, float* score, int* flip, bf16_t* logits_bf16) {
    __shared__ float mean[256];
    __shared__ float lg[2];
    const int n = blockIdx.x, lane = threadIdx.x;
    const bf16_t* f = feat + (size_t)n * P * Cs;
    for (int c = lane; c < C; c += 64) {
        float s = 0.f;
        for (int q = 0; q < P; ++q) s = __fadd_rn(s, bf16_to_f32(f[(size_t)q * Cs + c]));
        mean[c] = __fdiv_rn(s, (float)P);
    }
    __syncthreads();
    if (lane < 2) {
        float acc = 0.f;
        for (int c = 0; c < C; ++c) acc = __fadd_rn(acc, __fmul_rn(w[lane * C + c], mean[c]));
        lg[lane] = __fadd_rn(acc, b[lane]);
    }
    __syncthreads();
    if (lane == 0) {
        const int lab = lg[1] > lg[0] ? 1 : 0;
        const float d = fabsf(__fsub_rn(lg[1], lg[0]));
        const float sc = __fdiv_rn(1.f, __fadd_rn(1.f, expf(-d)));
        label[n] = lab; score[n] = sc; flip[n] = (lab == 1 && sc > thresh) ? 1 : 0;
        logits_bf16[2 * n] = f32_to_bf16(lg[0]); logits_bf16[2 * n + 1] = f32_to_bf16(lg[1]);
    }
}

}  // namespace

hipError_t maxpool_launch(const bf16_t* x, bf16_t* y, int N, int H, int W, int C, int k, int s, int pad, int Ho, int Wo, hipStream_t st) {
    hipLaunchKernelGGL(maxpool_kernel, dim3(grid_for((size_t)N * Ho * Wo * (C / 8))), dim3(256), 0, st, x, y, N, H, W, C, k, s, pad, Ho, Wo);
    return hipGetLastError();
}

hipError_t dwconv_launch(const bf16_t* x, const bf16_t* w, const float* bias, bf16_t* y, int N, int H, int W, int C, int k,
                         int sh, int act, hipStream_t st) {
    const int Ho = (H + 2 * (k / 2) - k) / sh + 1;
    const size_t total = (size_t)N * Ho * ((W + 3) / 4) * (C / 8);
    if (total > 0x7fffffffull || (k != 3 && k != 5)) return hipErrorInvalidValue;
    const size_t lds = ((size_t)k * k * C + C) * sizeof(float);
    if (lds > 60 * 1024) return hipErrorInvalidValue;
    const dim3 g(grid_for(total));
#define DW(K_, A_) hipLaunchKernelGGL((dwconv_kernel<K_, A_>), g, dim3(256), lds, st, x, w, bias, y, N, H, W, C, sh, Ho)
#define DW_ACT(K_)                                                     \
    switch (act) {                                                     \
        case ACT_NONE: DW(K_, ACT_NONE); break;                        \
        case ACT_RELU: DW(K_, ACT_RELU); break;                        \
        case ACT_HSWISH: DW(K_, ACT_HSWISH); break;                    \
        default: return hipErrorInvalidValue;                          \
    }
    if (k == 3) { DW_ACT(3) } else { DW_ACT(5) }
#undef DW_ACT
#undef DW
    return hipGetLastError();
}

hipError_t se_fc_launch(const float* pool, int strips, const bf16_t* w1, const float* b1, const bf16_t* w2, const float* b2, bf16_t* gate,
                        int N, int HW, int C, int mid, hipStream_t st) {
    hipLaunchKernelGGL(se_fc_kernel, dim3(N), dim3(256), ((size_t)C + mid) * sizeof(float), st, pool, strips, w1, b1, w2, b2, gate, HW, C, mid);
    return hipGetLastError();
}

hipError_t se_scale_launch(const bf16_t* x, const bf16_t* gate, bf16_t* y, int N, int HW, int C, hipStream_t st) {
    hipLaunchKernelGGL(se_scale_kernel, dim3(grid_for((size_t)N * HW * (C / 8))), dim3(256), 0, st, x, gate, y, N, HW, C);
    return hipGetLastError();
}

hipError_t lstm_recurrent_launch(const bf16_t* xproj, const bf16_t* whh, bf16_t* out, int N, int T, hipStream_t st, int waves) {
    if (N < 1 || T < 1 || (waves != 3 && waves != 12)) return hipErrorInvalidValue;
    const dim3 grid(((N + LSEQ - 1) / LSEQ) * 2);
    if (waves == 3) hipLaunchKernelGGL(lstm3_kernel, grid, dim3(192), 0, st, xproj, whh, out, N, T);
    else hipLaunchKernelGGL(lstm_kernel, grid, dim3(768), 0, st, xproj, whh, out, N, T);
    return hipGetLastError();
}

size_t ctc_packed_weight_elems(int C, int K) { return (size_t)((C + CT_BN - 1) / CT_BN) * CT_BN * K; }

void pack_ctc_weights(const bf16_t* w, int C, int K, bf16_t* out) {
    const int ntiles = (C + CT_BN - 1) / CT_BN, npl = K / 8;
    for (int t = 0; t < ntiles; ++t)
        for (int c = 0; c < npl; ++c)
            for (int n = 0; n < CT_BN; ++n)
                for (int j = 0; j < 8; ++j) {
                    const int cls = t * CT_BN + n;
                    out[(((size_t)t * npl + c) * CT_BN + n) * 8 + j] = cls < C ? w[(size_t)cls * K + c * 8 + j] : (bf16_t)0;
                }
}

hipError_t ctc_fc_argmax_launch(const CtcFcParams& p, hipStream_t st) {
    if (p.K != CT_K || p.ntiles < 1 || p.M < 1) return hipErrorInvalidValue;   // the kernel is built for the recognisers' K = 192
    const size_t lds = CT_LDS;
    if (p.f16) {
        { hipError_t e = locr_dyn_lds(reinterpret_cast<const void*>(ctc_fc_argmax_kernel<1>), (int)CT_LDS); if (e != hipSuccess) return e; }
        hipLaunchKernelGGL(ctc_fc_argmax_kernel<1>, dim3((p.M + CT_ROWS - 1) / CT_ROWS), dim3(256), lds, st, p);
    } else {
        { hipError_t e = locr_dyn_lds(reinterpret_cast<const void*>(ctc_fc_argmax_kernel<0>), (int)CT_LDS); if (e != hipSuccess) return e; }
        hipLaunchKernelGGL(ctc_fc_argmax_kernel<0>, dim3((p.M + CT_ROWS - 1) / CT_ROWS), dim3(256), lds, st, p);
    }
    return hipGetLastError();
}

hipError_t ctc_collapse_launch(const int* idx, const float* prob, int* text, int* len, float* score, int N, int T, hipStream_t st) {
    if (T > 128) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ctc_collapse_kernel, dim3(N), dim3(64), 0, st, idx, prob, text, len, score, T);
    return hipGetLastError();
}

hipError_t ctc_words_launch(const int* idx, const float* prob, const int* quads, const int* widths, const int* flip, int space_id, int* text,
                            int* len, float* score, int* word_quads, int* word_span, float* word_score, int* word_count, int N, int T,
                            hipStream_t st) {
    if (T > 128) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ctc_words_kernel, dim3(N), dim3(64), 0, st, idx, prob, quads, widths, flip, space_id, text, len, score, word_quads,
                       word_span, word_score, word_count, T);
    return hipGetLastError();
}

hipError_t cls_head_launch(const bf16_t* feat, const float* w, const float* b, int N, int P, int C, int Cs, float thresh, int* label, float* score,
                           int* flip, bf16_t* logits_bf16, hipStream_t st) {
    if (N <= 0) return hipSuccess;
    if (C <= 0 || C > 256 || Cs < C || P <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cls_head_kernel, dim3(N), dim3(64), 0, st, feat, w, b, P, C, Cs, thresh, label, score, flip, logits_bf16);
    return hipGetLastError();
}
