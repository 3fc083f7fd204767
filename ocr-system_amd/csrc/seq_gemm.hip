// A-stationary streaming GEMM for the recogniser's tail (gfx950): the staging pattern of the CTC head (ops.hip, ctc_fc_argmax_kernel)
// with a storing epilogue.  A 256-thread work-group owns 128 rows; a wave's 32 rows stay in registers as the MFMA B operand for the
// whole launch, the 64-column weight tiles stream through two LDS buffers by LDS-DMA, a tile's 64 biases through a ring of four slots,
// both one tile ahead: one barrier per tile, and every weight byte is staged once per 128 rows instead of once per 64 x 64 tile.
// What defines the bits: v_mfma_f32_32x32x16_bf16 over the k steps ascending into a zero C operand (the sums of conv_mfma_kernel's
// 1x1 path), + bias in fp32, [activation,] one rounding to bf16.
#include "seq_gemm.h"

namespace {

constexpr int SG_ROWS = 4 * 32, SG_BN = 64, SG_NT = 2, SG_BIAS_SLOTS = 4;

template <int K, int EPI>
__global__ __launch_bounds__(256, 2) void seq_gemm_kernel(const SeqGemmParams p) {
    constexpr int KSTEPS = K / 16, NM = EPI == SEQ_POOL4 ? 4 : 1;   // NM: rows of x per output row (the pool window's members)
    constexpr int W_ITEMS = SG_BN * (K / 8), WIT = (W_ITEMS + 255) / 256, WBYTES = W_ITEMS * 16;
    static_assert(K % 16 == 0 && W_ITEMS % 64 == 0, "whole k steps; the ragged last staging pass ends on a wave boundary");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // the bias ring is an LDS object of its own: the compiler then knows that the weight DMA cannot write what the epilogue reads
    __shared__ __attribute__((aligned(16))) float sB[SG_BIAS_SLOTS * SG_BN];
    unsigned char* sW = smem;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int ntiles = (p.Cout + SG_BN - 1) / SG_BN, last = ntiles - 1;
    const int row = blockIdx.x * SG_ROWS + wave * 32 + r;
    const bool valid = row < p.M;

    // this lane's part of its row(s): the B operand of every k step (rows past M are zero and are not stored)
    bf16x8_t arow[NM][KSTEPS];
#pragma unroll
    for (int m = 0; m < NM; ++m) {
        size_t pix = (size_t)row;
        if constexpr (EPI == SEQ_POOL4) {
            const int n = row / p.T, t = row - n * p.T;
            pix = ((size_t)(n * 2 + (m >> 1))) * (2 * p.T) + 2 * t + (m & 1);
        }
        const bf16x8_t* src = reinterpret_cast<const bf16x8_t*>(p.x + pix * K) + h;
#pragma unroll
        for (int kc = 0; kc < KSTEPS; ++kc) {
            bf16x8_t v = {};
            if (valid) v = src[2 * kc];
            arow[m][kc] = v;
        }
    }

    // weight tile `tile` -> LDS buffer slot & 1 by LDS-DMA, lane-linear, which is the packed tile's own order; its 64 biases travel
    // through a register of 16 lanes into bias slot slot & 3 (landed).  A request past the last tile repeats the last tile into a
    // buffer nobody reads any more.
    uint4 breg = make_uint4(0, 0, 0, 0);
    auto stage = [&](int tile, int slot) {
        const uint4* src = reinterpret_cast<const uint4*>(p.wpk) + (size_t)tile * W_ITEMS + tid;
        unsigned char* dst = sW + (slot & 1) * WBYTES + (tid - lane) * 16;
#pragma unroll
        for (int it = 0; it < WIT; ++it)
            if (W_ITEMS % 256 == 0 || tid - lane + 256 * it < W_ITEMS)   // (whole waves: W_ITEMS % 64 == 0)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + 256 * it),
                                                 (__attribute__((address_space(3))) void*)(dst + 256 * it * 16), 16, 0, 0);
        if (tid < SG_BN / 4) breg = reinterpret_cast<const uint4*>(p.bias + (size_t)tile * SG_BN)[tid];
    };
    // the requests of this wave have landed; the barrier then makes every wave's part visible
    auto landed = [&](int slot) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (tid < SG_BN / 4) reinterpret_cast<uint4*>(sB + (slot & (SG_BIAS_SLOTS - 1)) * SG_BN)[tid] = breg;
        __syncthreads();
    };

    // tile t: the MFMAs from buffer t & 1 (the fragments of k step k + 1 are requested before the MFMAs of step k; the first step's
    // C operand is zero).  Tile t + 1 is requested into the other buffer before them.
    auto mma = [&](f32x16_t (&acc)[NM][SG_NT], int t) {
        const unsigned char* w = sW + (t & 1) * WBYTES + (h * SG_BN + r) * 16;
        bf16x8_t wf[2][SG_NT];
#pragma unroll
        for (int nt = 0; nt < SG_NT; ++nt) wf[0][nt] = *reinterpret_cast<const bf16x8_t*>(w + nt * 32 * 16);
#pragma unroll
        for (int kc = 0; kc < KSTEPS; ++kc) {
            if (kc + 1 < KSTEPS) {
#pragma unroll
                for (int nt = 0; nt < SG_NT; ++nt)
                    wf[(kc + 1) & 1][nt] = *reinterpret_cast<const bf16x8_t*>(w + (2 * (kc + 1) * SG_BN + nt * 32) * 16);
            }
#pragma unroll
            for (int m = 0; m < NM; ++m)
#pragma unroll
                for (int nt = 0; nt < SG_NT; ++nt) {
                    const f32x16_t c = kc == 0 ? f32x16_t{} : acc[m][nt];
                    acc[m][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[kc & 1][nt], arow[m][kc], c, 0, 0, 0);
                }
        }
    };
    // tile t's output values from its accumulators, then 16-byte stores: a lane holds 4 consecutive columns per accumulator quad;
    // v_permlane32_swap exchanges quad 2gp of the upper half-wave with quad 2gp + 1 of the lower one, after which half-wave h owns
    // columns 16 gp + 8 h .. + 7 of its row (conv_mfma.hip's direct store)
    auto store = [&](const f32x16_t (&acc)[NM][SG_NT], int t) {
        const float* bt = sB + (t & (SG_BIAS_SLOTS - 1)) * SG_BN + 4 * h;
        bf16_t* yrow = p.y + (size_t)row * p.Cout + t * SG_BN + 8 * h;
#pragma unroll
        for (int nt = 0; nt < SG_NT; ++nt)
#pragma unroll
            for (int gp = 0; gp < 2; ++gp) {
                float o[8];
#pragma unroll
                for (int g = 0; g < 2; ++g) {
                    const int q = 2 * gp + g;   // columns nt * 32 + 8 q + 4 h + (0 .. 3) are accumulator entries 4 q + (0 .. 3)
                    // (read as a fragment and re-typed, as the CTC head does: a float4 read of LDS while an LDS-DMA is pending gets a
                    // wait for that DMA in front of it)
                    const f32x4_t b = __builtin_bit_cast(f32x4_t, *reinterpret_cast<const bf16x8_t*>(bt + nt * 32 + 8 * q));
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if constexpr (EPI == SEQ_POOL4) {
                            float mx = -3.0e38f;   // maxpool_kernel's chain over the members' stored (rounded) values
#pragma unroll
                            for (int m = 0; m < NM; ++m)
                                mx = fmaxf(mx, bf16_to_f32(f32_to_bf16(apply_act(acc[m][nt][4 * q + e] + b[e], ACT_HSWISH))));
                            o[4 * g + e] = mx;
                        } else {
                            o[4 * g + e] = acc[0][nt][4 * q + e] + b[e];
                        }
                    }
                }
                const uint32_t q0x = pack_bf16x2(o[0], o[1]), q0y = pack_bf16x2(o[2], o[3]);
                const uint32_t q1x = pack_bf16x2(o[4], o[5]), q1y = pack_bf16x2(o[6], o[7]);
                const auto sx = __builtin_amdgcn_permlane32_swap(q0x, q1x, false, false);
                const auto sy = __builtin_amdgcn_permlane32_swap(q0y, q1y, false, false);
                const int co = nt * 32 + 16 * gp;
                if (valid && t * SG_BN + co + 8 * h < p.Cout) *reinterpret_cast<uint4*>(yrow + co) = make_uint4(sx[0], sy[0], sx[1], sy[1]);
            }
    };

    stage(0, 0);
    landed(0);
    if constexpr (EPI == SEQ_POOL4) {
        // four accumulator sets (one per window member) are one generation: MFMAs, then the tile's epilogue
        f32x16_t acc[NM][SG_NT];
        for (int t = 0; t < ntiles; ++t) {
            stage(min(t + 1, last), t + 1);
            mma(acc, t);
            store(acc, t);
            landed(t + 1);
        }
    } else {
        // two accumulator sets: the stores of tile t - 1 are issued in front of the MFMAs of tile t, so the wait for the next
        // weight tile at the end of the step finds them long done.  One barrier: after it buffer (t + 1) & 1 and bias slot
        // (t + 1) & 3 are complete, and buffer t & 1 and slot (t - 1) & 3 are free for the requests of step t + 1
        auto step = [&](f32x16_t (&accc)[NM][SG_NT], const f32x16_t (&acce)[NM][SG_NT], int t) {
            stage(min(t + 1, last), t + 1);
            store(acce, t - 1);
            mma(accc, t);
            landed(t + 1);
        };
        f32x16_t acc0[NM][SG_NT], acc1[NM][SG_NT];
        stage(min(1, last), 1);
        mma(acc0, 0);
        landed(1);
        int t = 1;
        for (; t + 1 < ntiles; t += 2) {
            step(acc1, acc0, t);
            step(acc0, acc1, t + 1);
        }
        if (t < ntiles) {
            step(acc1, acc0, t);
            store(acc1, t);
        } else {
            store(acc0, last);
        }
    }
}

template <int K, int EPI>
hipError_t launch(const SeqGemmParams& p, hipStream_t st) {
    const int lds = 2 * SG_BN * (K / 8) * 16;
    const void* fn = reinterpret_cast<const void*>(seq_gemm_kernel<K, EPI>);
    { hipError_t e = locr_dyn_lds(fn, lds); if (e != hipSuccess) return e; }
    hipLaunchKernelGGL((seq_gemm_kernel<K, EPI>), dim3((p.M + SG_ROWS - 1) / SG_ROWS), dim3(256), lds, st, p);
    return hipGetLastError();
}

}  // namespace

size_t seq_gemm_packed_elems(int cout, int K) { return (size_t)((cout + SG_BN - 1) / SG_BN) * SG_BN * K; }

void seq_gemm_pack_weights(const bf16_t* w, int cout, int K, bf16_t* out) {
    const int ntiles = (cout + SG_BN - 1) / SG_BN, npl = K / 8;
    for (int t = 0; t < ntiles; ++t)
        for (int c = 0; c < npl; ++c)
            for (int n = 0; n < SG_BN; ++n)
                for (int j = 0; j < 8; ++j) {
                    const int co = t * SG_BN + n;
                    out[(((size_t)t * npl + c) * SG_BN + n) * 8 + j] = co < cout ? w[(size_t)co * K + c * 8 + j] : (bf16_t)0;
                }
}

bool seq_gemm_supported(const SeqGemmParams& p) {
    if (p.M < 1 || p.Cout < 8 || p.Cout % 8 != 0 || (size_t)p.M * 4 > 0x7fffffffull) return false;
    if (p.epi == SEQ_STORE) return p.K == 288 || p.K == 192;
    if (p.epi == SEQ_POOL4) return p.K == 48 && p.T >= 1 && p.M % p.T == 0;
    return false;
}

hipError_t seq_gemm_launch(const SeqGemmParams& p, hipStream_t st) {
    if (!seq_gemm_supported(p)) return hipErrorInvalidValue;
    if (p.epi == SEQ_POOL4) return launch<48, SEQ_POOL4>(p, st);
    return p.K == 288 ? launch<288, SEQ_STORE>(p, st) : launch<192, SEQ_STORE>(p, st);
}

const char* seq_gemm_kernel_name(const SeqGemmParams& p) {
    if (p.epi == SEQ_POOL4) return "seq_gemm_kernel<48,1>";
    return p.K == 288 ? "seq_gemm_kernel<288,0>" : "seq_gemm_kernel<192,0>";
}
