// A-stationary streaming GEMM of the recogniser's tail (seq_gemm.hip): y[M][Cout] = x[M][K] * W^T[K][Cout] + bias for the short K of the
// LSTM x-projections (288, 192) and of rec.conv2 (48), all output columns per work-group.
#pragma once
#include "common.h"

enum SeqGemmEpi : int {
    SEQ_STORE = 0,   // y[m][co] = bf16(acc + bias): the conv epilogue with ACT_NONE
    SEQ_POOL4 = 1,   // 1x1 conv + hswish + 2x2 / stride-2 max pool of a [N][2][2T][K] tensor: row m = (n, t) is the maximum over the window
                     // members (dy, dx) = (0,0) (0,1) (1,0) (1,1) of bf16(hswish(acc + bias)), y is [N][1][T][Cout]
};

struct SeqGemmParams {
    const bf16_t* x;    // SEQ_STORE: [M][K]; SEQ_POOL4: [N][2][2T][K]
    const bf16_t* wpk;  // seq_gemm_pack_weights
    const float* bias;  // [ntiles * 64], zero padded
    bf16_t* y;          // [M][Cout]
    int M, K, Cout;     // Cout % 8 == 0; columns >= Cout of the last tile are not stored
    int T;              // SEQ_POOL4: pooled positions per image (M = N * T)
    int epi;
};

// tiles of 64 output columns in the order the kernel's LDS buffers hold them: [tile][K / 8][64 columns][8]; rows >= cout are zero
size_t seq_gemm_packed_elems(int cout, int K);
void seq_gemm_pack_weights(const bf16_t* w /*[cout][K]*/, int cout, int K, bf16_t* out);
bool seq_gemm_supported(const SeqGemmParams& p);
hipError_t seq_gemm_launch(const SeqGemmParams& p, hipStream_t st);
const char* seq_gemm_kernel_name(const SeqGemmParams& p);
