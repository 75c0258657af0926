// bf16 x packed-weight (MLX affine 4/8-bit) GEMM on the matrix cores (qgemm.hip): the compute-bound Linear of a quantized
// DiT, the weights dequantised inside the kernel (no bf16 copy of W in HBM).  Format as quant.hip states it: packed u32
// [N, K*bits/32] (LSB first), bf16 scales / biases [N, K/group]; bits 4 / 8, group 32 / 64 / 128, K % 64 == 0.
#pragma once
#include "common.hpp"

namespace omx {

struct QWeight {
    const uint32_t* w;       // [rows, K*bits/32]
    const bf16_t* scales;    // [rows, K/group]
    const bf16_t* biases;    // [rows, K/group] or null (bias 0)
    int group, bits;
};

// 0 when (K, group, bits) is a format the kernel takes; otherwise set_error(`who`: ...) and 1
int qgemm_check_format(const char* who, int K, int group, int bits);

// out[M, N] = bf16(x . dq(W)^T); with resid and gate: out = bf16(resid + (x . dq(W)^T) * gate[col]) (the DiT's gated residual)
int launch_qgemm(bf16_t* out, const bf16_t* x, const QWeight& w, const bf16_t* resid, const bf16_t* gate, int M, int N, int K,
                 hipStream_t s);
// W = [n_plain plain rows | half gate rows | half up rows]: out_plain[m, c] = bf16(x.W[c]^T) (row stride ld_plain),
// out_act[m, c] = fused_swiglu(bf16(x.Wg[c]^T), bf16(x.Wu[c]^T)) (row stride ld_act) -- launch_gemm_bf16_swiglu's epilogue.
// n_plain % 4 == 0, half % 4 == 0, half > 0.
int launch_qgemm_swiglu(bf16_t* out_plain, int ld_plain, bf16_t* out_act, int ld_act, const bf16_t* x, const QWeight& w, int M,
                        int n_plain, int half, int K, hipStream_t s);

}  // namespace omx
