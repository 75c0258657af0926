// What follows a float32 product in the SAN-M layers (funasr-mlx/src/paraformer.rs, funasr-nano-mlx/src/sensevoice_encoder.rs), shared by
// paraformer.hip and sensevoice_encoder.hip: the FSMN memory block on its own (fsmn_add_kernel), the fused epilogue that finishes a float32
// GEMM -- split sum, bias, FSMN, residual, LayerNorm -- in one launch (f32_epilogue_ln_kernel), and the description of such a tail
// (F32Tail) with its two launchers.  Each kernel has a one-utterance form (SEG = false: Paraformer's launches, unchanged) and a form over
// stacked utterances (SEG = true) whose FSMN taps stop at utterance boundaries.
#pragma once
#include <stdlib.h>

#include "gemm.hpp"

namespace omx {
namespace {

// out[t, c] = attn_proj[t, c] + v[t, c] + sum_j w[c, j] * v[t + j - pad, c]     (depthwise conv, zero padded)
// resid != null: out = resid + bf16(that)   (the layer's attention residual, paraformer.rs:625-629, in the same launch)
// SEG: the T rows are the utterances of `sg` stacked; the taps of a row stop at its utterance's first and last row (each utterance zero
// padded on its own, as when it is passed alone).  SEG = false is the Paraformer launch: one utterance, rows 0 .. T - 1.
template <int DT, bool SEG>
__global__ __launch_bounds__(256) void fsmn_add_kernel(typename Elem<DT>::T* __restrict__ out, const typename Elem<DT>::T* __restrict__ attn_proj,
                                                       const typename Elem<DT>::T* __restrict__ v, int64_t ldv,
                                                       const typename Elem<DT>::T* __restrict__ w, int T, int C, int ksize,
                                                       const typename Elem<DT>::T* __restrict__ resid, SegTable sg) {
    typedef Elem<DT> E;
    const int pad = ksize / 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < (int64_t)T * C; i += (int64_t)gridDim.x * 256) {
        const int t = (int)(i / C), c = (int)(i % C);
        int lo = 0, hi = T;
        if constexpr (SEG) seg_bounds(sg, t, lo, hi);
        float acc = 0.f;
        for (int j = 0; j < ksize; ++j) {
            const int tt = t + j - pad;
            if (tt >= lo && tt < hi) acc = fmaf(E::ld(w + (size_t)c * ksize + j), E::ld(v + (size_t)tt * ldv + c), acc);
        }
        // fsmn_out = conv(v) + v (arrays of the activation dtype in the reference's op chain), then attn_proj + fsmn_out
        const float fsmn = E::rnd(E::rnd(acc) + E::ld(v + (size_t)t * ldv + c));
        float o = E::ld(attn_proj + i) + fsmn;
        if (resid) o = E::ld(resid + i) + E::rnd(o);
        E::st(out + i, o);
    }
}

// ---- round 6: a float32 GEMM's epilogue, the FSMN memory block and the LayerNorm that follows, in ONE launch ----
// The 30 s pass was ~1 000 dependent launches; 216 of them were split-K reduces and 168 LayerNorms, each 4-5 us for a [T, 512] tensor that
// the launch before had just written.  Here the rows of a product the GEMM left raw (gemm.hpp GemmF32::defer_partial) are finished in place:
//     y = sum over splits (in split order) + bias  [relu]  [+ resid]                          -- gemm_f32_reduce_kernel's epilogue, same order
//     FSMN:  y = y + (conv(v)[t] + v[t]),  then  y = resid2 + y                               -- fsmn_add_kernel's arithmetic, same order
//     out = y;   ln_out = LayerNorm(y)
// TPR threads share a row (one 16-byte vector each, VPT of them when the row is longer than 1 024 floats), 256 / TPR rows per block: a first
// form with one WAVE per row (rownorm_kernel's shape, bit-identical sums) took 11 us per launch -- 8 columns x 11 taps of dependent loads per
// lane -- and made the pass slower than the three launches it replaced.  The row sums go lane -> wave -> LDS here, so the normalised values
// can differ from the separate LayerNorm launch in the last bit.
// SEG: as in fsmn_add_kernel -- the FSMN taps of a row stay inside its utterance of `sg`; everything else is per row and does not change.
template <int TPR, int VPT, bool SEG>
__global__ __launch_bounds__(256) void f32_epilogue_ln_kernel(float* __restrict__ out, float* __restrict__ ln_out, const float* __restrict__ partial,
                                                              int splits, int M, int dim, const float* __restrict__ bias, int relu,
                                                              const float* __restrict__ resid, int64_t ldr, const float* __restrict__ v, int64_t ldv,
                                                              const float* __restrict__ fw, int ksize, const float* __restrict__ resid2,
                                                              const float* __restrict__ ln_w, const float* __restrict__ ln_b, float eps, SegTable sg) {
    constexpr int RPB = 256 / TPR, WPR = TPR / 64;          // rows per block, waves per row
    __shared__ float red[2][4];
    const int rl = threadIdx.x / TPR, t = threadIdx.x % TPR;
    const int row = blockIdx.x * RPB + rl;
    const bool live = row < M;
    const int pad = ksize / 2;
    f32x4 y[VPT];
#pragma unroll
    for (int k = 0; k < VPT; ++k) {
        const int c0 = (t + k * TPR) * 4;
        f32x4 a = {0.f, 0.f, 0.f, 0.f};
        if (live) {
            for (int sp = 0; sp < splits; ++sp) a += *reinterpret_cast<const f32x4*>(partial + ((int64_t)sp * M + row) * dim + c0);
            if (bias) a += *reinterpret_cast<const f32x4*>(bias + c0);
            if (relu) { a[0] = fmaxf(a[0], 0.f); a[1] = fmaxf(a[1], 0.f); a[2] = fmaxf(a[2], 0.f); a[3] = fmaxf(a[3], 0.f); }
            if (resid) a += *reinterpret_cast<const f32x4*>(resid + (int64_t)row * ldr + c0);
            if (v) {
                int lo = 0, hi = M;
                if constexpr (SEG) seg_bounds(sg, row, lo, hi);
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                const float* fwc = fw + (size_t)c0 * ksize;      // the taps of this thread's four columns: 4 * ksize consecutive floats
                for (int jj = 0; jj < ksize; ++jj) {
                    const int tt = row + jj - pad;
                    if (tt >= lo && tt < hi) {
                        const f32x4 vv = *reinterpret_cast<const f32x4*>(v + (int64_t)tt * ldv + c0);
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[j] = fmaf(fwc[j * ksize + jj], vv[j], acc[j]);
                    }
                }
                const f32x4 vt = *reinterpret_cast<const f32x4*>(v + (int64_t)row * ldv + c0);
                a = a + (acc + vt);
                if (resid2) a = *reinterpret_cast<const f32x4*>(resid2 + (int64_t)row * dim + c0) + a;
            }
            if (out) *reinterpret_cast<f32x4*>(out + (int64_t)row * dim + c0) = a;
        }
        y[k] = a;
    }
    if (!ln_out) return;
    auto row_sum = [&](float x, int which) -> float {
        x = wave_sum(x);
        if (WPR == 1) return x;
        const int w = threadIdx.x >> 6;
        __syncthreads();
        if ((threadIdx.x & 63) == 0) red[which][w] = x;
        __syncthreads();
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < WPR; ++i) s += red[which][rl * WPR + i];
        return s;
    };
    float sm = 0.f;
#pragma unroll
    for (int k = 0; k < VPT; ++k) sm += (y[k][0] + y[k][1]) + (y[k][2] + y[k][3]);
    const float mean = row_sum(sm, 0) / (float)dim;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < VPT; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) q += (y[k][j] - mean) * (y[k][j] - mean);
    const float rstd = 1.0f / sqrtf(row_sum(q, 1) / (float)dim + eps);
    if (!live) return;
#pragma unroll
    for (int k = 0; k < VPT; ++k) {
        const int c0 = (t + k * TPR) * 4;
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (y[k][j] - mean) * rstd;
        if (ln_w) o = o * *reinterpret_cast<const f32x4*>(ln_w + c0);
        if (ln_b) o = o + *reinterpret_cast<const f32x4*>(ln_b + c0);
        *reinterpret_cast<f32x4*>(ln_out + (int64_t)row * dim + c0) = o;
    }
}

inline bool f32_tail_width_ok(int n) { return n == 512 || n == 1024 || n == 2048; }
struct F32Tail {                 // what follows a float32 product (all optional)
    const float* bias = nullptr; int relu = 0;
    const float* resid = nullptr; int64_t ldr = 0;
    const float* v = nullptr; int64_t ldv = 0; const float* fw = nullptr; int ksize = 0; const float* resid2 = nullptr;   // the FSMN memory block
    const float* ln_w = nullptr; const float* ln_b = nullptr; float* ln_out = nullptr;
    const SegTable* seg = nullptr;   // the rows are stacked utterances: the FSMN taps stop at their boundaries (sensevoice_encoder.hip)
};
// rows of `partial` ([splits][M, N], summed in split order) finished by ONE launch with everything in `t`; out may be null when only the
// normalised rows are kept
inline int launch_f32_tail(float* out, const float* partial, int splits, int M, int N, const F32Tail& t, hipStream_t s) {
    OMX_REQUIRE(f32_tail_width_ok(N), "paraformer: fused epilogue takes rows of 512, 1024 or 2048 floats (N=%d)", N);
    const bool seg = t.seg && t.v;
    const SegTable sg = seg ? *t.seg : SegTable{};
#define OMX_TAIL(TPR, VPT, SEG)                                                                                                           \
    f32_epilogue_ln_kernel<TPR, VPT, SEG><<<(unsigned)((M + 256 / TPR - 1) / (256 / TPR)), 256, 0, s>>>(                                   \
        out, t.ln_out, partial, splits, M, N, t.bias, t.relu, t.resid, t.ldr, t.v, t.ldv, t.fw, t.ksize, t.resid2, t.ln_w, t.ln_b, 1e-5f, sg)
    if (seg) {
        if (N == 512) OMX_TAIL(128, 1, true);
        else if (N == 1024) OMX_TAIL(256, 1, true);
        else OMX_TAIL(256, 2, true);
    } else {
        if (N == 512) OMX_TAIL(128, 1, false);
        else if (N == 1024) OMX_TAIL(256, 1, false);
        else OMX_TAIL(256, 2, false);
    }
#undef OMX_TAIL
    OMX_LAUNCH_CHECK();
    return 0;
}
// out [M, N] = x [M, K] . w [N, K]^T, finished by the launch above
inline int gemm_f32_with_tail(float* out, const float* x, const float* w, int M, int N, int K, const F32Tail& t, float* scratch_out, hipStream_t s) {
    const float* partial = nullptr;
    int splits = 1;
    float* raw = out ? out : scratch_out;       // (a product nobody reads as such still needs somewhere to land when K is not split)
    GemmF32 p = {x, w, nullptr, nullptr, raw, M, N, K, K, K, N, N, 0, 0, 0, 1, 0, 0, 1.0f};
    p.defer_partial = &partial;
    p.defer_splits = &splits;
    if (launch_gemm_f32(p, s)) return 1;
    return launch_f32_tail(out, partial, splits, M, N, t, s);
}
inline bool fuse_f32_tails() {
    static const bool on = [] { const char* e = getenv("OMX_PARAFORMER_FUSE"); return !(e && e[0] == '0'); }();
    return on;
}

}  // namespace
}  // namespace omx
