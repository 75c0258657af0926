// The arithmetic that the decode GEMV kernels share, each piece written ONCE: gemv.hip (bf16 / float16 weights), quant.hip (packed
// weights, VALU), qgemv_mfma.hip (packed 4-bit, matrix cores), qgemv_rows.hip (packed, a handful of rows), gemv_chain.hip (down +
// q/k/v in one launch) and attn_step.hip (O, gate/up, down and the next q/k/v inside the attention launch) must agree bit for bit -- the
// VALU-against-rows comparison is exact and token equality across the routes and the step's forms rests on it -- so they call these
// instead of carrying a copy.  Everything here is inlined straight-line code on values: no pointer, no branch enters a kernel's
// streaming loop through it.  A = Act16<F16> (act16.hpp): bfloat16, or float16 with the same rounding points.
// Who calls what:
//   dot8                     rows_dot below; gemv.hip (gemv_generic_kernel, whose rows are not held in registers)
//   rows_dot                 gemv.hip (gemv_kernel's OMX_COMPUTE); gemv_chain.hip (phase A's OMX_COMPUTE, the q/k/v rows); attn_step.hip
//                            (oproj_phase, gateup_reduce, down_reduce, the q/k/v rows of down_qkv_phase)
//   residual_pair            gemv_chain.hip (down_qkv_kernel); attn_step.hip (down_qkv_phase)
//   sumsq8 / norm8           the prologues of gemv.hip, qgemv_body.inc (quant.hip), qgemv_mfma.hip, qgemv_rows.hip; rmsnorm_in_lds below
//   rmsnorm_in_lds           gemv_chain.hip (down_qkv_kernel); attn_step.hip (gateup_phase, down_qkv_phase)
//   epi_bits                 every row epilogue of the files above; residual_pair below
// (The packed kernels' unpack and activation staging are beside qfield in quant.hpp; argmax_key is in common.hpp.)
#pragma once
#include "act16.hpp"
#include "gemv.hpp"

namespace omx {

// one 16-byte weight vector against its eight activations: lo then hi of each dword, one fma chain.
// F16: float16 weights, widened to f32 (exact) for the same fma chain as bf16 -- not v_dot2_f32_f16, whose two products and the
// accumulator meet in one unspecified rounding step: the chain keeps one rounding per product-add in a fixed order, the bound the
// tests check, and the kernel is bound by HBM, not by these VALU ops
template <bool F16 = false>
__device__ __forceinline__ float dot8(const u32x4 w, const float (&xf)[8], float acc) {
    typedef Act16<F16> A;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        acc = fmaf(A::lo(w[i]), xf[2 * i], acc);
        acc = fmaf(A::hi(w[i]), xf[2 * i + 1], acc);
    }
    return acc;
}

// ---- NR rows held in registers (NV 16-byte vectors per lane each) against a vector in LDS: the reduce of every decode GEMV ----
// xs is already advanced to the caller's K slice.  acc[r] = the wave's sum of row r: zeroed, the dot8 chain over j = 0..NV-1 on
// xs[j * 64 + lane] unpacked lo then hi of each dword, wave_sum.  What happens to acc stays with the caller.
template <bool F16, int NR, int NV>
__device__ __forceinline__ void rows_dot(const u32x4 (*w)[NV], const u32x4* xs, int lane, float (&acc)[NR]) {
    typedef Act16<F16> A;
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[r] = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const u32x4 xp = xs[j * 64 + lane];
        float xf[8];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            xf[2 * q] = A::lo(xp[q]);
            xf[2 * q + 1] = A::hi(xp[q]);
        }
#pragma unroll
        for (int r = 0; r < NR; ++r) acc[r] = dot8<F16>(w[r][j], xf, acc[r]);
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[r] = wave_sum(acc[r]);
}

// ---- RMSNorm prologue on one packed 16-byte vector (eight elements) ----
// the squares of the eight elements join ss in one fma chain: lo then hi of dword q = 0..3
template <class A>
__device__ __forceinline__ float sumsq8(const u32x4 raw, float ss) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float lo = A::lo(raw[q]), hi = A::hi(raw[q]);
        ss = fmaf(lo, lo, ss);
        ss = fmaf(hi, hi, ss);
    }
    return ss;
}
// x * rstd * w, two products and one rounding per element
template <class A>
__device__ __forceinline__ u32x4 norm8(const u32x4 raw, const u32x4 nw, float rstd) {
    u32x4 o;
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = A::pack(A::lo(raw[q]) * rstd * A::lo(nw[q]), A::hi(raw[q]) * rstd * A::hi(nw[q]));
    return o;
}

// ---- the PRO_RMSNORM prologue on a row that already sits in LDS (a kernel that received it as granules in mid-launch), in place ----
// Thread t of the first 256 (`member`) owns vectors t, t + 256, ...: the same sumsq8 chain, block_sum<4> (common.hpp: wave sums, then the
// four of them added in wave order from 0.f) and norm8 as gemv_kernel's prologue.  Every barrier waits for LDS only, so weight rows the
// caller has asked for stay in flight across it; ALL waves of the workgroup call this (the waves past the fourth only join the barriers).
__device__ __forceinline__ u32x4 ld_nt(const u32x4* p) { return __builtin_nontemporal_load(p); }   // a weight vector: streamed once
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
template <class A, int PV>
__device__ __forceinline__ void rmsnorm_in_lds(u32x4* xs, float* red, const u32x4 (&nwv)[PV], int n, float eps, bool member) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float ss = 0.f;
    u32x4 xv[PV];
#pragma unroll
    for (int i = 0; i < PV; ++i) {
        xv[i] = xs[(threadIdx.x & 255) + i * 256];
        ss = sumsq8<A>(xv[i], ss);
    }
    ss = wave_sum(ss);
    lds_barrier();
    if (member && lane == 0) red[wave] = ss;
    lds_barrier();
    ss = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) ss += red[i];
    const float rstd = 1.0f / sqrtf(ss / (float)n + eps);
    if (member) {
#pragma unroll
        for (int i = 0; i < PV; ++i) xs[threadIdx.x + i * 256] = norm8<A>(xv[i], nwv[i], rstd);
    }
    lds_barrier();
}

// ---- the 16 bits a row leaves behind: v0 the row's f32 sum (v1: the `up` row's of a SwiGLU pair) ----
// EPI_STORE / EPI_ARGMAX: the rounded sum (the caller stores it and, for EPI_ARGMAX, builds its argmax_key from A::val of it);
// EPI_RESIDUAL: resid + the rounded sum, rounded again (resid_bits is read by the caller, under EPI_RESIDUAL only); EPI_SWIGLU below
template <int EPI, class A>
__device__ __forceinline__ uint16_t epi_bits(float v0, float v1, uint16_t resid_bits, int single_round) {
    static_assert(EPI == EPI_STORE || EPI == EPI_RESIDUAL || EPI == EPI_SWIGLU || EPI == EPI_ARGMAX, "the 16-bit epilogues");
    if (EPI == EPI_RESIDUAL) return A::bits(A::val(resid_bits) + A::rnd(v0));
    if (EPI == EPI_SWIGLU) {
        // nn::silu(gate) * up, every primitive's result held in 16 bits
        // (qwen3-mlx/src/model.rs:264-265; mlx-rs/src/nn/activation.rs:876-880)
        const float g = A::rnd(v0);
        const float u = A::rnd(v1);
        const float den = 1.0f + expf(-g);
        // mlx_rs_core::fused_swiglu(up, gate) (metal_kernels.rs:11-18): one kernel, one rounding
        if (single_round) return A::bits(g / den * u);
        const float sg = A::rnd(1.0f / den);
        return A::bits(A::rnd(g * sg) * u);
    }
    return A::bits(v0);
}

// ---- the finish of a PAIR of K-split EPI_RESIDUAL rows: part_of_pair = [2][KSPLIT] partials, res2 = the two residuals packed ----
// each row's partials added in wave order from 0.f, bf16(resid + bf16(sum)) on the low and the high half, one dword out
template <class A, int KSPLIT>
__device__ __forceinline__ uint32_t residual_pair(const float* part_of_pair, uint32_t res2) {
    float v[2] = {0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 2; ++e) {
#pragma unroll
        for (int w = 0; w < KSPLIT; ++w) v[e] += part_of_pair[e * KSPLIT + w];
    }
    return (uint32_t)epi_bits<EPI_RESIDUAL, A>(v[0], 0.f, (uint16_t)(res2 & 0xFFFFu), 0) |
           ((uint32_t)epi_bits<EPI_RESIDUAL, A>(v[1], 0.f, (uint16_t)(res2 >> 16), 0) << 16);
}

// ---- expert parallelism: only experts [lo, lo + n) live on this rank (n == 0: all of them) ----
// false: expert e belongs to another rank and the block has no work (block-uniform: the caller returns BEFORE any barrier);
// otherwise e becomes the index into this rank's stack
__device__ __forceinline__ bool local_expert(size_t& e, int lo, int n) {
    if (n > 0) {
        if (e < (size_t)lo || e >= (size_t)(lo + n)) return false;
        e -= (size_t)lo;
    }
    return true;
}

}  // namespace omx
