// KV-cached decode attention (Tq == 1) for gfx950: split-KV flash-decode.
//   reference: mlx_rs_core::scaled_dot_product_attention (mlx-rs-core/src/utils.rs:191-209) ->
//   mlx_fast_scaled_dot_product_attention (mlx-c fast.h:189-198), whose Tq==1 case MLX serves with
//   a dedicated vector kernel (mlx-rs/src/fast.rs:114).  HBM-bound: 2*Hkv*T*D*2 bytes per layer,
//   but at batch 1 / ctx 2k it is LATENCY that matters (9 MB per layer): the kernel is written to
//   have a short dependent chain, not just coalesced loads.
//
// The per-split arithmetic and its lane mapping (K/V rows straight to registers, the G = H/Hkv query heads of a KV head together, one
// running max per head and wave, the waves' partials merged through LDS) are AttnRow's (attn_row.hpp), the text the batched decode's
// attention (engine_batch.hip) is built from as well.  Here: grid = (B*Hkv) x nsplit, a split's token range derived from the launch's
// split count, the runtime mask, and attn_combine_kernel, which merges the splits and rounds once to the output dtype.
// The decode ENGINE does not use this kernel: its attention launch (q/k norm + RoPE + cache append + SDPA + split merge with a
// position-independent first load round) is attn_step.hip.
#include <algorithm>

#include "attn.hpp"
#include "attn_row.hpp"

namespace omx {

namespace {

// the launch's runtime mask over the keys, one value per token for every row and head: scores()'s hook
struct KeyMask {
    int mode;
    const void* mask;
    __device__ __forceinline__ float operator()(float d, int tok, bool live) const {
        if (mode == OMX_MASK_BOOL) {
            if (live && !reinterpret_cast<const uint8_t*>(mask)[tok]) d = -INFINITY;
        } else if (mode == OMX_MASK_ADDITIVE) {
            if (live) d += bf16_to_f32(reinterpret_cast<const bf16_t*>(mask)[tok]);
        }
        return d;
    }
};

// block (b, kvh, split): this launch's token range and K/V base, then AttnRow (attn_row.hpp) over the row's own K/V -- the rows of
// the next step in flight while this step's are applied, the loop of attn_own_row (engine_batch.hip)
template <int D, int GT>
__global__ __launch_bounds__(kBlock) void attn_decode_kernel(const AttnDecodeArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    using Row = AttnRow<D, GT>;
    constexpr int LPR = Row::LPR, STEP = Row::STEP;
    const int bk = blockIdx.x, split = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int c = lane % LPR;           // 8-element chunk of the head dim owned by this lane
    const int sg = lane / LPR;          // token sub-group inside the wave
    const int b = bk / a.Hkv, kvh = bk % a.Hkv;
    const int G = a.H / a.Hkv;
    const int Tk = a.Tk - (a.causal_tail ? a.B - 1 - b : 0);
    // token range of this split: multiples of the block step
    const int per = (Tk + a.nsplit - 1) / a.nsplit;
    const int chunk = ((per + STEP * kWaves - 1) / (STEP * kWaves)) * (STEP * kWaves);
    const int t_begin = split * chunk;
    const int t_end = min(Tk, t_begin + chunk);

    const bf16_t* Kb = a.k + (size_t)b * a.kv_batch_stride + (size_t)kvh * a.kv_head_stride;
    const bf16_t* Vb = a.v + (size_t)b * a.kv_batch_stride + (size_t)kvh * a.kv_head_stride;

    // the first K/V step goes out before anything else
    u32x4 kr[kUnroll], vr[kUnroll];
    int t0 = t_begin + wave * STEP;
    if (t0 < t_end) Row::issue_kv(kr, vr, Kb, Vb, t0, t_end, sg, c);

    const KeyMask mask = {a.mask_mode, a.mask};
    Row row;
    row.begin(a.q + (size_t)b * (a.q_bs ? a.q_bs : (int64_t)a.H * D), a.q_hs ? a.q_hs : D, a.scale, kvh, G, c);
    for (; t0 < t_end; t0 += STEP * kWaves) {
        float s[kUnroll][GT];
        float vf[kUnroll][8];
        row.scores(kr, vr, t0, t_end, sg, mask, s, vf);
        if (t0 + STEP * kWaves < t_end) Row::issue_kv(kr, vr, Kb, Vb, t0 + STEP * kWaves, t_end, sg, c);   // independent of the softmax below
        row.update(s, vf);
    }
    row.finish(smem, a.ws_o, a.ws_ml, a.nsplit, (size_t)b * a.H + kvh * G, G, split);
}

// merge splits: out[head, d] = sum_i e^{m_i-M} o_i[d] / sum_i e^{m_i-M} l_i, rounded once to bf16.
// Phase 1 is split-parallel (one lane per split, wave reductions), phase 2 is d-parallel with the
// split loop unrolled so its loads pipeline instead of forming a dependent chain.
template <int D>
__global__ __launch_bounds__(D) void attn_combine_kernel(bf16_t* __restrict__ out, const float* __restrict__ ws_o,
                                                         const float* __restrict__ ws_ml, int nsplit) {
    __shared__ float sm_f[512];
    __shared__ float sm_L;
    const size_t head = blockIdx.x;
    const int d = threadIdx.x, lane = threadIdx.x & 63;
    const float* ml = ws_ml + head * nsplit * 2;
    if (threadIdx.x < 64) {
        float mloc = -INFINITY;
        for (int i = lane; i < nsplit; i += 64) mloc = fmaxf(mloc, ml[2 * i]);
        const float M = wave_max(mloc);
        float lloc = 0.f;
        for (int i = lane; i < nsplit; i += 64) {
            const float mi = ml[2 * i];
            const float f = (mi == -INFINITY) ? 0.f : __expf(mi - M);
            sm_f[i] = f;
            lloc = fmaf(f, ml[2 * i + 1], lloc);
        }
        const float L = wave_sum(lloc);
        if (lane == 0) sm_L = L;
    }
    __syncthreads();
    const float* src = ws_o + head * nsplit * D + d;
    float acc0 = 0.f, acc1 = 0.f;
    int i = 0;
    for (; i + 16 <= nsplit; i += 16) {   // 16 independent loads in flight, then the FMAs
        float v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = src[(size_t)(i + j) * D];
#pragma unroll
        for (int j = 0; j < 16; j += 2) {
            acc0 = fmaf(sm_f[i + j], v[j], acc0);
            acc1 = fmaf(sm_f[i + j + 1], v[j + 1], acc1);
        }
    }
    for (; i + 4 <= nsplit; i += 4) {
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = src[(size_t)(i + j) * D];
        acc0 = fmaf(sm_f[i], v[0], acc0);
        acc1 = fmaf(sm_f[i + 1], v[1], acc1);
        acc0 = fmaf(sm_f[i + 2], v[2], acc0);
        acc1 = fmaf(sm_f[i + 3], v[3], acc1);
    }
    for (; i < nsplit; ++i) acc0 = fmaf(sm_f[i], src[(size_t)i * D], acc0);
    out[head * D + d] = f32_to_bf16((acc0 + acc1) / sm_L);
}

}  // namespace

size_t attn_decode_ws_bytes(int BH, int nsplit, int D) { return (size_t)BH * nsplit * (D + 2) * sizeof(float); }

int launch_attn_decode(const AttnDecodeArgs& a, int D, hipStream_t s) {
    const int G = a.H / a.Hkv;
    OMX_REQUIRE(a.H % a.Hkv == 0, "sdpa: H=%d not a multiple of Hkv=%d", a.H, a.Hkv);
    OMX_REQUIRE(G >= 1 && G <= 8, "sdpa decode: %d query heads per KV head unsupported (max 8)", G);
    OMX_REQUIRE(a.nsplit >= 1 && a.nsplit <= 512, "sdpa decode: nsplit %d out of range (1..512)", a.nsplit);
    const dim3 grid(a.B * a.Hkv, a.nsplit), block(kBlock);
    const int gt = G <= 1 ? 1 : G <= 2 ? 2 : G <= 4 ? 4 : 8;
#define OMX_ATTN_CASE(DD, GG)                                                                           \
    if (D == DD && gt == GG) {                                                                          \
        const size_t shmem = AttnRow<DD, GG>::SMEM_BYTES;                                               \
        if (shmem > 48 * 1024)                                                                          \
            OMX_HIP_CHECK(hipFuncSetAttribute((const void*)attn_decode_kernel<DD, GG>,                  \
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem)); \
        attn_decode_kernel<DD, GG><<<grid, block, shmem, s>>>(a);                                       \
        OMX_LAUNCH_CHECK();                                                                             \
        attn_combine_kernel<DD><<<a.B * a.H, DD, 0, s>>>(a.out, a.ws_o, a.ws_ml, a.nsplit);             \
        OMX_LAUNCH_CHECK();                                                                             \
        return 0;                                                                                       \
    }
    OMX_ATTN_CASE(128, 1) OMX_ATTN_CASE(128, 2) OMX_ATTN_CASE(128, 4) OMX_ATTN_CASE(128, 8)
    OMX_ATTN_CASE(64, 1) OMX_ATTN_CASE(64, 2) OMX_ATTN_CASE(64, 4) OMX_ATTN_CASE(64, 8)
#undef OMX_ATTN_CASE
    return set_error("sdpa decode: head_dim %d unsupported (64 or 128)", D);
}

}  // namespace omx
