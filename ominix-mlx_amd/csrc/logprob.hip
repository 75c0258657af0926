// Per-row log-probability of a target column from bf16 logits, without a softmax row: what a text's log-likelihood is made of
// (include/omx.h "per-row log-probability").  Two launches, neither waits on another block (no flags, no atomics):
//
//   logprob_partial_kernel   one wave per (row, 1024-column chunk): 64 lanes x 16 elements, two 16-byte loads per lane
//                            -> m = max, l = sum exp(x - m), arg = first index of the max; the chunk that holds the row's target
//                               column also writes that logit
//   logprob_merge_kernel     one wave per row over its ceil(V / 1024) partials in ascending chunk order
//                            -> lse = M + log(sum l_j exp(m_j - M)), logprob = target logit - lse, greedy = arg of the first chunk at M
//
// The chunk grid is counted from column 0 of the FULL row and every sum has one order (a lane's 16 terms by index, the wave_sum tree of
// common.hpp, the chunks ascending), so a row's bits are a function of its V logits alone: not of the panel the chunk was read from,
// nor of the number of rows or which rows share the launch.  HBM-bound: the panel is read once, 8 + 4 bytes leave per 2 KB read.
#include <math.h>

#include "vec.hpp"
#include "workspace.hpp"

namespace omx {
namespace {

constexpr int kChunk = OMX_LOGPROB_CHUNK;   // columns per (row, chunk) wave: 64 lanes x 2 loads x 8 bf16
static_assert(kChunk == kWave * 16, "one wave reads a chunk with two 16-byte loads per lane");

// the total order of argmax_key (common.hpp) on the value alone: larger float <=> larger word, NaN below everything
__device__ __forceinline__ uint32_t orderable(float v) {
    uint32_t u = __float_as_uint(v);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return v != v ? 0u : u;
}
__device__ __forceinline__ float from_orderable(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u); }

template <int CTRL>
__device__ __forceinline__ uint32_t dpp_u(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true);
}
__device__ __forceinline__ uint32_t readlane_u(uint32_t v, int lane) { return (uint32_t)__builtin_amdgcn_readlane((int)v, lane); }
__device__ __forceinline__ uint32_t wave_max_u(uint32_t v) {
    v = max(v, dpp_u<kDppXor1>(v));
    v = max(v, dpp_u<kDppXor2>(v));
    v = max(v, dpp_u<kDppHalfMirror>(v));
    v = max(v, dpp_u<kDppRowMirror>(v));
    return max(max(readlane_u(v, 0), readlane_u(v, 16)), max(readlane_u(v, 32), readlane_u(v, 48)));
}
__device__ __forceinline__ uint32_t wave_min_u(uint32_t v) {
    v = min(v, dpp_u<kDppXor1>(v));
    v = min(v, dpp_u<kDppXor2>(v));
    v = min(v, dpp_u<kDppHalfMirror>(v));
    v = min(v, dpp_u<kDppRowMirror>(v));
    return min(min(readlane_u(v, 0), readlane_u(v, 16)), min(readlane_u(v, 32), readlane_u(v, 48)));
}

// panel [rows, ld]: its column 0 is column c0 of the row; chunks [c0 / 1024, c0 / 1024 + npc) of the row's nch are reduced.
// partials [rows, nch, 2] = (m, l), part_arg [rows, nch], tgt [rows].
__global__ __launch_bounds__(256) void logprob_partial_kernel(float* __restrict__ partials, uint32_t* __restrict__ part_arg,
                                                              float* __restrict__ tgt, const bf16_t* __restrict__ panel, int64_t ld,
                                                              int c0, int npc, const uint32_t* __restrict__ targets, int64_t rows,
                                                              int V, int nch) {
    const int lane = threadIdx.x & 63;
    const int64_t wid = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wid >= rows * npc) return;   // (whole waves leave: nothing below synchronises the block)
    const int64_t r = wid / npc;
    const int chunk = c0 / kChunk + (int)(wid % npc);
    const bf16_t* row = panel + r * ld;        // row[c - c0] = column c of the full row, for c in this panel
    float x[16];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        // columns >= V count as -inf (clamped address + select: a predicated LOAD makes hipcc branch and drain the queue per load)
        const int c = chunk * kChunk + h * 512 + lane * 8;
        float v[8];
        Vec16<OMX_BFLOAT16>::ld(row + (min(c, V - 8) - c0), v);
#pragma unroll
        for (int j = 0; j < 8; ++j) x[h * 8 + j] = c < V ? v[j] : -INFINITY;
    }
    uint32_t um = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) um = max(um, orderable(x[j]));
    um = wave_max_u(um);
    const float m = from_orderable(um);   // exact: a logit widened to f32
    float l = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) l += __expf(x[j] - m);   // the lane's 16 terms in index order
    l = wave_sum(l);
    uint32_t first = 0xFFFFFFFFu;
#pragma unroll
    for (int j = 15; j >= 0; --j)
        if (orderable(x[j]) == um) first = (uint32_t)(chunk * kChunk + (j >> 3) * 512 + lane * 8 + (j & 7));
    first = wave_min_u(first);
    if (lane == 0) {
        const int64_t p = r * nch + chunk;
        partials[2 * p] = m;
        partials[2 * p + 1] = m == -INFINITY ? 0.f : l;   // a chunk of -inf only: no mass (exp(-inf - -inf) is not a number)
        part_arg[p] = first;
        const uint32_t t = targets[r];
        if (t < (uint32_t)V && (int)(t / kChunk) == chunk) tgt[r] = bf16_to_f32(row[(int)t - c0]);
    }
}

__global__ __launch_bounds__(64) void logprob_merge_kernel(float* __restrict__ logprobs, uint32_t* __restrict__ greedy,
                                                           float* __restrict__ lse_out, const float* __restrict__ partials,
                                                           const uint32_t* __restrict__ part_arg, const float* __restrict__ tgt,
                                                           const uint32_t* __restrict__ targets, int V, int nch) {
    __shared__ float term[1024];   // V <= 2^20: at most 1024 chunks
    const int lane = threadIdx.x;
    const int64_t r = blockIdx.x;
    const float* pr = partials + r * nch * 2;
    uint32_t um = 0;
    for (int j = lane; j < nch; j += 64) um = max(um, orderable(pr[2 * j]));
    um = wave_max_u(um);
    const float M = from_orderable(um);
    uint32_t first = 0xFFFFFFFFu;
    for (int j = lane; j < nch; j += 64) {
        const float mj = pr[2 * j], lj = pr[2 * j + 1];
        term[j] = lj == 0.f ? 0.f : lj * expf(mj - M);
        if (orderable(mj) == um) first = min(first, (uint32_t)j);
    }
    first = wave_min_u(first);
    __syncthreads();
    if (lane == 0) {
        float L = 0.f;
        for (int j = 0; j < nch; ++j) L += term[j];   // ascending chunk order
        const float lse = M + logf(L);
        const uint32_t t = targets[r];
        logprobs[r] = t == OMX_NO_TARGET ? 0.f : (t < (uint32_t)V ? tgt[r] - lse : __uint_as_float(0x7FC00000u));
        if (lse_out) lse_out[r] = lse;
        if (greedy) greedy[r] = part_arg[r * nch + first];
    }
}

int check_shape(const char* name, int64_t ld, int64_t rows, int V, omx_dtype dtype) {
    OMX_REQUIRE(dtype == OMX_BFLOAT16, "%s: dtype %d is not supported (bfloat16 logits only)", name, (int)dtype);
    OMX_REQUIRE(V > 0 && V % 8 == 0, "%s: V = %d must be a positive multiple of 8 (16-byte loads)", name, V);
    OMX_REQUIRE(V <= (1 << 20), "%s: V = %d exceeds 2^20 columns", name, V);
    OMX_REQUIRE(ld % 8 == 0, "%s: ld = %lld must be a multiple of 8 (16-byte loads)", name, (long long)ld);
    OMX_REQUIRE(rows >= 0 && rows <= (1 << 24), "%s: %lld rows (0..2^24)", name, (long long)rows);
    return 0;
}

}  // namespace
}  // namespace omx

extern "C" {

int omx_logprob_partial(float* partials, uint32_t* part_arg, float* tgt, const void* panel, int64_t ld, int c0, int P,
                        const uint32_t* targets, int64_t rows, int V, omx_dtype dtype, omx_stream stream) {
    using namespace omx;
    OMX_REQUIRE(partials && part_arg && tgt && panel && targets, "omx_logprob_partial: null tensor");
    if (check_shape("omx_logprob_partial", ld, rows, V, dtype)) return 1;
    OMX_REQUIRE(c0 >= 0 && c0 % kChunk == 0 && P > 0 && c0 <= V - P && (P % kChunk == 0 || c0 + P == V),
                "omx_logprob_partial: columns [%d, %d + %d) of %d: c0 must be a multiple of %d, and P too unless the panel ends the row",
                c0, c0, P, V, kChunk);
    OMX_REQUIRE(ld >= P, "omx_logprob_partial: ld = %lld is below the panel's %d columns", (long long)ld, P);
    OMX_REQUIRE(aligned16(panel), "omx_logprob_partial: the panel must be 16-byte aligned");
    if (rows == 0) return 0;
    const int nch = (V + kChunk - 1) / kChunk, npc = (P + kChunk - 1) / kChunk;
    const int64_t waves = rows * npc;
    OMX_REQUIRE(waves <= ((int64_t)1 << 32), "omx_logprob_partial: %lld rows x %d chunks exceed one launch", (long long)rows, npc);
    logprob_partial_kernel<<<(unsigned)((waves + 3) / 4), 256, 0, (hipStream_t)stream>>>(partials, part_arg, tgt, (const bf16_t*)panel, ld,
                                                                                       c0, npc, targets, rows, V, nch);
    OMX_LAUNCH_CHECK();
    return 0;
}

int omx_logprob_merge(float* logprobs, uint32_t* greedy, float* lse, const float* partials, const uint32_t* part_arg, const float* tgt,
                      const uint32_t* targets, int64_t rows, int V, omx_stream stream) {
    using namespace omx;
    OMX_REQUIRE(logprobs && partials && part_arg && tgt && targets, "omx_logprob_merge: null tensor");
    if (check_shape("omx_logprob_merge", 0, rows, V, OMX_BFLOAT16)) return 1;
    if (rows == 0) return 0;
    logprob_merge_kernel<<<(unsigned)rows, 64, 0, (hipStream_t)stream>>>(logprobs, greedy, lse, partials, part_arg, tgt, targets, V,
                                                                        (V + kChunk - 1) / kChunk);
    OMX_LAUNCH_CHECK();
    return 0;
}

int omx_logprob_rows(float* logprobs, uint32_t* greedy, float* lse, const void* logits, int64_t ld, const uint32_t* targets, int64_t rows,
                     int V, omx_dtype dtype, omx_stream stream) {
    using namespace omx;
    OMX_REQUIRE(logprobs && logits && targets, "omx_logprob_rows: null tensor");
    if (check_shape("omx_logprob_rows", ld, rows, V, dtype)) return 1;
    OMX_REQUIRE(ld >= V, "omx_logprob_rows: ld = %lld is below V = %d", (long long)ld, V);
    if (rows == 0) return 0;
    const int64_t nch = (V + kChunk - 1) / kChunk;
    void* ws = nullptr;
    if (get_workspace(&ws, (size_t)rows * nch * 12 + (size_t)rows * 4)) return 1;
    float* partials = (float*)ws;
    uint32_t* part_arg = (uint32_t*)(partials + rows * nch * 2);
    float* tgt = (float*)(part_arg + rows * nch);
    return omx_logprob_partial(partials, part_arg, tgt, logits, ld, 0, V, targets, rows, V, dtype, stream) ||
           omx_logprob_merge(logprobs, greedy, lse, partials, part_arg, tgt, targets, rows, V, stream);
}

}  // extern "C"
