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
//
// The top-n form (omx_logprob_rows_top; the decode steps' per-token log-probabilities, logprob.hpp) keeps both launches and both texts:
//
//   logprob_top_partial_kernel   the partial kernel's body, then top_n rounds of a wave-wide maximum over the chunk's 1024 keys (16 per
//                                lane, in registers) -> the chunk's own best top_n as 32-bit keys, descending
//   logprob_top_merge_kernel     the merge kernel's body on wave 0 of a 256-thread block, then top_n rounds over the heads of the row's
//                                ceil(V / 1024) sorted candidate lists (at most four per thread)
//
// A key orders by (logit descending, column ascending), sample_key's order (random.hpp).  A bf16 logit widened to f32 has an orderable
// word (below) whose upper half decides, so a chunk-local key is (upper half + 1) << 10 | (1023 - column in the chunk); 0 = no column.
#include <math.h>

#include "logprob.hpp"
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
// TOP: also cand [rows, nch, top_n], the chunk's best top_n keys in descending order (0 where the chunk has fewer columns)
template <bool TOP>
__device__ __forceinline__ void logprob_partial_body(float* __restrict__ partials, uint32_t* __restrict__ part_arg,
                                                     float* __restrict__ tgt, const bf16_t* __restrict__ panel, int64_t ld,
                                                     int c0, int npc, const uint32_t* __restrict__ targets, int64_t rows,
                                                     int V, int nch, uint32_t* __restrict__ cand, int top_n) {
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
    if (TOP) {
        uint32_t key[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int cl = (j >> 3) * 512 + lane * 8 + (j & 7);   // column in the chunk; columns >= V take no part
            key[j] = chunk * kChunk + cl < V ? (((orderable(x[j]) >> 16) + 1u) << 10) | (uint32_t)(kChunk - 1 - cl) : 0u;
        }
        uint32_t mine = 0;   // lane t keeps the winner of round t
        for (int t = 0; t < top_n; ++t) {
            uint32_t best = 0;
#pragma unroll
            for (int j = 0; j < 16; ++j) best = max(best, key[j]);
            best = wave_max_u(best);
#pragma unroll
            for (int j = 0; j < 16; ++j) key[j] = key[j] == best ? 0u : key[j];   // (keys are distinct: one column leaves)
            mine = lane == t ? best : mine;
        }
        if (lane < top_n) cand[(r * nch + chunk) * top_n + lane] = mine;
    }
}

__global__ __launch_bounds__(256) void logprob_partial_kernel(float* __restrict__ partials, uint32_t* __restrict__ part_arg,
                                                              float* __restrict__ tgt, const bf16_t* __restrict__ panel, int64_t ld,
                                                              int c0, int npc, const uint32_t* __restrict__ targets, int64_t rows,
                                                              int V, int nch) {
    logprob_partial_body<false>(partials, part_arg, tgt, panel, ld, c0, npc, targets, rows, V, nch, nullptr, 0);
}

__global__ __launch_bounds__(256) void logprob_top_partial_kernel(float* __restrict__ partials, uint32_t* __restrict__ part_arg,
                                                                  float* __restrict__ tgt, uint32_t* __restrict__ cand,
                                                                  const bf16_t* __restrict__ panel, int64_t ld, int c0, int npc,
                                                                  const uint32_t* __restrict__ targets, int64_t rows, int V, int nch,
                                                                  int top_n) {
    logprob_partial_body<true>(partials, part_arg, tgt, panel, ld, c0, npc, targets, rows, V, nch, cand, top_n);
}

// a row's statistics from its nch partials, by wave 0 of the block (further waves only join the barrier): lse and arg are thread 0's
__device__ __forceinline__ void merge_row_stats(float* term, const float* __restrict__ pr, const uint32_t* __restrict__ pa, int nch,
                                                float& lse, uint32_t& arg) {
    const int lane = threadIdx.x;
    float M = 0.f;
    uint32_t first = 0xFFFFFFFFu;
    if (lane < 64) {
        uint32_t um = 0;
        for (int j = lane; j < nch; j += 64) um = max(um, orderable(pr[2 * j]));
        um = wave_max_u(um);
        M = from_orderable(um);
        for (int j = lane; j < nch; j += 64) {
            const float mj = pr[2 * j], lj = pr[2 * j + 1];
            term[j] = lj == 0.f ? 0.f : lj * expf(mj - M);
            if (orderable(mj) == um) first = min(first, (uint32_t)j);
        }
        first = wave_min_u(first);
    }
    __syncthreads();
    if (lane == 0) {
        float L = 0.f;
        for (int j = 0; j < nch; ++j) L += term[j];   // ascending chunk order
        lse = M + logf(L);
        arg = pa[first];
    }
}

__device__ __forceinline__ float target_logprob(uint32_t t, float tgt, float lse, int V) {
    return t == OMX_NO_TARGET ? 0.f : (t < (uint32_t)V ? tgt - lse : __uint_as_float(0x7FC00000u));
}

__global__ __launch_bounds__(64) void logprob_merge_kernel(float* __restrict__ logprobs, uint32_t* __restrict__ greedy,
                                                           float* __restrict__ lse_out, const float* __restrict__ partials,
                                                           const uint32_t* __restrict__ part_arg, const float* __restrict__ tgt,
                                                           const uint32_t* __restrict__ targets, int V, int nch) {
    __shared__ float term[1024];   // V <= 2^20: at most 1024 chunks
    const int64_t r = blockIdx.x;
    float lse = 0.f;
    uint32_t arg = 0;
    merge_row_stats(term, partials + r * nch * 2, part_arg + r * nch, nch, lse, arg);
    if (threadIdx.x == 0) {
        logprobs[r] = target_logprob(targets[r], tgt[r], lse, V);
        if (lse_out) lse_out[r] = lse;
        if (greedy) greedy[r] = arg;
    }
}

// a chunk-local key as the row's 64-bit key (orderable upper half + 1 : ~column), 0 staying 0
__device__ __forceinline__ unsigned long long row_key(uint32_t k, int chunk) {
    const uint32_t col = (uint32_t)chunk * kChunk + (kChunk - 1 - (k & (kChunk - 1)));
    return k ? ((unsigned long long)(k >> 10) << 32) | (uint32_t)~col : 0ull;
}
// ... and the logit a row key stands for: the orderable word of a widened bf16 ends in 0000 (positive) or FFFF (negative)
__device__ __forceinline__ float row_key_logit(unsigned long long key) {
    const uint32_t hi = (uint32_t)(key >> 32) - 1u;
    return from_orderable((hi << 16) | ((hi & 0x8000u) ? 0u : 0xFFFFu));
}

// The merge of the top-n form: the statistics as above, then the row's top_n out of its nch descending candidate lists.  Thread t owns
// the lists of chunks t, t + 256, ..; a round takes the block-wide maximum of the lists' heads and the owner moves that list on.
// Row r's outputs land at entry r of `o`'s arrays -- or, o.ring_count set (ONE row), at entry (*ring_count - 1) % ring_cap: the slot of
// the token the step's finalize just counted --, and o.row_slot set, once more at entry row_slot[r] of the slot_ arrays.
__global__ __launch_bounds__(256) void logprob_top_merge_kernel(const LogprobTopOut o, const float* __restrict__ partials,
                                                                const uint32_t* __restrict__ part_arg, const float* __restrict__ tgt,
                                                                const uint32_t* __restrict__ targets,
                                                                const uint32_t* __restrict__ cand, int V, int nch, int top_n) {
    __shared__ float term[1024];
    __shared__ unsigned long long red[2][4];
    __shared__ float lse_all;
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x;
    const int64_t at = o.ring_count ? (int64_t)((*o.ring_count - 1) % o.ring_cap) : r;
    const int64_t slot = o.row_slot ? o.row_slot[r] : 0;
    float lse = 0.f;
    uint32_t arg = 0;
    merge_row_stats(term, partials + r * nch * 2, part_arg + r * nch, nch, lse, arg);
    if (tid == 0) {
        const float lp = target_logprob(targets[r], tgt[r], lse, V);
        o.logprobs[at] = lp;
        if (o.lse) o.lse[at] = lse;
        if (o.greedy) o.greedy[at] = arg;
        if (o.row_slot) o.slot_lp[slot] = lp;
        lse_all = lse;
    }
    if (top_n == 0) return;
    __syncthreads();
    lse = lse_all;
    const uint32_t* cr = cand + r * nch * top_n;
    unsigned long long head[4];
    int next[4];   // the list's entries taken so far + 1
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int c = tid + 256 * u;
        head[u] = c < nch ? row_key(cr[(int64_t)c * top_n], c) : 0ull;
        next[u] = 1;
    }
    for (int t = 0; t < top_n; ++t) {
        unsigned long long best = max(max(head[0], head[1]), max(head[2], head[3]));
#pragma unroll
        for (int w = 32; w > 0; w >>= 1) best = max(best, (unsigned long long)__shfl_xor(best, w, 64));
        if ((tid & 63) == 0) red[t & 1][tid >> 6] = best;
        __syncthreads();   // (one barrier a round: the next round writes the other half of red)
        best = max(max(red[t & 1][0], red[t & 1][1]), max(red[t & 1][2], red[t & 1][3]));
        if (best == 0ull) break;   // fewer than top_n columns (refused on the host: top_n <= V)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (head[u] != best) continue;
            const uint32_t id = ~(uint32_t)best;
            const float lp = row_key_logit(best) - lse;
            o.top_ids[at * top_n + t] = id;
            o.top_lp[at * top_n + t] = lp;
            if (o.row_slot) {
                o.slot_ids[slot * top_n + t] = id;
                o.slot_top[slot * top_n + t] = lp;
            }
            const int c = tid + 256 * u;
            head[u] = next[u] < top_n ? row_key(cr[(int64_t)c * top_n + next[u]], c) : 0ull;
            next[u] += 1;
        }
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

int check_top_n(const char* name, int top_n, int V) {
    OMX_REQUIRE(top_n >= 1 && top_n <= OMX_LOGPROBS_MAX_TOP && top_n <= V, "%s: top_n = %d is outside 1..min(%d, V = %d)", name, top_n,
                OMX_LOGPROBS_MAX_TOP, V);
    return 0;
}

// the scratch of the top-n form, carved in this order: partials [rows, nch, 2] f32, part_arg [rows, nch], cand [rows, nch, top_n], tgt [rows]
struct TopScratch {
    float* partials;
    uint32_t *part_arg, *cand;
    float* tgt;
};
TopScratch carve_top_scratch(void* ws, int64_t rows, int64_t nch, int top_n) {
    TopScratch t;
    t.partials = (float*)ws;
    t.part_arg = (uint32_t*)(t.partials + rows * nch * 2);
    t.cand = t.part_arg + rows * nch;
    t.tgt = (float*)(t.cand + rows * nch * top_n);
    return t;
}

int launch_top_merge(const LogprobTopOut& o, const TopScratch& t, const uint32_t* targets, int64_t rows, int V, int top_n, hipStream_t s) {
    logprob_top_merge_kernel<<<(unsigned)rows, 256, 0, s>>>(o, t.partials, t.part_arg, t.tgt, targets, t.cand, V, (V + kChunk - 1) / kChunk,
                                                           top_n);
    OMX_LAUNCH_CHECK();
    return 0;
}

}  // namespace

size_t logprob_top_scratch_bytes(int64_t rows, int V, int top_n) {
    const int64_t nch = (V + kChunk - 1) / kChunk;
    return (size_t)(rows * nch * (12 + 4 * (int64_t)top_n) + rows * 4);
}

int launch_logprob_top(const LogprobTopOut& out, void* scratch, const bf16_t* logits, int64_t ld, const uint32_t* targets, int64_t rows,
                       int V, int top_n, hipStream_t s) {
    OMX_REQUIRE(scratch && logits && targets && out.logprobs, "launch_logprob_top: null tensor");
    if (check_shape("launch_logprob_top", ld, rows, V, OMX_BFLOAT16)) return 1;
    OMX_REQUIRE(ld >= V && aligned16(logits), "launch_logprob_top: ld = %lld is below V = %d, or the rows are not 16-byte aligned", (long long)ld, V);
    if (top_n != 0 && check_top_n("launch_logprob_top", top_n, V)) return 1;
    OMX_REQUIRE(top_n == 0 || (out.top_ids && out.top_lp), "launch_logprob_top: top_n = %d without top_ids / top_lp", top_n);
    OMX_REQUIRE(!out.row_slot || (out.slot_lp && (top_n == 0 || (out.slot_ids && out.slot_top))), "launch_logprob_top: row_slot without the slots' arrays");
    OMX_REQUIRE(!out.ring_count || rows == 1, "launch_logprob_top: a ring takes one row a launch, not %lld", (long long)rows);
    if (rows == 0) return 0;
    const int nch = (V + kChunk - 1) / kChunk;
    const TopScratch t = carve_top_scratch(scratch, rows, nch, top_n);
    const unsigned grid = (unsigned)((rows * nch + 3) / 4);
    if (top_n == 0)
        logprob_partial_kernel<<<grid, 256, 0, s>>>(t.partials, t.part_arg, t.tgt, logits, ld, 0, nch, targets, rows, V, nch);
    else
        logprob_top_partial_kernel<<<grid, 256, 0, s>>>(t.partials, t.part_arg, t.tgt, t.cand, logits, ld, 0, nch, targets, rows, V, nch, top_n);
    OMX_LAUNCH_CHECK();
    return launch_top_merge(out, t, targets, rows, V, top_n, s);
}

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

int omx_logprob_top_partial(float* partials, uint32_t* part_arg, float* tgt, uint32_t* cand, const void* panel, int64_t ld, int c0, int P,
                            const uint32_t* targets, int64_t rows, int V, int top_n, omx_dtype dtype, omx_stream stream) {
    using namespace omx;
    OMX_REQUIRE(partials && part_arg && tgt && cand && panel && targets, "omx_logprob_top_partial: null tensor");
    if (check_shape("omx_logprob_top_partial", ld, rows, V, dtype) || check_top_n("omx_logprob_top_partial", top_n, V)) return 1;
    OMX_REQUIRE(c0 >= 0 && c0 % kChunk == 0 && P > 0 && c0 <= V - P && (P % kChunk == 0 || c0 + P == V),
                "omx_logprob_top_partial: columns [%d, %d + %d) of %d: c0 must be a multiple of %d, and P too unless the panel ends the row",
                c0, c0, P, V, kChunk);
    OMX_REQUIRE(ld >= P, "omx_logprob_top_partial: ld = %lld is below the panel's %d columns", (long long)ld, P);
    OMX_REQUIRE(aligned16(panel), "omx_logprob_top_partial: the panel must be 16-byte aligned");
    if (rows == 0) return 0;
    const int nch = (V + kChunk - 1) / kChunk, npc = (P + kChunk - 1) / kChunk;
    const int64_t waves = rows * npc;
    OMX_REQUIRE(waves <= ((int64_t)1 << 32), "omx_logprob_top_partial: %lld rows x %d chunks exceed one launch", (long long)rows, npc);
    logprob_top_partial_kernel<<<(unsigned)((waves + 3) / 4), 256, 0, (hipStream_t)stream>>>(partials, part_arg, tgt, cand, (const bf16_t*)panel,
                                                                                           ld, c0, npc, targets, rows, V, nch, top_n);
    OMX_LAUNCH_CHECK();
    return 0;
}

int omx_logprob_top_merge(float* logprobs, uint32_t* greedy, float* lse, uint32_t* top_ids, float* top_logprobs, const float* partials,
                          const uint32_t* part_arg, const float* tgt, const uint32_t* cand, const uint32_t* targets, int64_t rows, int V,
                          int top_n, omx_stream stream) {
    using namespace omx;
    OMX_REQUIRE(logprobs && top_ids && top_logprobs && partials && part_arg && tgt && cand && targets, "omx_logprob_top_merge: null tensor");
    if (check_shape("omx_logprob_top_merge", 0, rows, V, OMX_BFLOAT16) || check_top_n("omx_logprob_top_merge", top_n, V)) return 1;
    if (rows == 0) return 0;
    LogprobTopOut o = {};
    o.logprobs = logprobs; o.greedy = greedy; o.lse = lse; o.top_ids = top_ids; o.top_lp = top_logprobs;
    const TopScratch t = {const_cast<float*>(partials), const_cast<uint32_t*>(part_arg), const_cast<uint32_t*>(cand), const_cast<float*>(tgt)};
    return launch_top_merge(o, t, targets, rows, V, top_n, (hipStream_t)stream);
}

int omx_logprob_rows_top(float* logprobs, uint32_t* greedy, float* lse, uint32_t* top_ids, float* top_logprobs, const void* logits,
                         int64_t ld, const uint32_t* targets, int64_t rows, int V, int top_n, omx_dtype dtype, omx_stream stream) {
    using namespace omx;
    OMX_REQUIRE(logprobs && top_ids && top_logprobs && logits && targets, "omx_logprob_rows_top: null tensor");
    if (check_shape("omx_logprob_rows_top", ld, rows, V, dtype) || check_top_n("omx_logprob_rows_top", top_n, V)) return 1;
    OMX_REQUIRE(ld >= V, "omx_logprob_rows_top: ld = %lld is below V = %d", (long long)ld, V);
    OMX_REQUIRE(aligned16(logits), "omx_logprob_rows_top: the rows must be 16-byte aligned");
    if (rows == 0) return 0;
    void* ws = nullptr;
    if (get_workspace(&ws, logprob_top_scratch_bytes(rows, V, top_n))) return 1;
    LogprobTopOut o = {};
    o.logprobs = logprobs; o.greedy = greedy; o.lse = lse; o.top_ids = top_ids; o.top_lp = top_logprobs;
    return launch_logprob_top(o, ws, (const bf16_t*)logits, ld, targets, rows, V, top_n, (hipStream_t)stream);
}

}  // extern "C"
