// Batched decode of up to 8 independent sequences on one loaded Qwen3 model (include/omx.h "Batched decode").
//
// The reference's Model::forward and KVCache carry a batch dimension ([B, L] ids, [B, Hkv, T, D] cache, mlx-rs-core/src/cache.rs); the
// engine's own step pins B = 1.  A batch object adds the ragged form: n_slots sequences, each with its own K/V slabs, position, pending
// token and sampler, of which one step advances any subset as the M rows of ONE weight stream per Linear -- the rows launches of the
// speculative verify pass (gemv_rows.hip, qgemv_rows.hip), called through the same batched pass (engine_prefill.hip).  What differs
// from a verify pass is here: the rows are M different sequences, so the embedding gather, the cache append and the attention take
// their position, token and slab per row from a slot table in device memory, and the sampler advances that table -- n steps of a call
// are enqueued back to back and the host waits once.
//
// Attention splits are kChunk tokens wide whatever the batch holds: a sequence's partials, and the order its merge adds them in,
// depend on its own length only, so a sequence's bits do not depend on its neighbours (attn_decode_kernel derives its chunk from the
// launch's split count, which follows the longest sequence).
//
// kv_bits = 8 (omx_qwen3_batch_create_kv): the slots keep their K/V rows as 8-bit MLX affine codes (Kv8Layer, engine_model.hpp) --
// quantised by the scatter as they are appended (SlotRows8, prefill.hip), read packed by batch_attn_kv8_kernel, the same block over
// another row source (KvAffine8, attn_row.hpp); a prompt pass works on one bf16 staging pair (KvSlabs::packed).
#include "attn_row.hpp"
#include "engine_model.hpp"

namespace omx {
namespace {

constexpr int kMaxSlots = 8;
constexpr int kChunk = 256;        // tokens per attention split: a multiple of the block step of both head widths (64 / 128 tokens)
constexpr int kRingSteps = 1024;   // steps of one decode call the token ring holds

// ---- embedding rows of the pending tokens.  BITS = 0: a bf16 table, rows copied; else the packed table, each element
// (float)q * scale + bias with one rounding -- qembed_row (quant.hpp), what qembed_rows_kernel (engine_prefill.hip) runs.  One block per row.
template <int BITS>
__global__ __launch_bounds__(256) void batch_embed_kernel(bf16_t* __restrict__ out, const void* __restrict__ table_, const bf16_t* __restrict__ scales,
                                                          const bf16_t* __restrict__ biases, const BatchSlot* __restrict__ slots,
                                                          const int* __restrict__ row_slot, int hidden, int group) {
    const size_t id = slots[row_slot[blockIdx.x]].pending;
    if constexpr (BITS == 0) {
        const u32x4* src = reinterpret_cast<const u32x4*>(reinterpret_cast<const bf16_t*>(table_) + id * (size_t)hidden);
        u32x4* dst = reinterpret_cast<u32x4*>(out + (size_t)blockIdx.x * hidden);
        for (int j = threadIdx.x; j < hidden / 8; j += blockDim.x) dst[j] = src[j];
    } else {
        qembed_row<BITS>(out + (size_t)blockIdx.x * hidden, reinterpret_cast<const uint32_t*>(table_), scales, biases, id, hidden, group);
    }
}

// ---- ragged split-KV decode attention, built from AttnRow (attn_row.hpp: the per-split arithmetic and its lane mapping, the text of
// attn_decode_kernel as well).
// grid = (T * Hkv) x nsplit; block (r, kvh, split) covers tokens [split * chunk, min(len, (split + 1) * chunk)) of row r's slot, len =
// pos + 1 read from the slot table; a block past its sequence's end writes nothing and the merge never reads its partial.
struct BatchAttnArgs {
    const bf16_t* q;           // [T, H, D]
    const bf16_t *kbase, *vbase;
    size_t slot_stride, head_stride;
    const BatchSlot* slots;
    const int* row_slot;
    int H, Hkv, cap, chunk, nsplit_cap;
    float scale;
    float *ws_o, *ws_ml;       // [T * H][nsplit_cap][D], [T * H][nsplit_cap][2]
    bf16_t* out;               // [T, H * D]
};
// ... and of the grouped form (batch_attn_shared_kernel): the call's rows, their shared spans (RaggedRows) and the tuning
struct BatchSharedArgs {
    BatchAttnArgs a;
    int T, group_min, group_rows;
    int grp_owner[kMaxSlots], grp_shared[kMaxSlots];
};

// The slabs of a launch: rows(slot, kvh) = the source (attn_row.hpp) of that slot's KV head.  bf16 slabs [Hkv, cap, D] ...
struct Bf16Slabs {
    const BatchAttnArgs& a;
    __device__ __forceinline__ KvBf16 rows(int slot, int kvh) const {
        return {a.kbase + (size_t)slot * a.slot_stride + (size_t)kvh * a.head_stride,
                a.vbase + (size_t)slot * a.slot_stride + (size_t)kvh * a.head_stride};
    }
};
// ... and the 8-bit slabs of a kv_bits = 8 batch (Kv8Layer): codes slot_stride / head_stride bytes apart, scale | bias words sb_*
struct Affine8Slabs {
    Kv8Layer kv;
    size_t slot_stride, head_stride, sb_slot_stride, sb_head_stride;
    __device__ __forceinline__ KvAffine8 rows(int slot, int kvh) const {
        const size_t at = (size_t)slot * slot_stride + (size_t)kvh * head_stride, sb = (size_t)slot * sb_slot_stride + (size_t)kvh * sb_head_stride;
        return {kv.kq + at, kv.vq + at, kv.ksb + sb, kv.vsb + sb};
    }
};

// block (r, kvh, split) on row r's own slab: K/V rows of the next step in flight while this step's are applied
template <int D, int GT, class Slabs>
__device__ __forceinline__ void attn_own_row(const BatchAttnArgs& a, const Slabs& slabs, unsigned char* smem, int r, int kvh, int split) {
    using Row = AttnRow<D, GT>;
    typedef decltype(slabs.rows(0, 0)) Src;
    constexpr int LPR = Row::LPR, STEP = Row::STEP;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int c = lane % LPR;           // 8-element chunk of the head dim owned by this lane
    const int sg = lane / LPR;          // token sub-group inside the wave
    const int G = a.H / a.Hkv;
    const int slot = a.row_slot[r];
    const int Tk = min(a.slots[slot].pos + 1, a.cap);
    const int t_begin = split * a.chunk;
    if (t_begin >= Tk) return;          // (block-uniform: past this sequence's end)
    const int t_end = min(Tk, t_begin + a.chunk);

    const Src src = slabs.rows(slot, kvh);

    typename Src::Raw kr[kUnroll], vr[kUnroll];
    int t0 = t_begin + wave * STEP;
    if (t0 < t_end) Row::issue_rows(kr, vr, src, t0, t_end, sg, c);

    Row row;
    row.begin(a.q + (size_t)r * a.H * D, D, a.scale, kvh, G, c);
    for (; t0 < t_end; t0 += STEP * kWaves) {
        float s[kUnroll][GT];
        float vf[kUnroll][8];
        row.template scores_of<Src>(kr, vr, t0, t_end, sg, NoMask{}, s, vf);
        if (t0 + STEP * kWaves < t_end) Row::issue_rows(kr, vr, src, t0 + STEP * kWaves, t_end, sg, c);
        row.update(s, vf);
    }
    row.finish(smem, a.ws_o, a.ws_ml, a.nsplit_cap, (size_t)r * a.H + kvh * G, G, split);
}

// The ungrouped launch, every row on its own slab: what a batch without forks runs
template <int D, int GT>
__global__ __launch_bounds__(kBlock) void batch_attn_kernel(const BatchAttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int r = blockIdx.x / a.Hkv, kvh = blockIdx.x % a.Hkv;
    attn_own_row<D, GT>(a, Bf16Slabs{a}, smem, r, kvh, blockIdx.y);
}

// ... and every row on its own 8-bit slab (a kv_bits = 8 batch): the same block over packed rows, nothing expanded in memory
template <int D, int GT>
__global__ __launch_bounds__(kBlock) void batch_attn_kv8_kernel(const BatchAttnArgs a, const Affine8Slabs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int r = blockIdx.x / a.Hkv, kvh = blockIdx.x % a.Hkv;
    attn_own_row<D, GT>(a, p, smem, r, kvh, blockIdx.y);
}

// ---- the same launch when listed rows share a prefix (omx_qwen3_batch_fork).  The rows whose owner is row r's and whose shared span
// reaches past split `split` form a group, in row order; with group_min members or more, every group_rows-th member's block takes
// that member and the next group_rows - 1: it loads the split's 256 K and 256 V rows of the KV head from the OWNER's slab into
// registers once -- a shared split is a whole chunk below every member's position -- and runs AttnRow over them once per member row,
// token -> (wave, sub-group, unroll slot) as in attn_own_row, so that each partial is the one batch_attn_kernel writes for that
// (row, KV head, split); the other members' blocks leave at once.  Every other block is attn_own_row.
template <int D, int GT>
__global__ __launch_bounds__(kBlock) void batch_attn_shared_kernel(const BatchSharedArgs sa) {
    const BatchAttnArgs& a = sa.a;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    using Row = AttnRow<D, GT>;
    constexpr int LPR = Row::LPR, TPW = Row::TPW, STEP = Row::STEP;
    constexpr int NIT = kChunk / (STEP * kWaves);   // steps of a wave over a whole chunk
    const int bk = blockIdx.x, split = blockIdx.y;
    const int r = bk / a.Hkv, kvh = bk % a.Hkv;
    const int t_begin = split * kChunk;
    unsigned members = 0;
    int before = 0;
    if (sa.grp_shared[r] > t_begin) {
        const int owner = sa.grp_owner[r];
        for (int r2 = 0; r2 < sa.T; ++r2)
            if (sa.grp_owner[r2] == owner && sa.grp_shared[r2] > t_begin) {
                members |= 1u << r2;
                before += r2 < r;
            }
    }
    if (__builtin_popcount(members) < sa.group_min) {
        attn_own_row<D, GT>(a, Bf16Slabs{a}, smem, r, kvh, split);
        return;
    }
    if (before % sa.group_rows) return;   // an earlier member's block takes this row

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int c = lane % LPR, sg = lane / LPR;
    const int G = a.H / a.Hkv;
    const int oslot = sa.grp_owner[r];
    const bf16_t* Kb = a.kbase + (size_t)oslot * a.slot_stride + (size_t)kvh * a.head_stride;
    const bf16_t* Vb = a.vbase + (size_t)oslot * a.slot_stride + (size_t)kvh * a.head_stride;
    const int t_end = t_begin + kChunk;  // <= shared_len <= pos of every member
    u32x4 kr[NIT][kUnroll], vr[NIT][kUnroll];
#pragma unroll
    for (int it = 0; it < NIT; ++it)
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int tc = t_begin + (it * kWaves + wave) * STEP + u * TPW + sg;
            kr[it][u] = *reinterpret_cast<const u32x4*>(Kb + (size_t)tc * D + c * 8);
            vr[it][u] = *reinterpret_cast<const u32x4*>(Vb + (size_t)tc * D + c * 8);
        }
    int take = sa.group_rows;
    for (int r2 = r; r2 < sa.T && take > 0; ++r2) {
        if (!((members >> r2) & 1u)) continue;
        --take;
        Row row;
        row.begin(a.q + (size_t)r2 * a.H * D, D, a.scale, kvh, G, c);
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            // (the rows stay packed between the member rows: unpacked once for all of them they would not fit the register file)
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) asm volatile("" : "+v"(kr[it][u]), "+v"(vr[it][u]));
            float s[kUnroll][GT];
            float vf[kUnroll][8];
            row.scores(kr[it], vr[it], t_begin + (it * kWaves + wave) * STEP, t_end, sg, NoMask{}, s, vf);
            row.update(s, vf);
        }
        row.finish(smem, a.ws_o, a.ws_ml, a.nsplit_cap, (size_t)r2 * a.H + kvh * G, G, split);
        __syncthreads();   // the merge has read the LDS area before the next row parks in it
    }
}

// merge of a (row, head)'s splits: out[d] = sum_i e^{m_i - M} o_i[d] / sum_i e^{m_i - M} l_i over the ceil(len / chunk) splits of ITS
// sequence, added in split order, rounded once to bf16.  One block per (row, head), one thread per d.
template <int D>
__global__ __launch_bounds__(D) void batch_attn_merge_kernel(const BatchAttnArgs a) {
    const size_t head = blockIdx.x;
    const int r = (int)(head / a.H), d = threadIdx.x;
    const int Tk = min(a.slots[a.row_slot[r]].pos + 1, a.cap);
    const int ns = (Tk + a.chunk - 1) / a.chunk;
    const float* ml = a.ws_ml + head * a.nsplit_cap * 2;
    const float* src = a.ws_o + head * a.nsplit_cap * D + d;
    float M = -INFINITY;
    for (int i = 0; i < ns; ++i) M = fmaxf(M, ml[2 * i]);
    float L = 0.f, acc = 0.f;
    for (int i = 0; i < ns; ++i) {
        const float mi = ml[2 * i];
        const float f = (mi == -INFINITY) ? 0.f : __expf(mi - M);
        L = fmaf(f, ml[2 * i + 1], L);
        acc = fmaf(f, src[(size_t)i * D], acc);
    }
    a.out[head * D + d] = f32_to_bf16(acc / L);
}

// ---- per-row sampler + state advance.  One block per row: the row's logits are kept as its slot's last logits, the token is the
// argmax (inv_temp 0) or categorical(logits / T) -- logits * (1/T) + Gumbel noise, the noise of vocabulary entry v being word v of a
// V-word draw from the NEXT key of the slot's own sequence (RandomState::next, the rule of rng_next_kernel + sample_noise_kernel,
// random.hip) -- first index winning a tie; then ring[step][row] = token, pending[s] = token, pos[s] += 1.
struct BatchSampleArgs {
    const bf16_t* rows;        // [T, V] logits of this step
    bf16_t* slot_logits;       // [n_slots, V]
    BatchSlot* slots;
    const int* row_slot;
    uint32_t* ring;            // this step's [T] entries
    int V;
    float inv_temp[kMaxSlots]; // per row; 0 = greedy
};

__global__ __launch_bounds__(1024) void batch_sample_kernel(const BatchSampleArgs a) {
    __shared__ unsigned long long red[16];
    const int r = blockIdx.x, slot = a.row_slot[r];
    BatchSlot* S = a.slots + slot;
    const float it = a.inv_temp[r];
    const bf16_t* row = a.rows + (size_t)r * a.V;
    bf16_t* keep = a.slot_logits + (size_t)slot * a.V;
    uint32_t s0 = 0, s1 = 0, k0 = 0, k1 = 0;
    if (it != 0.f) {   // (state, key) = split(state, 2)
        const uint32_t c0 = S->rng[0], c1 = S->rng[1];
        threefry2x32(c0, c1, 0u, 2u, s0, k0);
        threefry2x32(c0, c1, 1u, 3u, s1, k1);
    }
    __syncthreads();   // every thread has read the state before thread 0 replaces it
    unsigned long long best = 0;
    for (int v = threadIdx.x; v < a.V; v += blockDim.x) {
        const bf16_t raw = row[v];
        keep[v] = raw;
        float x = bf16_to_f32(raw);
        if (it != 0.f) x = x * it + gumbel_from_word(random_word(k0, k1, (uint64_t)v, (uint64_t)a.V));
        const unsigned long long kx = sample_key(x, (uint32_t)v);
        best = kx > best ? kx : best;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(best, o, 64);
        best = other > best ? other : best;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (unsigned w = 1; w < blockDim.x / 64; ++w) best = red[w] > best ? red[w] : best;
        const uint32_t token = ~(uint32_t)(best & 0xFFFFFFFFull);
        a.ring[r] = token;
        S->pending = token;
        S->pos += 1;
        if (it != 0.f) { S->rng[0] = s0; S->rng[1] = s1; S->rng[2] = k0; S->rng[3] = k1; }
    }
}

}  // namespace

int launch_batch_embed(omx_qwen3 m, const RaggedRows& rag, int T, hipStream_t s) {
    const omx_qwen3_config& c = m->cfg;
    const int hd = c.hidden_size;
#define OMX_BATCH_EMB(B) \
    case B: batch_embed_kernel<B><<<T, 256, 0, s>>>(m->pf_h, m->q_embed.w, m->q_embed.scales, m->q_embed.biases, rag.slots, rag.row_slot, hd, m->q_embed.group); break;
    switch (c.quant_bits ? m->q_embed.bits : 0) {      // (a packed table: the embedding's own format)
        case 0: batch_embed_kernel<0><<<T, 256, 0, s>>>(m->pf_h, m->embed, nullptr, nullptr, rag.slots, rag.row_slot, hd, 0); break;
        OMX_BATCH_EMB(2) OMX_BATCH_EMB(3) OMX_BATCH_EMB(4) OMX_BATCH_EMB(5) OMX_BATCH_EMB(6) OMX_BATCH_EMB(8)
        default: return set_error("batch embed: quantization bits %d unsupported", m->q_embed.bits);
    }
#undef OMX_BATCH_EMB
    OMX_LAUNCH_CHECK();
    return 0;
}

int launch_batch_attention(omx_qwen3 m, int layer, const RaggedRows& rag, int T, hipStream_t s) {
    const int D = m->cfg.head_dim, H = m->H, Hkv = m->Hkv, G = H / Hkv;
    OMX_REQUIRE(G >= 1 && G <= 8, "batch attention: %d query heads per KV head unsupported (max 8)", G);
    OMX_REQUIRE(rag.nsplit >= 1 && rag.nsplit <= rag.nsplit_cap, "batch attention: %d splits of %d", rag.nsplit, rag.nsplit_cap);
    BatchAttnArgs a = {};
    a.q = m->pf_qt;
    if (!rag.kv8) { a.kbase = rag.kbase[layer]; a.vbase = rag.vbase[layer]; }
    a.slot_stride = rag.slot_stride; a.head_stride = (size_t)rag.cap * D;
    a.slots = rag.slots; a.row_slot = rag.row_slot;
    a.H = H; a.Hkv = Hkv; a.cap = rag.cap; a.chunk = rag.chunk; a.nsplit_cap = rag.nsplit_cap;
    a.scale = 1.0f / sqrtf((float)D);
    a.ws_o = rag.ws_o; a.ws_ml = rag.ws_ml;
    a.out = m->pf_attn;
    BatchSharedArgs sa = {};
    if (rag.grouped) {
        sa.a = a;
        sa.T = T; sa.group_min = rag.group_min; sa.group_rows = rag.group_rows;
        for (int r = 0; r < kMaxSlots; ++r) {
            sa.grp_owner[r] = r < T ? rag.grp_owner[r] : -1;
            sa.grp_shared[r] = r < T ? rag.grp_shared[r] : 0;
        }
    }
    OMX_REQUIRE(!rag.grouped || (rag.chunk == kChunk && rag.group_min >= 2 && rag.group_rows >= 1), "batch attention: grouped splits of %d tokens, "
                "groups from %d members, %d rows per block", rag.chunk, rag.group_min, rag.group_rows);
    const dim3 grid(T * Hkv, rag.nsplit), block(kBlock);
    const int gt = G <= 1 ? 1 : G <= 2 ? 2 : G <= 4 ? 4 : 8;
    if (rag.kv8) {   // the same grid and merge over the 8-bit slabs
        OMX_REQUIRE(!rag.grouped, "batch attention: the grouped read is not built for 8-bit K/V slabs");
        const Affine8Slabs p = {rag.kv8[layer], rag.slot_stride, (size_t)rag.cap * D, rag.sb_stride, (size_t)rag.cap * (D / 64)};
#define OMX_BATCH_ATTN8_CASE(DD, GG)                                                                    \
    if (D == DD && gt == GG) {                                                                          \
        const size_t shmem = AttnRow<DD, GG>::SMEM_BYTES;                                               \
        if (shmem > 48 * 1024)                                                                          \
            OMX_HIP_CHECK(hipFuncSetAttribute((const void*)batch_attn_kv8_kernel<DD, GG>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem)); \
        batch_attn_kv8_kernel<DD, GG><<<grid, block, shmem, s>>>(a, p);                                 \
        OMX_LAUNCH_CHECK();                                                                             \
        batch_attn_merge_kernel<DD><<<T * H, DD, 0, s>>>(a);                                            \
        OMX_LAUNCH_CHECK();                                                                             \
        return 0;                                                                                       \
    }
        OMX_BATCH_ATTN8_CASE(128, 1) OMX_BATCH_ATTN8_CASE(128, 2) OMX_BATCH_ATTN8_CASE(128, 4) OMX_BATCH_ATTN8_CASE(128, 8)
        OMX_BATCH_ATTN8_CASE(64, 1) OMX_BATCH_ATTN8_CASE(64, 2) OMX_BATCH_ATTN8_CASE(64, 4) OMX_BATCH_ATTN8_CASE(64, 8)
#undef OMX_BATCH_ATTN8_CASE
        return set_error("batch attention: head_dim %d unsupported (64 or 128)", D);
    }
#define OMX_BATCH_ATTN_CASE(DD, GG)                                                                     \
    if (D == DD && gt == GG) {                                                                          \
        const size_t shmem = AttnRow<DD, GG>::SMEM_BYTES;                                               \
        const void* fn = rag.grouped ? (const void*)batch_attn_shared_kernel<DD, GG> : (const void*)batch_attn_kernel<DD, GG>; \
        if (shmem > 48 * 1024)                                                                          \
            OMX_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem)); \
        if (rag.grouped) /* rows that share a prefix: the same grid, grouped blocks over the shared splits */ \
            batch_attn_shared_kernel<DD, GG><<<grid, block, shmem, s>>>(sa);                            \
        else                                                                                            \
            batch_attn_kernel<DD, GG><<<grid, block, shmem, s>>>(a);                                    \
        OMX_LAUNCH_CHECK();                                                                             \
        batch_attn_merge_kernel<DD><<<T * H, DD, 0, s>>>(a);                                            \
        OMX_LAUNCH_CHECK();                                                                             \
        return 0;                                                                                       \
    }
    OMX_BATCH_ATTN_CASE(128, 1) OMX_BATCH_ATTN_CASE(128, 2) OMX_BATCH_ATTN_CASE(128, 4) OMX_BATCH_ATTN_CASE(128, 8)
    OMX_BATCH_ATTN_CASE(64, 1) OMX_BATCH_ATTN_CASE(64, 2) OMX_BATCH_ATTN_CASE(64, 4) OMX_BATCH_ATTN_CASE(64, 8)
#undef OMX_BATCH_ATTN_CASE
    return set_error("batch attention: head_dim %d unsupported (64 or 128)", D);
}

}  // namespace omx

struct omx_qwen3_batch_ {
    omx_qwen3 m = nullptr;
    int n_slots = 0, cap = 0;
    std::vector<bf16_t*> kbase, vbase;                 // per layer: [n_slots][Hkv, cap, D]
    std::vector<bf16_t*> slot_k[kMaxSlots], slot_v[kMaxSlots];   // the same slabs per slot, as the prompt pass takes them (KvSlabs)
    size_t slot_stride = 0;
    // kv_bits = 8: no bf16 slabs; per layer the 8-bit slabs of all slots (layer8, Kv8Layer: slot s at + s * slot_stride codes and
    // + s * sb_stride words) and the same per slot (slot8); ONE bf16 staging pair [Hkv, cap, D] every prompt pass attends over, named
    // once per layer for KvSlabs (stage_k / stage_v); dbg_slots: the positions omx_qwen3_batch_debug_attention reads instead of `slots`
    int kv_bits = 0;
    std::vector<Kv8Layer> layer8, slot8[kMaxSlots];
    size_t sb_stride = 0;
    std::vector<bf16_t*> stage_k, stage_v;
    size_t kv_bytes = 0;                               // bytes of K/V storage (slabs only)
    BatchSlot* slots = nullptr;                        // device [n_slots]
    BatchSlot* dbg_slots = nullptr;
    int* row_slot = nullptr;                           // device [kMaxSlots]: the rows of the call in flight
    bf16_t *step_logits = nullptr, *slot_logits = nullptr;   // [kMaxSlots, V] rows of a step; [n_slots, V] kept per slot
    uint32_t* ring = nullptr;                          // [kRingSteps][kMaxSlots]
    float *ws_o = nullptr, *ws_ml = nullptr;           // attention partials
    int nsplit_cap = 0;
    // host mirror: a step advances every listed slot by exactly one token, so the positions never have to be read back
    int pos[kMaxSlots] = {};
    bool prefilled[kMaxSlots] = {};
    float temperature[kMaxSlots] = {};
    // per-slot filters (omx_qwen3_batch_set_sampling): the settings, and `filtered` = they prune or penalise (else the plain sampler).
    // seen [n_slots, V] bytes, there from the first penalty on: the tokens a slot sampled since its last prefill, marked by the step
    // for slots with a penalty on.  sel: one selection scratch per ROW of a step.  decoded: steps a slot took since its last prefill
    omx_sampling sampling[kMaxSlots];
    bool filtered[kMaxSlots] = {};
    uint8_t* seen = nullptr;
    uint8_t* sel = nullptr;
    int decoded[kMaxSlots] = {};
    // shared prefixes (omx_qwen3_batch_fork), the host's copy of the slot table's owner / shared_len: rows [0, shared_len[s]) of slot s
    // and of slot owner[s] hold the same bits, and shared_len[s] <= pos[s] rounded down to kChunk
    int owner[kMaxSlots] = {}, shared_len[kMaxSlots] = {};
    int share_stage[kMaxSlots][2] = {};                // what set_share copies to the table from: alive until the caller synchronises
    bool share_on = true;                              // OMX_BATCH_SHARE=0: forks copy, nothing is read through an owner
    // OMX_BATCH_SHARE_MIN / _ROWS: grouped blocks from this many members on; member rows per grouped block.  The grouped block lost to
    // the rows' own blocks at every group size measured (2, 4, 8 members), so by default no group is large enough
    int group_min = kMaxSlots + 1, group_rows = 8;
    float last_decode_ms = 0.f;                        // device time of the last decode call's steps (the model's event pair)
    // per-token log-probabilities (omx_qwen3_batch_set_logprobs): lp_top = -1 off, else the alternatives per token.  The rings are laid
    // out as the token ring is ([kRingSteps][kMaxSlots] and the same x lp_top); slot_lp / slot_ids / slot_top keep every slot's last
    // values ([n_slots] and [n_slots, lp_top]), written by the same merge launch.  All allocated at the first switch-on, for
    // OMX_LOGPROBS_MAX_TOP, with the scratch of the two launches over kMaxSlots rows.  lp_valid: the slot has sampled since the setting changed
    int lp_top = -1;
    float *lp_ring = nullptr, *top_lp_ring = nullptr, *slot_lp = nullptr, *slot_top = nullptr;
    uint32_t *top_id_ring = nullptr, *slot_ids = nullptr;
    uint8_t* lp_scratch = nullptr;
    bool lp_valid[kMaxSlots] = {};
    std::vector<void*> owned;
};

namespace {

template <class T>
int batch_alloc(omx_qwen3_batch b, T** p, size_t n) {
    void* q = nullptr;
    OMX_HIP_CHECK(hipMalloc(&q, n * sizeof(T) + 64));
    OMX_HIP_CHECK(hipMemsetAsync(q, 0, n * sizeof(T) + 64, b->m->stream));
    *p = (T*)q;
    b->owned.push_back(q);
    return 0;
}

uint8_t* seen_row(omx_qwen3_batch b, int slot) {
    return b->seen && sampling_penalised(b->sampling[slot]) ? b->seen + (size_t)slot * b->m->V : nullptr;
}

int clear_history(omx_qwen3_batch b, int slot) {
    if (b->seen) OMX_HIP_CHECK(hipMemsetAsync(b->seen + (size_t)slot * b->m->V, 0, (size_t)b->m->V, b->m->stream));
    return 0;
}

// after the sampler: the log-probabilities of the M tokens it just wrote at ring_at (and the rows' alternatives) over the same raw
// rows, into the rings at the same offset and into the slots' last values
int batch_logprobs(omx_qwen3_batch b, const bf16_t* logits, const int* rows, int M, const uint32_t* ring_at) {
    if (b->lp_top < 0) return 0;
    const size_t at = (size_t)(ring_at - b->ring), top = (size_t)b->lp_top;
    LogprobTopOut o = {};
    o.logprobs = b->lp_ring + at; o.top_ids = b->top_id_ring + at * top; o.top_lp = b->top_lp_ring + at * top;
    o.row_slot = b->row_slot; o.slot_lp = b->slot_lp; o.slot_ids = b->slot_ids; o.slot_top = b->slot_top;
    if (launch_logprob_top(o, b->lp_scratch, logits, b->m->V, ring_at, M, b->m->V, b->lp_top, b->m->stream)) return 1;
    for (int r = 0; r < M; ++r) b->lp_valid[rows[r]] = true;
    return 0;
}

int batch_sample_rows(omx_qwen3_batch b, const bf16_t* logits, const int* rows, int M, uint32_t* ring_at);

// [per-row sample + advance] of logits[M, V] for slots rows[0..M) (row_slot already on the device): the plain kernel while no listed
// slot filters, else every row under its own slot's rule (launch_batch_filtered; a plain row draws the same token there); then,
// where asked for, the drawn tokens' log-probabilities
int batch_sample(omx_qwen3_batch b, const bf16_t* logits, const int* rows, int M, uint32_t* ring_at) {
    return batch_sample_rows(b, logits, rows, M, ring_at) || batch_logprobs(b, logits, rows, M, ring_at);
}

int batch_sample_rows(omx_qwen3_batch b, const bf16_t* logits, const int* rows, int M, uint32_t* ring_at) {
    hipStream_t s = b->m->stream;
    const int V = b->m->V;
    bool any = false;
    for (int r = 0; r < M; ++r) any = any || b->filtered[rows[r]];
    if (!any) {
        BatchSampleArgs a = {};
        a.rows = logits; a.slot_logits = b->slot_logits; a.slots = b->slots; a.row_slot = b->row_slot; a.ring = ring_at; a.V = V;
        for (int r = 0; r < M; ++r) a.inv_temp[r] = b->temperature[rows[r]] == 0.f ? 0.f : 1.0f / b->temperature[rows[r]];
        batch_sample_kernel<<<M, 1024, 0, s>>>(a);
        OMX_LAUNCH_CHECK();
        return 0;
    }
    BatchFilterArgs a = {};
    a.rows = logits; a.slot_logits = b->slot_logits; a.slots = b->slots; a.row_slot = b->row_slot; a.ring = ring_at; a.ws = b->sel; a.V = V;
    for (int r = 0; r < M; ++r) a.row[r] = batch_filter_row(b->sampling[rows[r]], V, seen_row(b, rows[r]));
    return launch_batch_filtered(a, M, s);
}

// [final RMSNorm] -> [lm_head over M rows] -> [per-row sample + advance]: rows x[M, hidden] of slots row_slot[0..M) (already on the device)
int batch_head_and_sample(omx_qwen3_batch b, const bf16_t* x, const int* rows, int M, uint32_t* ring_at) {
    omx_qwen3 m = b->m;
    hipStream_t s = m->stream;
    const int hd = m->cfg.hidden_size, V = m->V;
    if (m->cfg.quant_bits) {   // the packed head (or the tied q_embed table), the final RMSNorm as its prologue
        QGemvArgs a = {};
        a.m[0] = m->q_head; a.m[0].n = V; a.N = V; a.K = hd; a.group = m->q_head.group;   // the head's own format
        a.x = x; a.norm_w = m->final_norm; a.eps = m->cfg.rms_norm_eps; a.out = b->step_logits;
        if (packed_rows(a, M, nullptr, m->q_head.bits, PRO_RMSNORM, EPI_STORE, s)) return 1;
    } else {
        if (omx_rms_norm(m->pf_xn, x, m->final_norm, M, hd, m->cfg.rms_norm_eps, OMX_BFLOAT16, s)) return 1;
        if (launch_gemm_bf16(b->step_logits, m->pf_xn, m->lm_head, nullptr, M, V, hd, s)) return 1;
    }
    return batch_sample(b, b->step_logits, rows, M, ring_at);
}

int write_slot(omx_qwen3_batch b, int slot, const BatchSlot& v, size_t bytes) {   // the leading `bytes` of the entry: pos | pending
    OMX_HIP_CHECK(hipMemcpyAsync(b->slots + slot, &v, bytes, hipMemcpyHostToDevice, b->m->stream));
    OMX_HIP_CHECK(hipStreamSynchronize(b->m->stream));
    return 0;
}

// owner | shared_len of a slot, host copy and device table (the caller synchronises)
int set_share(omx_qwen3_batch b, int slot, int owner, int shared_len) {
    if (b->owner[slot] == owner && b->shared_len[slot] == shared_len) return 0;
    b->owner[slot] = owner;
    b->shared_len[slot] = shared_len;
    b->share_stage[slot][0] = owner;
    b->share_stage[slot][1] = shared_len;
    OMX_HIP_CHECK(hipMemcpyAsync(&b->slots[slot].owner, b->share_stage[slot], 8, hipMemcpyHostToDevice, b->m->stream));
    return 0;
}

// slot's cache now ends at `pos` (trim; 0: reset, or a prompt from position 0): what it shares, and what others share with it, ends
// at the chunk boundary at or below -- the rows above are about to be overwritten in ONE of the copies
int lower_share(omx_qwen3_batch b, int slot, int pos) {
    const int lim = pos / kChunk * kChunk;
    if (b->shared_len[slot] > lim && set_share(b, slot, lim ? b->owner[slot] : slot, lim)) return 1;
    for (int c = 0; c < b->n_slots; ++c)
        if (c != slot && b->owner[c] == slot && b->shared_len[c] > lim && set_share(b, c, lim ? slot : c, lim)) return 1;
    return 0;
}

// the ragged launches' view of the batch, for sequences of up to `longest` tokens: slabs, slot table, workspace; no groups
RaggedRows batch_rows(omx_qwen3_batch b, int longest) {
    RaggedRows rag = {};
    rag.slots = b->slots; rag.row_slot = b->row_slot;
    rag.kbase = b->kbase.data(); rag.vbase = b->vbase.data();
    rag.slot_stride = b->slot_stride; rag.cap = b->cap;
    rag.chunk = kChunk; rag.nsplit_cap = b->nsplit_cap;
    rag.nsplit = (longest + kChunk - 1) / kChunk;
    rag.ws_o = b->ws_o; rag.ws_ml = b->ws_ml;
    rag.kv8 = b->kv_bits ? b->layer8.data() : nullptr;
    rag.sb_stride = b->sb_stride;
    return rag;
}

int env_int(const char* name, int dflt, int lo, int hi) {
    const char* e = getenv(name);
    if (!e || !*e) return dflt;
    return std::min(hi, std::max(lo, atoi(e)));
}

}  // namespace

#define OMX_BATCH_SLOT(fn)                                                                                \
    OMX_REQUIRE(b, fn ": null batch");                                                                    \
    OMX_REQUIRE(slot >= 0 && slot < b->n_slots, fn ": slot %d out of range (0..%d)", slot, b->n_slots - 1)

extern "C" {

int omx_qwen3_batch_create(omx_qwen3_batch* out, omx_qwen3 m, int n_slots, int max_context) {
    return omx_qwen3_batch_create_kv(out, m, n_slots, max_context, 0);
}

int omx_qwen3_batch_create_kv(omx_qwen3_batch* out, omx_qwen3 m, int n_slots, int max_context, int kv_bits) {
    OMX_REQUIRE(out && m, "omx_qwen3_batch_create: null argument");
    OMX_REQUIRE(kv_bits == 0 || kv_bits == 8, "omx_qwen3_batch_create_kv: kv_bits %d unsupported (0 = bf16 K/V slabs, 8 = 8-bit MLX affine "
                "rows of group 64)", kv_bits);
    OMX_REQUIRE(n_slots >= 1 && n_slots <= kMaxSlots, "omx_qwen3_batch_create: %d slots (1..%d)", n_slots, kMaxSlots);
    const omx_qwen3_config& c = m->cfg;
    OMX_REQUIRE(c.num_experts == 0, "omx_qwen3_batch_create: models with experts (MoE) are not supported; dense models only");
    OMX_REQUIRE(m->allreduce == nullptr && c.tp_size <= 1 && c.ep_size <= 1,
                "omx_qwen3_batch_create: tensor / expert parallel models are not supported (single-rank models only)");
    OMX_REQUIRE(!c.float16_weights, "omx_qwen3_batch_create: dense float16 models (float16_weights) are not supported; batched decode runs "
                "on bf16 weights or bf16-scale packed weights");
    OMX_REQUIRE(!c.quant_scales_f16,
                "omx_qwen3_batch_create: float16 triplets (scales_dtype float16) are not supported on packed models; bf16 scales only");
    OMX_REQUIRE(!m->filter_on, "omx_qwen3_batch_create: filtered sampling (top-k / top-p / penalties, omx_qwen3_set_sampling) is on: a batch "
                "slot draws from unfiltered rows; call omx_qwen3_set_sampler first");
    OMX_REQUIRE(m->H / m->Hkv <= 8, "omx_qwen3_batch_create: %d query heads per KV head unsupported (max 8)", m->H / m->Hkv);
    OMX_REQUIRE(max_context >= 0, "omx_qwen3_batch_create: max_context %d must be >= 0 (0 = the model's)", max_context);
    const int step = 256;   // cache.rs:110-117
    const int cap = max_context > 0 ? (max_context + step - 1) / step * step : m->cap;
    OMX_REQUIRE(cap <= m->cap, "omx_qwen3_batch_create: max_context %d exceeds the model's %d (its RoPE tables end there)", max_context, m->cap);
    omx_qwen3_batch b = new omx_qwen3_batch_();
    b->m = m;
    b->n_slots = n_slots;
    b->cap = cap;
    for (int s = 0; s < kMaxSlots; ++s) b->sampling[s] = {0.f, 0, 1.f, 1.f, 0.f};
    const int D = c.head_dim, L = c.num_hidden_layers, V = m->V;
    b->kv_bits = kv_bits;
    b->slot_stride = (size_t)m->Hkv * cap * D;
    b->sb_stride = (size_t)m->Hkv * cap * (D / 64);
    int rc = 0;
    if (kv_bits == 0) {
        b->kbase.resize(L);
        b->vbase.resize(L);
    }
    for (int l = 0; l < L && !rc && kv_bits == 0; ++l) {
        rc = batch_alloc(b, &b->kbase[l], b->slot_stride * n_slots) || batch_alloc(b, &b->vbase[l], b->slot_stride * n_slots);
        b->kv_bytes += 2 * b->slot_stride * n_slots * sizeof(bf16_t);
        for (int s = 0; s < n_slots && !rc; ++s) {
            b->slot_k[s].push_back(b->kbase[l] + (size_t)s * b->slot_stride);
            b->slot_v[s].push_back(b->vbase[l] + (size_t)s * b->slot_stride);
        }
    }
    for (int l = 0; l < L && !rc && kv_bits == 8; ++l) {
        Kv8Layer q = {};
        rc = batch_alloc(b, &q.kq, b->slot_stride * n_slots) || batch_alloc(b, &q.vq, b->slot_stride * n_slots) ||
             batch_alloc(b, &q.ksb, b->sb_stride * n_slots) || batch_alloc(b, &q.vsb, b->sb_stride * n_slots);
        b->kv_bytes += 2 * (b->slot_stride + b->sb_stride * sizeof(uint32_t)) * n_slots;
        b->layer8.push_back(q);
        for (int s = 0; s < n_slots && !rc; ++s)
            b->slot8[s].push_back({q.kq + (size_t)s * b->slot_stride, q.vq + (size_t)s * b->slot_stride, q.ksb + (size_t)s * b->sb_stride,
                                   q.vsb + (size_t)s * b->sb_stride});
    }
    if (kv_bits == 8 && !rc) {
        bf16_t *sk = nullptr, *sv = nullptr;
        rc = batch_alloc(b, &sk, b->slot_stride) || batch_alloc(b, &sv, b->slot_stride);
        b->stage_k.assign(L, sk);
        b->stage_v.assign(L, sv);
    }
    b->nsplit_cap = cap / kChunk;
    rc = rc || batch_alloc(b, &b->slots, (size_t)n_slots) || batch_alloc(b, &b->dbg_slots, (size_t)n_slots) || batch_alloc(b, &b->row_slot, (size_t)kMaxSlots) ||
         batch_alloc(b, &b->step_logits, (size_t)kMaxSlots * V) || batch_alloc(b, &b->slot_logits, (size_t)n_slots * V) ||
         batch_alloc(b, &b->ring, (size_t)kRingSteps * kMaxSlots) ||
         batch_alloc(b, &b->ws_o, (size_t)kMaxSlots * m->H * b->nsplit_cap * D) || batch_alloc(b, &b->ws_ml, (size_t)kMaxSlots * m->H * b->nsplit_cap * 2);
    // every slot starts with the key sequence of seed 0, like a model whose sampler was set to (T, 0)
    for (int s = 0; s < n_slots && !rc; ++s) rc = omx_random_key(b->slots[s].rng, 0, (omx_stream)m->stream);
    for (int s = 0; s < n_slots && !rc; ++s) {
        b->owner[s] = -1;
        rc = set_share(b, s, s, 0);
    }
    b->share_on = env_int("OMX_BATCH_SHARE", 1, 0, 1) != 0;
    b->group_min = env_int("OMX_BATCH_SHARE_MIN", b->group_min, 2, kMaxSlots + 1);
    b->group_rows = env_int("OMX_BATCH_SHARE_ROWS", b->group_rows, 1, kMaxSlots);
    if (!rc && hipStreamSynchronize(m->stream) != hipSuccess) rc = set_error("omx_qwen3_batch_create: stream synchronise failed");
    if (rc) {
        omx_qwen3_batch_destroy(b);
        return 1;
    }
    *out = b;
    return 0;
}

int omx_qwen3_batch_destroy(omx_qwen3_batch b) {
    if (!b) return 0;
    if (b->m && b->m->stream) (void)hipStreamSynchronize(b->m->stream);
    for (void* p : b->owned) (void)hipFree(p);
    delete b;
    return 0;
}

int omx_qwen3_batch_set_sampler(omx_qwen3_batch b, int slot, float temperature, uint64_t seed) {
    OMX_BATCH_SLOT("omx_qwen3_batch_set_sampler");
    OMX_REQUIRE(temperature >= 0.f && temperature == temperature, "omx_qwen3_batch_set_sampler: temperature %f must be >= 0", (double)temperature);
    if (omx_random_key(b->slots[slot].rng, seed, (omx_stream)b->m->stream)) return 1;
    if (clear_history(b, slot)) return 1;
    OMX_HIP_CHECK(hipStreamSynchronize(b->m->stream));
    b->temperature[slot] = temperature;
    b->sampling[slot] = {temperature, 0, 1.f, 1.f, 0.f};   // the plain sampler: every filter and penalty off
    b->filtered[slot] = false;
    return 0;
}

int omx_qwen3_batch_set_sampling(omx_qwen3_batch b, int slot, const omx_sampling* p, uint64_t seed) {
    OMX_BATCH_SLOT("omx_qwen3_batch_set_sampling");
    const int V = b->m->V;
    if (check_sampling("omx_qwen3_batch_set_sampling", p, V)) return 1;
    const bool on = sampling_filters(*p, V);
    if (on && sampling_penalised(*p) && !b->seen && batch_alloc(b, &b->seen, (size_t)b->n_slots * V)) return 1;
    if (on && !b->sel && batch_alloc(b, &b->sel, (size_t)kMaxSlots * sample_select_ws_bytes())) return 1;
    if (omx_random_key(b->slots[slot].rng, seed, (omx_stream)b->m->stream)) return 1;
    if (clear_history(b, slot)) return 1;
    OMX_HIP_CHECK(hipStreamSynchronize(b->m->stream));
    b->temperature[slot] = p->temperature;
    b->sampling[slot] = *p;
    b->filtered[slot] = on;
    return 0;
}

// omx_qwen3_batch_prefill, and omx_qwen3_batch_prefill_embeds (span: the caller's rows over the gathered ones, as omx_qwen3_prefill_embeds)
static int batch_prefill_prompt(omx_qwen3_batch b, int slot, const uint32_t* prompt, int n_prompt, uint32_t* first_token, const RowSpan* span) {
    OMX_BATCH_SLOT("omx_qwen3_batch_prefill");
    OMX_REQUIRE(prompt && first_token, "omx_qwen3_batch_prefill: null argument");
    OMX_REQUIRE(n_prompt >= 1, "omx_qwen3_batch_prefill: empty prompt");
    omx_qwen3 m = b->m;
    const int off = b->pos[slot];
    OMX_REQUIRE(off + n_prompt + 1 <= b->cap, "omx_qwen3_batch_prefill: %d cached + %d prompt tokens exceed max_context %d", off, n_prompt, b->cap);
    for (int i = 0; i < n_prompt; ++i)
        OMX_REQUIRE(prompt[i] < (uint32_t)m->cfg.vocab_size, "omx_qwen3_batch_prefill: token id %u out of range (vocab %d)", prompt[i], m->cfg.vocab_size);
    OMX_REQUIRE(n_prompt <= m->prompt_cap, "omx_qwen3_batch_prefill: prompt of %d tokens exceeds the model's prompt buffer (%d)", n_prompt, m->prompt_cap);
    OMX_REQUIRE(!m->filter_on, "omx_qwen3_batch_prefill: filtered sampling (omx_qwen3_set_sampling) is on; call omx_qwen3_set_sampler first");
    // a handful of rows of a packed model: the packed rows launches, as the verify pass (nothing dequantised); else the prompt pass's GEMMs
    const bool prow = m->cfg.quant_bits != 0 && n_prompt <= 8;
    // (those launches gather and unpack the embedding rows in their own form: there is no row buffer to put the caller's rows in)
    OMX_REQUIRE(!(span && prow), "InvalidConfig: omx_qwen3_batch_prefill_embeds: a packed model sends prompts of 8 rows or fewer through the "
                "few-row packed launches, which cannot take embedding rows (%d rows); pass at least 9", n_prompt);
    if (resolve_weights(m)) return 1;
    if (off == 0 && lower_share(b, slot, 0)) return 1;   // rows from 0 on are rewritten: nobody shares them any more
    if (clear_history(b, slot)) return 1;                // the penalties see the tokens sampled since THIS prefill (as omx_qwen3_prefill)
    hipStream_t s = m->stream;
    if (m->cfg.quant_bits && !prow) dq_cache_prepare(m);
    if (prefill_reserve(m, n_prompt, !prow)) return 1;
    OMX_HIP_CHECK(hipMemcpyAsync(m->prompt_dev, prompt, (size_t)n_prompt * 4, hipMemcpyHostToDevice, s));
    const KvSlabs kv = b->kv_bits ? KvSlabs{b->stage_k.data(), b->stage_v.data(), b->cap, b->slot8[slot].data()}
                                  : KvSlabs{b->slot_k[slot].data(), b->slot_v[slot].data(), b->cap};
    if (prefill_prefix_batched(m, n_prompt, off, nullptr, /*full_last=*/true, prow, &kv, nullptr, span)) return 1;
    // the last row through the head and the slot's sampler: the sample launch turns pos = off + n - 1 into off + n
    BatchSlot v = {};
    v.pos = off + n_prompt - 1;
    v.pending = prompt[n_prompt - 1];
    OMX_HIP_CHECK(hipMemcpyAsync(b->slots + slot, &v, 8, hipMemcpyHostToDevice, s));
    OMX_HIP_CHECK(hipMemcpyAsync(b->row_slot, &slot, 4, hipMemcpyHostToDevice, s));
    if (batch_head_and_sample(b, m->pf_h + (size_t)(n_prompt - 1) * m->cfg.hidden_size, &slot, 1, b->ring)) return 1;
    OMX_HIP_CHECK(hipMemcpyAsync(first_token, b->ring, 4, hipMemcpyDeviceToHost, s));
    OMX_HIP_CHECK(hipStreamSynchronize(s));
    b->pos[slot] = off + n_prompt;
    b->prefilled[slot] = true;
    b->decoded[slot] = 0;
    return 0;
}

int omx_qwen3_batch_prefill(omx_qwen3_batch b, int slot, const uint32_t* prompt, int n_prompt, uint32_t* first_token) {
    return batch_prefill_prompt(b, slot, prompt, n_prompt, first_token, nullptr);
}

/* omx_qwen3_batch_prefill with rows [first_row, first_row + n_rows) of the pass supplied by the caller (omx_qwen3_prefill_embeds' span, its
 * refusals and their texts): what a multimodal model needs to decode several clips together.  The slot's cache append (bf16 or kv_bits = 8),
 * sampler, penalty history and log-probabilities are omx_qwen3_batch_prefill's.  n_rows = 0 IS omx_qwen3_batch_prefill. */
int omx_qwen3_batch_prefill_embeds(omx_qwen3_batch b, int slot, const uint32_t* prompt, int n_prompt, const void* rows, omx_dtype rows_dtype,
                                   int first_row, int n_rows, uint32_t* first_token) {
    OMX_REQUIRE(b && prompt && first_token, "omx_qwen3_batch_prefill_embeds: null argument");
    OMX_REQUIRE(n_rows >= 0, "omx_qwen3_batch_prefill_embeds: n_rows %d is negative", n_rows);
    if (n_rows == 0) return batch_prefill_prompt(b, slot, prompt, n_prompt, first_token, nullptr);
    omx_qwen3 m = b->m;
    OMX_REQUIRE(rows != nullptr, "omx_qwen3_batch_prefill_embeds: null rows with n_rows %d", n_rows);
    OMX_REQUIRE(rows_dtype == OMX_FLOAT32 || rows_dtype == OMX_BFLOAT16 || rows_dtype == OMX_FLOAT16,
                "omx_qwen3_batch_prefill_embeds: rows of dtype %d (float32, bfloat16 or float16)", (int)rows_dtype);
    OMX_REQUIRE(first_row >= 0 && first_row <= n_prompt && n_rows <= n_prompt - first_row,
                "omx_qwen3_batch_prefill_embeds: rows [%d, %d + %d) lie outside the prompt of %d tokens", first_row, first_row, n_rows, n_prompt);
    OMX_REQUIRE(m->allreduce == nullptr && m->cfg.tp_size <= 1 && m->cfg.ep_size <= 1,
                "omx_qwen3_batch_prefill_embeds: tensor-parallel / expert-parallel engines are not supported (single-rank models only)");
    OMX_REQUIRE(m->cfg.num_experts == 0, "omx_qwen3_batch_prefill_embeds: sparse-MoE models are not supported (dense models only)");
    OMX_REQUIRE(n_prompt >= 2, "InvalidConfig: omx_qwen3_batch_prefill_embeds: a one-row prompt goes through the decode step, which cannot take "
                "embedding rows; pass at least 2 rows");
    const RowSpan span = {rows, rows_dtype, first_row, n_rows};
    return batch_prefill_prompt(b, slot, prompt, n_prompt, first_token, &span);
}

int omx_qwen3_batch_fork(omx_qwen3_batch b, int src, int dst, int resample, uint32_t* first_token) {
    OMX_REQUIRE(b && first_token, "omx_qwen3_batch_fork: null argument");
    OMX_REQUIRE(src >= 0 && src < b->n_slots, "omx_qwen3_batch_fork: source slot %d out of range (0..%d)", src, b->n_slots - 1);
    OMX_REQUIRE(dst >= 0 && dst < b->n_slots, "omx_qwen3_batch_fork: destination slot %d out of range (0..%d)", dst, b->n_slots - 1);
    OMX_REQUIRE(src != dst, "omx_qwen3_batch_fork: source and destination are the same slot %d", src);
    OMX_REQUIRE(b->prefilled[src] && b->pos[src] >= 1, "omx_qwen3_batch_fork: source slot %d has not been prefilled", src);
    OMX_REQUIRE(!b->prefilled[dst] && b->pos[dst] == 0, "omx_qwen3_batch_fork: destination slot %d is not empty (reset it first)", dst);
    omx_qwen3 m = b->m;
    OMX_REQUIRE(!m->filter_on, "omx_qwen3_batch_fork: filtered sampling (omx_qwen3_set_sampling) is on; call omx_qwen3_set_sampler first");
    // a resampled sibling starts the history a prefill of its own would have started: only right at the token after the prompt
    OMX_REQUIRE(!(resample && sampling_penalised(b->sampling[dst]) && b->decoded[src] > 0),
                "omx_qwen3_batch_fork: destination slot %d has a repetition / presence penalty on and source slot %d has decoded %d tokens past "
                "its prefill: the history of a resampled sibling would miss them (fork right after the prefill, or with resample = 0)",
                dst, src, b->decoded[src]);
    hipStream_t s = m->stream;
    const int pos = b->pos[src], D = m->cfg.head_dim, V = m->V;
    // rows [0, pos) of every KV head, layer by layer: the heads of a slab lie cap rows apart
    const size_t pitch = (size_t)b->cap * D * sizeof(bf16_t), width = (size_t)pos * D * sizeof(bf16_t);
    for (size_t l = 0; l < b->kbase.size(); ++l) {
        OMX_HIP_CHECK(hipMemcpy2DAsync(b->slot_k[dst][l], pitch, b->slot_k[src][l], pitch, width, (size_t)m->Hkv, hipMemcpyDeviceToDevice, s));
        OMX_HIP_CHECK(hipMemcpy2DAsync(b->slot_v[dst][l], pitch, b->slot_v[src][l], pitch, width, (size_t)m->Hkv, hipMemcpyDeviceToDevice, s));
    }
    // (a kv_bits = 8 batch: the packed rows and their scale | bias words)
    const size_t qpitch = (size_t)b->cap * D, qwidth = (size_t)pos * D, spitch = (size_t)b->cap * (D / 64) * 4, swidth = (size_t)pos * (D / 64) * 4;
    for (size_t l = 0; l < b->layer8.size(); ++l) {
        const Kv8Layer &from = b->slot8[src][l], &to = b->slot8[dst][l];
        OMX_HIP_CHECK(hipMemcpy2DAsync(to.kq, qpitch, from.kq, qpitch, qwidth, (size_t)m->Hkv, hipMemcpyDeviceToDevice, s));
        OMX_HIP_CHECK(hipMemcpy2DAsync(to.vq, qpitch, from.vq, qpitch, qwidth, (size_t)m->Hkv, hipMemcpyDeviceToDevice, s));
        OMX_HIP_CHECK(hipMemcpy2DAsync(to.ksb, spitch, from.ksb, spitch, swidth, (size_t)m->Hkv, hipMemcpyDeviceToDevice, s));
        OMX_HIP_CHECK(hipMemcpy2DAsync(to.vsb, spitch, from.vsb, spitch, swidth, (size_t)m->Hkv, hipMemcpyDeviceToDevice, s));
    }
    BatchSlot v = {};
    if (resample) {
        // src's kept row through dst's sampler: the sample launch keeps the row as dst's, draws with dst's next key and turns
        // pos - 1 into pos, as at the end of a prefill
        v.pos = pos - 1;
        OMX_HIP_CHECK(hipMemcpyAsync(b->slots + dst, &v, 8, hipMemcpyHostToDevice, s));
        OMX_HIP_CHECK(hipMemcpyAsync(b->row_slot, &dst, 4, hipMemcpyHostToDevice, s));
        if (clear_history(b, dst)) return 1;   // an EMPTY history: the launch marks the token it draws
        if (batch_sample(b, b->slot_logits + (size_t)src * V, &dst, 1, b->ring)) return 1;
        OMX_HIP_CHECK(hipMemcpyAsync(first_token, b->ring, 4, hipMemcpyDeviceToHost, s));
    } else {
        v.pos = pos;
        OMX_HIP_CHECK(hipMemcpyAsync(b->slots + dst, &v, 4, hipMemcpyHostToDevice, s));
        OMX_HIP_CHECK(hipMemcpyAsync(&b->slots[dst].pending, &b->slots[src].pending, 4, hipMemcpyDeviceToDevice, s));
        OMX_HIP_CHECK(hipMemcpyAsync(b->slot_logits + (size_t)dst * V, b->slot_logits + (size_t)src * V, (size_t)V * sizeof(bf16_t),
                                     hipMemcpyDeviceToDevice, s));
        OMX_HIP_CHECK(hipMemcpyAsync(first_token, &b->slots[src].pending, 4, hipMemcpyDeviceToHost, s));
        if (b->seen)   // the sibling continues src's sequence: src's history with it
            OMX_HIP_CHECK(hipMemcpyAsync(b->seen + (size_t)dst * V, b->seen + (size_t)src * V, (size_t)V, hipMemcpyDeviceToDevice, s));
        if (b->lp_top >= 0) {   // ... and the values of the token it shares with src
            const size_t top = (size_t)b->lp_top;
            OMX_HIP_CHECK(hipMemcpyAsync(b->slot_lp + dst, b->slot_lp + src, 4, hipMemcpyDeviceToDevice, s));
            if (top) OMX_HIP_CHECK(hipMemcpyAsync(b->slot_ids + dst * top, b->slot_ids + src * top, top * 4, hipMemcpyDeviceToDevice, s));
            if (top) OMX_HIP_CHECK(hipMemcpyAsync(b->slot_top + dst * top, b->slot_top + src * top, top * 4, hipMemcpyDeviceToDevice, s));
            b->lp_valid[dst] = b->lp_valid[src];
        }
    }
    // one level deep: a fork of a child shares what the child shares with the root, and holds the rest in its own copy alone
    const bool child = b->shared_len[src] > 0 && b->owner[src] != src;
    const int root = child ? b->owner[src] : src;
    const int sh = !b->share_on ? 0 : child ? b->shared_len[src] : pos / kChunk * kChunk;
    if (set_share(b, dst, root, sh)) return 1;
    if (!child && sh > b->shared_len[src] && set_share(b, src, src, sh)) return 1;
    OMX_HIP_CHECK(hipStreamSynchronize(s));
    b->pos[dst] = pos;
    b->prefilled[dst] = true;
    b->decoded[dst] = resample ? 0 : b->decoded[src];
    return 0;
}

int omx_qwen3_batch_shared(omx_qwen3_batch b, int slot, int* owner, int* shared_len) {
    OMX_BATCH_SLOT("omx_qwen3_batch_shared");
    OMX_REQUIRE(owner && shared_len, "omx_qwen3_batch_shared: null argument");
    BatchSlot v;   // the device's table, as omx_qwen3_batch_offset
    OMX_HIP_CHECK(hipMemcpyAsync(&v, b->slots + slot, sizeof(v), hipMemcpyDeviceToHost, b->m->stream));
    OMX_HIP_CHECK(hipStreamSynchronize(b->m->stream));
    *owner = v.owner;
    *shared_len = v.shared_len;
    return 0;
}

// n_steps steps of the listed slots; logprobs != null: also the rings' entries of those steps (omx_qwen3_batch_decode_logprobs, which has
// checked that they exist)
static int batch_decode_steps(omx_qwen3_batch b, const int* slots, int n_slots, int n_steps, uint32_t* tokens_out, float* logprobs,
                              uint32_t* top_ids, float* top_logprobs) {
    OMX_REQUIRE(n_slots >= 1 && n_slots <= b->n_slots, "omx_qwen3_batch_decode: %d slots listed (1..%d)", n_slots, b->n_slots);
    OMX_REQUIRE(n_steps >= 0 && n_steps <= kRingSteps, "omx_qwen3_batch_decode: n_steps=%d out of range (0..%d per call)", n_steps, kRingSteps);
    omx_qwen3 m = b->m;
    int rows[kMaxSlots];
    int longest = 0;
    for (int r = 0; r < n_slots; ++r) {
        const int slot = slots[r];
        OMX_REQUIRE(slot >= 0 && slot < b->n_slots, "omx_qwen3_batch_decode: slot %d out of range (0..%d)", slot, b->n_slots - 1);
        for (int q = 0; q < r; ++q) OMX_REQUIRE(slots[q] != slot, "omx_qwen3_batch_decode: slot %d listed twice", slot);
        OMX_REQUIRE(b->prefilled[slot], "omx_qwen3_batch_decode: slot %d has not been prefilled", slot);
        OMX_REQUIRE(b->pos[slot] + n_steps <= b->cap, "omx_qwen3_batch_decode: slot %d: %d cached + %d new tokens exceed max_context %d", slot,
                    b->pos[slot], n_steps, b->cap);
        rows[r] = slot;
        longest = std::max(longest, b->pos[slot] + n_steps);
    }
    OMX_REQUIRE(!m->filter_on, "omx_qwen3_batch_decode: filtered sampling (omx_qwen3_set_sampling) is on; call omx_qwen3_set_sampler first");
    if (n_steps == 0) return 0;
    if (resolve_weights(m)) return 1;
    hipStream_t s = m->stream;
    const bool packed = m->cfg.quant_bits != 0;
    if (prefill_reserve(m, n_slots, false)) return 1;
    OMX_HIP_CHECK(hipMemcpyAsync(b->row_slot, rows, (size_t)n_slots * 4, hipMemcpyHostToDevice, s));
    RaggedRows rag = batch_rows(b, longest);        // the longest listed sequence at the end of the call
    // the groups of the call: positions only grow inside it, so a row that may read a split from its owner now may do so at every step
    rag.group_min = b->group_min; rag.group_rows = b->group_rows;
    for (int r = 0; r < n_slots; ++r) {
        const int sh = std::min(b->shared_len[rows[r]], b->pos[rows[r]] / kChunk * kChunk);
        rag.grp_owner[r] = sh > 0 ? b->owner[rows[r]] : -1;
        rag.grp_shared[r] = sh;
        int same = 0;
        for (int q = 0; q <= r; ++q) same += sh > 0 && rag.grp_shared[q] > 0 && rag.grp_owner[q] == rag.grp_owner[r];
        rag.grouped = rag.grouped || (same >= b->group_min && !b->kv_bits);   // (8-bit slabs: every row reads its own, always)
    }
    OMX_HIP_CHECK(hipEventRecord(m->ev0, s));
    for (int i = 0; i < n_steps; ++i) {
        if (prefill_prefix_batched(m, n_slots, 0, nullptr, /*full_last=*/true, packed, nullptr, &rag)) return 1;
        if (batch_head_and_sample(b, m->pf_h, rows, n_slots, b->ring + (size_t)i * n_slots)) return 1;
    }
    OMX_HIP_CHECK(hipEventRecord(m->ev1, s));
    OMX_HIP_CHECK(hipMemcpyAsync(tokens_out, b->ring, (size_t)n_steps * n_slots * 4, hipMemcpyDeviceToHost, s));
    const size_t cells = (size_t)n_steps * n_slots, top = (size_t)std::max(b->lp_top, 0);
    if (logprobs) OMX_HIP_CHECK(hipMemcpyAsync(logprobs, b->lp_ring, cells * 4, hipMemcpyDeviceToHost, s));
    if (logprobs && top_ids && top) OMX_HIP_CHECK(hipMemcpyAsync(top_ids, b->top_id_ring, cells * top * 4, hipMemcpyDeviceToHost, s));
    if (logprobs && top_logprobs && top) OMX_HIP_CHECK(hipMemcpyAsync(top_logprobs, b->top_lp_ring, cells * top * 4, hipMemcpyDeviceToHost, s));
    OMX_HIP_CHECK(hipStreamSynchronize(s));
    OMX_HIP_CHECK(hipEventElapsedTime(&b->last_decode_ms, m->ev0, m->ev1));
    for (int r = 0; r < n_slots; ++r) {
        b->pos[rows[r]] += n_steps;
        b->decoded[rows[r]] += n_steps;
    }
    return 0;
}

int omx_qwen3_batch_decode(omx_qwen3_batch b, const int* slots, int n_slots, int n_steps, uint32_t* tokens_out) {
    OMX_REQUIRE(b && slots && tokens_out, "omx_qwen3_batch_decode: null argument");
    return batch_decode_steps(b, slots, n_slots, n_steps, tokens_out, nullptr, nullptr, nullptr);
}

int omx_qwen3_batch_decode_logprobs(omx_qwen3_batch b, const int* slots, int n_slots, int n_steps, uint32_t* tokens_out, float* logprobs,
                                    uint32_t* top_ids, float* top_logprobs) {
    OMX_REQUIRE(b && slots && tokens_out && logprobs, "omx_qwen3_batch_decode_logprobs: null argument");
    OMX_REQUIRE(b->lp_top >= 0, "omx_qwen3_batch_decode_logprobs: log-probabilities are off (omx_qwen3_batch_set_logprobs)");
    return batch_decode_steps(b, slots, n_slots, n_steps, tokens_out, logprobs, top_ids, top_logprobs);
}

int omx_qwen3_batch_set_logprobs(omx_qwen3_batch b, int top_n) {
    OMX_REQUIRE(b, "omx_qwen3_batch_set_logprobs: null batch");
    const int V = b->m->V;
    OMX_REQUIRE(top_n >= -1 && top_n <= OMX_LOGPROBS_MAX_TOP && top_n <= V,
                "omx_qwen3_batch_set_logprobs: top_n = %d is outside -1..min(%d, V = %d) (-1 = off, 0 = the drawn token only)", top_n,
                OMX_LOGPROBS_MAX_TOP, V);
    OMX_REQUIRE(top_n < 0 || (V % 8 == 0 && V <= (1 << 20)),
                "omx_qwen3_batch_set_logprobs: vocabulary %d must be a multiple of 8 and at most 2^20 (omx_logprob_rows' shapes)", V);
    if (top_n >= 0 && !b->lp_ring) {
        const size_t cells = (size_t)kRingSteps * kMaxSlots, mt = OMX_LOGPROBS_MAX_TOP;
        if (batch_alloc(b, &b->lp_ring, cells) || batch_alloc(b, &b->top_lp_ring, cells * mt) || batch_alloc(b, &b->top_id_ring, cells * mt) ||
            batch_alloc(b, &b->slot_lp, (size_t)b->n_slots) || batch_alloc(b, &b->slot_top, b->n_slots * mt) ||
            batch_alloc(b, &b->slot_ids, b->n_slots * mt) ||
            batch_alloc(b, &b->lp_scratch, logprob_top_scratch_bytes(kMaxSlots, V, OMX_LOGPROBS_MAX_TOP)))
            return 1;
        OMX_HIP_CHECK(hipStreamSynchronize(b->m->stream));
    }
    if (top_n != b->lp_top) {
        b->lp_top = top_n;
        for (int s = 0; s < kMaxSlots; ++s) b->lp_valid[s] = false;   // (the slots' rows are laid out by top_n)
    }
    return 0;
}

int omx_qwen3_batch_last_logprobs(omx_qwen3_batch b, int slot, float* logprob, uint32_t* top_ids, float* top_logprobs) {
    OMX_BATCH_SLOT("omx_qwen3_batch_last_logprobs");
    OMX_REQUIRE(logprob, "omx_qwen3_batch_last_logprobs: null argument");
    OMX_REQUIRE(b->lp_top >= 0, "omx_qwen3_batch_last_logprobs: log-probabilities are off (omx_qwen3_batch_set_logprobs)");
    OMX_REQUIRE(b->lp_valid[slot], "omx_qwen3_batch_last_logprobs: slot %d has sampled no token since omx_qwen3_batch_set_logprobs", slot);
    hipStream_t s = b->m->stream;
    const size_t top = (size_t)b->lp_top;
    OMX_HIP_CHECK(hipMemcpyAsync(logprob, b->slot_lp + slot, 4, hipMemcpyDeviceToHost, s));
    if (top_ids && top) OMX_HIP_CHECK(hipMemcpyAsync(top_ids, b->slot_ids + slot * top, top * 4, hipMemcpyDeviceToHost, s));
    if (top_logprobs && top) OMX_HIP_CHECK(hipMemcpyAsync(top_logprobs, b->slot_top + slot * top, top * 4, hipMemcpyDeviceToHost, s));
    OMX_HIP_CHECK(hipStreamSynchronize(s));
    return 0;
}

int omx_qwen3_batch_last_decode_ms(omx_qwen3_batch b, float* ms) {
    OMX_REQUIRE(b && ms, "omx_qwen3_batch_last_decode_ms: null argument");
    *ms = b->last_decode_ms;
    return 0;
}

int omx_qwen3_batch_logits(omx_qwen3_batch b, int slot, void* host_bf16, int n) {
    OMX_BATCH_SLOT("omx_qwen3_batch_logits");
    OMX_REQUIRE(host_bf16, "omx_qwen3_batch_logits: null argument");
    OMX_REQUIRE(n == b->m->V, "omx_qwen3_batch_logits: expected %d entries, got %d", b->m->V, n);
    OMX_HIP_CHECK(hipMemcpyAsync(host_bf16, b->slot_logits + (size_t)slot * b->m->V, (size_t)n * 2, hipMemcpyDeviceToHost, b->m->stream));
    OMX_HIP_CHECK(hipStreamSynchronize(b->m->stream));
    return 0;
}

int omx_qwen3_batch_offset(omx_qwen3_batch b, int slot, int* offset) {
    OMX_BATCH_SLOT("omx_qwen3_batch_offset");
    OMX_REQUIRE(offset, "omx_qwen3_batch_offset: null argument");
    BatchSlot v;   // the device's word, not the host's count of it
    OMX_HIP_CHECK(hipMemcpyAsync(&v, b->slots + slot, sizeof(v), hipMemcpyDeviceToHost, b->m->stream));
    OMX_HIP_CHECK(hipStreamSynchronize(b->m->stream));
    *offset = v.pos;
    return 0;
}

int omx_qwen3_batch_kv_bytes(omx_qwen3_batch b, size_t* bytes) {
    OMX_REQUIRE(b && bytes, "omx_qwen3_batch_kv_bytes: null argument");
    *bytes = b->kv_bytes;
    return 0;
}

int omx_qwen3_batch_kv_read(omx_qwen3_batch b, int slot, int layer, int first, int n, void* k_rows, void* v_rows, void* k_scales,
                            void* k_biases, void* v_scales, void* v_biases) {
    OMX_BATCH_SLOT("omx_qwen3_batch_kv_read");
    omx_qwen3 m = b->m;
    const int L = m->cfg.num_hidden_layers, D = m->cfg.head_dim, Hkv = m->Hkv, gpr = D / 64;
    OMX_REQUIRE(layer >= 0 && layer < L, "omx_qwen3_batch_kv_read: layer %d out of range (0..%d)", layer, L - 1);
    OMX_REQUIRE(k_rows && v_rows, "omx_qwen3_batch_kv_read: null argument");
    OMX_REQUIRE(first >= 0 && n >= 1 && first + n <= b->pos[slot], "omx_qwen3_batch_kv_read: rows [%d, %d) of the %d slot %d holds", first,
                first + n, b->pos[slot], slot);
    hipStream_t s = m->stream;
    if (!b->kv_bits) {
        OMX_REQUIRE(!k_scales && !k_biases && !v_scales && !v_biases, "omx_qwen3_batch_kv_read: scales / biases asked of a bf16 batch "
                    "(kv_bits 0 stores bf16 rows; pass null)");
        const size_t pitch = (size_t)b->cap * D * 2, width = (size_t)n * D * 2;
        OMX_HIP_CHECK(hipMemcpy2DAsync(k_rows, width, b->slot_k[slot][layer] + (size_t)first * D, pitch, width, (size_t)Hkv, hipMemcpyDeviceToHost, s));
        OMX_HIP_CHECK(hipMemcpy2DAsync(v_rows, width, b->slot_v[slot][layer] + (size_t)first * D, pitch, width, (size_t)Hkv, hipMemcpyDeviceToHost, s));
        OMX_HIP_CHECK(hipStreamSynchronize(s));
        return 0;
    }
    OMX_REQUIRE(k_scales && k_biases && v_scales && v_biases, "omx_qwen3_batch_kv_read: a kv_bits 8 batch returns scales and biases; null argument");
    // the codes of a row are MLX's words as they lie (element j = byte j, LSB first); the scale | bias words are split on the host
    const Kv8Layer& q = b->slot8[slot][layer];
    const size_t qpitch = (size_t)b->cap * D, qwidth = (size_t)n * D, spitch = (size_t)b->cap * gpr * 4, swidth = (size_t)n * gpr * 4;
    std::vector<uint32_t> ksb((size_t)Hkv * n * gpr), vsb((size_t)Hkv * n * gpr);
    OMX_HIP_CHECK(hipMemcpy2DAsync(k_rows, qwidth, q.kq + (size_t)first * D, qpitch, qwidth, (size_t)Hkv, hipMemcpyDeviceToHost, s));
    OMX_HIP_CHECK(hipMemcpy2DAsync(v_rows, qwidth, q.vq + (size_t)first * D, qpitch, qwidth, (size_t)Hkv, hipMemcpyDeviceToHost, s));
    OMX_HIP_CHECK(hipMemcpy2DAsync(ksb.data(), swidth, q.ksb + (size_t)first * gpr, spitch, swidth, (size_t)Hkv, hipMemcpyDeviceToHost, s));
    OMX_HIP_CHECK(hipMemcpy2DAsync(vsb.data(), swidth, q.vsb + (size_t)first * gpr, spitch, swidth, (size_t)Hkv, hipMemcpyDeviceToHost, s));
    OMX_HIP_CHECK(hipStreamSynchronize(s));
    for (size_t i = 0; i < ksb.size(); ++i) {
        ((uint16_t*)k_scales)[i] = (uint16_t)(ksb[i] & 0xFFFFu); ((uint16_t*)k_biases)[i] = (uint16_t)(ksb[i] >> 16);
        ((uint16_t*)v_scales)[i] = (uint16_t)(vsb[i] & 0xFFFFu); ((uint16_t*)v_biases)[i] = (uint16_t)(vsb[i] >> 16);
    }
    return 0;
}

int omx_qwen3_batch_debug_attention(omx_qwen3_batch b, int layer, const int* slots, int n, const void* q, void* out) {
    OMX_REQUIRE(b && slots && q && out, "omx_qwen3_batch_debug_attention: null argument");
    omx_qwen3 m = b->m;
    const int L = m->cfg.num_hidden_layers, D = m->cfg.head_dim, H = m->H;
    OMX_REQUIRE(layer >= 0 && layer < L, "omx_qwen3_batch_debug_attention: layer %d out of range (0..%d)", layer, L - 1);
    OMX_REQUIRE(n >= 1 && n <= kMaxSlots, "omx_qwen3_batch_debug_attention: %d rows (1..%d)", n, kMaxSlots);
    int longest = 0;
    BatchSlot table[kMaxSlots] = {};
    for (int r = 0; r < n; ++r) {
        const int slot = slots[r];
        OMX_REQUIRE(slot >= 0 && slot < b->n_slots, "omx_qwen3_batch_debug_attention: slot %d out of range (0..%d)", slot, b->n_slots - 1);
        OMX_REQUIRE(b->prefilled[slot] && b->pos[slot] >= 1, "omx_qwen3_batch_debug_attention: slot %d has not been prefilled", slot);
        table[slot].pos = b->pos[slot] - 1;   // the launch reads pos + 1 rows: the rows the slot holds, nothing appended
        longest = std::max(longest, b->pos[slot]);
    }
    hipStream_t s = m->stream;
    if (prefill_reserve(m, n, false)) return 1;
    OMX_HIP_CHECK(hipMemcpyAsync(b->dbg_slots, table, (size_t)b->n_slots * sizeof(BatchSlot), hipMemcpyHostToDevice, s));
    OMX_HIP_CHECK(hipMemcpyAsync(b->row_slot, slots, (size_t)n * 4, hipMemcpyHostToDevice, s));
    OMX_HIP_CHECK(hipMemcpyAsync(m->pf_qt, q, (size_t)n * H * D * sizeof(bf16_t), hipMemcpyHostToDevice, s));
    RaggedRows rag = batch_rows(b, longest);
    rag.slots = b->dbg_slots;                 // the batch's own table stays as it is
    if (launch_batch_attention(m, layer, rag, n, s)) return 1;
    OMX_HIP_CHECK(hipMemcpyAsync(out, m->pf_attn, (size_t)n * H * D * sizeof(bf16_t), hipMemcpyDeviceToHost, s));
    OMX_HIP_CHECK(hipStreamSynchronize(s));
    return 0;
}

int omx_qwen3_batch_trim(omx_qwen3_batch b, int slot, int n, uint32_t next_token) {
    OMX_BATCH_SLOT("omx_qwen3_batch_trim");
    OMX_REQUIRE(next_token < (uint32_t)b->m->cfg.vocab_size, "omx_qwen3_batch_trim: token id %u out of range (vocab %d)", next_token, b->m->cfg.vocab_size);
    OMX_REQUIRE(n >= 0 && n <= b->pos[slot], "omx_qwen3_batch_trim: cannot drop %d of %d cached tokens", n, b->pos[slot]);
    OMX_REQUIRE(!sampling_penalised(b->sampling[slot]), "omx_qwen3_batch_trim: slot %d has a repetition / presence penalty on: the token "
                "history on the device cannot be trimmed; call omx_qwen3_batch_set_sampler first", slot);
    BatchSlot v = {};
    v.pos = b->pos[slot] - n;
    v.pending = next_token;
    if (lower_share(b, slot, v.pos)) return 1;
    if (write_slot(b, slot, v, 8)) return 1;
    b->pos[slot] = v.pos;
    return 0;
}

int omx_qwen3_batch_reset(omx_qwen3_batch b, int slot) {
    OMX_BATCH_SLOT("omx_qwen3_batch_reset");
    const BatchSlot v = {};
    if (lower_share(b, slot, 0) || set_share(b, slot, slot, 0)) return 1;
    if (clear_history(b, slot)) return 1;
    if (write_slot(b, slot, v, 8)) return 1;   // (the sampler's key sequence goes on, as omx_qwen3_reset leaves the model's)
    b->pos[slot] = 0;
    b->prefilled[slot] = false;
    b->decoded[slot] = 0;
    b->lp_valid[slot] = false;
    return 0;
}

}  // extern "C"
