// The batched pass of the Qwen3 engine (engine.hip) over T rows at once: a prompt, the rows of a speculative verify, the text
// encoder's tapped layers -- matrix-core GEMMs (bf16 / float16 weights, packed ones dequantised per GEMM or kept in the dequant cache)
// or, for the verify pass of a packed model, the few-row packed GEMV.
#include "engine_model.hpp"

// (the kernels keep the scopes -- omx:: or global, both unnamed -- their names in traces and profiles have had so far)
namespace omx {
namespace {

// a float16 partial product widened for the f32 all-reduce of a tensor-parallel float16 prompt pass
__global__ void f16_widen_kernel(float* __restrict__ out, const bf16_t* __restrict__ in, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) out[i] = Act16<true>::val(in[i]);
}

}  // namespace
}  // namespace omx

namespace {

__global__ void copy_rows_strided_kernel(bf16_t* dst, int64_t dst_ld, const bf16_t* src, int64_t src_ld, int rows, int cols8) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < (int64_t)rows * cols8; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / cols8, c = i % cols8;
        *reinterpret_cast<u32x4*>(dst + r * dst_ld + c * 8) = *reinterpret_cast<const u32x4*>(src + r * src_ld + c * 8);
    }
}

// qwen3_encoder.rs:172-198: additive mask 0 where (j <= i and attention_mask[j]) else bf16(-1e9)
__global__ void encoder_mask_kernel(bf16_t* mask, const uint8_t* am, int T) {
    const bf16_t neg = f32_to_bf16(-1e9f);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < (int64_t)T * T; i += (int64_t)gridDim.x * blockDim.x) {
        const int q = (int)(i / T), k = (int)(i % T);
        mask[i] = (k <= q && am[k]) ? (bf16_t)0 : neg;
    }
}

// out [T, H * D] = in [H, T, D] (16-bit elements): the attention output of the explicit SDPA form, token-major for the O projection
__global__ void heads_to_tokens_kernel(bf16_t* __restrict__ out, const bf16_t* __restrict__ in, int H, int T, int D) {
    const int vpr = D / 8;
    const int64_t n = (int64_t)H * T * vpr;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int v = (int)(i % vpr), t = (int)((i / vpr) % T), h = (int)(i / ((int64_t)vpr * T));
        reinterpret_cast<u32x4*>(out)[((int64_t)t * H + h) * vpr + v] = reinterpret_cast<const u32x4*>(in)[i];
    }
}

// QuantizedEmbedding::forward for the T rows of prompt_dev straight from the packed table (the verify pass of a packed model, which
// dequantises no matrix): qembed_row (quant.hpp), so the rows equal the prompt pass's gather-then-dequantise bit for bit.  One block per row.
template <int BITS>
__global__ __launch_bounds__(256) void qembed_rows_kernel(bf16_t* __restrict__ out, const uint32_t* __restrict__ table, const bf16_t* __restrict__ scales,
                                                          const bf16_t* __restrict__ biases, const uint32_t* __restrict__ ids, int hidden, int group) {
    qembed_row<BITS>(out + (size_t)blockIdx.x * hidden, table, scales, biases, ids[blockIdx.x], hidden, group);
}

// the caller's rows of omx_qwen3_prefill_embeds over the gathered ones: n elements of src (DT) converted to the activation dtype
// (F16: float16, else bf16) with ONE round-to-nearest-even, as mlx's as_dtype does (qwen3-asr-mlx/src/model.rs:759); rows already in
// the activation dtype pass through their float32 value unchanged, bit for bit (NaN payloads aside)
template <int DT, bool F16>
__global__ void override_rows_kernel(bf16_t* __restrict__ dst, const typename Elem<DT>::T* __restrict__ src, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        dst[i] = Act16<F16>::bits(Elem<DT>::ld(src + i));
}

}  // namespace

namespace omx {

void launch_encoder_mask(bf16_t* mask, const uint8_t* am, int T, hipStream_t s) { encoder_mask_kernel<<<512, 256, 0, s>>>(mask, am, T); }

// the prompt pass's row buffers (T rows each) and, for a packed model, the scratch its dequantised GEMM operands pass through: grown
// here, on the host, AHEAD of a prompt's device-timed region (a hipMalloc between the launches leaves the device idle for its duration)
// dequant = false: the row buffers only (the verify pass of a packed model dequantises no weight: qgemv_rows.hip)
int prefill_reserve(omx_qwen3 m, int T, bool dequant) {
    const EngineConfig& c = m->cfg;
    const int hd = c.hidden_size, D = c.head_dim, H = m->H, Hkv = m->Hkv, I = m->I;
    if (T > m->pf_cap) {
        OMX_HIP_CHECK(hipStreamSynchronize(m->stream));
        bf16_t** bufs[] = {&m->pf_h, &m->pf_h2, &m->pf_xn, &m->pf_q, &m->pf_k, &m->pf_v, &m->pf_qt, &m->pf_attn, &m->pf_g, &m->pf_u};
        const size_t sizes[] = {(size_t)hd, (size_t)hd, (size_t)hd, (size_t)H * D, (size_t)Hkv * D, (size_t)Hkv * D,
                                (size_t)H * D, (size_t)H * D, (size_t)I, (size_t)I};
        for (int i = 0; i < 10; ++i) {
            if (*bufs[i]) OMX_HIP_CHECK(hipFree(*bufs[i]));
            OMX_HIP_CHECK(hipMalloc((void**)bufs[i], sizes[i] * (size_t)T * 2));
        }
        m->pf_cap = T;
    }
    if (c.quant_bits != 0 && dequant) {
        const size_t need = std::max((size_t)std::max(std::max(H * D, I), hd) * (size_t)std::max(hd, I),
                                     std::max((size_t)(H + 2 * Hkv) * D * hd, (size_t)2 * I * hd));
        if (need > m->dq_cap) {
            OMX_HIP_CHECK(hipStreamSynchronize(m->stream));
            if (m->dq_buf) OMX_HIP_CHECK(hipFree(m->dq_buf));
            OMX_HIP_CHECK(hipMalloc((void**)&m->dq_buf, need * 2));
            m->dq_cap = need;
        }
    }
    return 0;
}

// OMX_DEQUANT_CACHE=1 / 0: keep / do not keep the dequantised matrices between prompts; default: keep them for a dense model when
// they take at most a quarter of the free HBM and 64 GB (Qwen3-8B: 13.7 GB; a sparse-MoE model's attention matrices only on request).
// ONE allocation, made once per model -- host time (~0.03 s per GB) that omx_qwen3_prefill spends ahead of its device-timed region.
void dq_cache_prepare(omx_qwen3 m) {
    if (m->dq_cache_mode >= 0) return;
    const EngineConfig& c = m->cfg;
    const size_t hd = c.hidden_size, D = c.head_dim, H = m->H, Hkv = m->Hkv, I = m->I;
    const size_t per_layer = (H * D * hd * 2 + 2 * Hkv * D * hd + (c.num_experts == 0 ? 3 * I * hd : 0)) * 2;
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    const size_t need_b = per_layer * (size_t)c.num_hidden_layers;
    m->dq_cache_mode = env_on("OMX_DEQUANT_CACHE", c.num_experts == 0 && need_b <= free_b / 4 && need_b <= ((size_t)64 << 30));
    if (m->dq_cache_mode == 1 && !m->dq_slab) {
        m->dq_slab_bytes = need_b + (size_t)7 * c.num_hidden_layers * 256;      // (every matrix starts on a 256-byte boundary)
        if (hipMalloc((void**)&m->dq_slab, m->dq_slab_bytes) != hipSuccess) {
            (void)hipGetLastError();
            m->dq_slab = nullptr;
            m->dq_cache_mode = 0;
        }
    }
}

// the f32 rows a sharded prompt pass all-reduces ([T, hidden] partial of the MoE block, widened float16 partial products): at least T
// rows, grown to the row buffers' capacity
static int reserve_ep_partial(omx_qwen3 m, int T) {
    if (m->pf_ep_partial && m->pf_ep_cap >= T) return 0;
    OMX_HIP_CHECK(hipStreamSynchronize(m->stream));
    if (m->pf_ep_partial) OMX_HIP_CHECK(hipFree(m->pf_ep_partial));
    OMX_HIP_CHECK(hipMalloc((void**)&m->pf_ep_partial, (size_t)std::max(T, m->pf_cap) * m->cfg.hidden_size * sizeof(float)));
    m->pf_ep_cap = std::max(T, m->pf_cap);
    return 0;
}

// one packed Linear of the verify pass over T rows: launch_qgemv_rows in blocks of <= 8 rows (x, resid, out and the member outputs
// advance by the block's rows).  bits / g.group: the format of the members that carry none of their own; a stack whose members differ
// (each into its own mout) runs as one launch per run of equal-format members -- row t of every member stays bit-identical to
// launch_qgemv on row t alone, which is a function of the member's own format
int packed_rows(const QGemvArgs& g, int T, bf16_t* const* mout, int bits, int pro, int epi, hipStream_t s) {
    int fb[3] = {0, 0, 0}, fg[3] = {0, 0, 0}, first = -1;
    bool mixed = false;
    for (int i = 0; i < 3; ++i) {
        if (!g.m[i].w) continue;
        fb[i] = qmat_bits(g.m[i], bits); fg[i] = qmat_group(g.m[i], g.group);
        if (first < 0) first = i;
        else if (fb[i] != fb[first] || fg[i] != fg[first]) mixed = true;
    }
    if (mixed) {
        OMX_REQUIRE(epi == EPI_STORE && mout, "packed rows: members of different formats need a plain store into per-member outputs (gate and up must share a format)");
        for (int i = 0; i < 3;) {
            if (!g.m[i].w) { ++i; continue; }
            QGemvArgs r = g;
            r.m[0] = r.m[1] = r.m[2] = QMat{};
            r.N = 0; r.out = nullptr; r.group = fg[i];
            bf16_t* outs[3] = {nullptr, nullptr, nullptr};
            int j = i, k = 0;
            for (; j < 3 && g.m[j].w && fb[j] == fb[i] && fg[j] == fg[i]; ++j, ++k) { r.m[k] = g.m[j]; outs[k] = mout[j]; r.N += g.m[j].n; }
            if (packed_rows(r, T, outs, fb[i], pro, epi, s)) return 1;
            i = j;
        }
        return 0;
    }
    QGemvArgs u = g;
    if (first >= 0) { bits = fb[first]; u.group = fg[first]; }
    for (int t0 = 0; t0 < T; t0 += 8) {
        QRowsArgs ra = {};
        ra.g = u;
        ra.M = std::min(8, T - t0);
        ra.g.x = g.x + (size_t)t0 * g.K;
        if (g.resid) ra.g.resid = g.resid + (size_t)t0 * g.N;
        if (g.out) ra.g.out = g.out + (size_t)t0 * g.N;
        for (int i = 0; mout && i < 3; ++i)
            if (mout[i]) ra.mout[i] = mout[i] + (size_t)t0 * g.m[i].n;
        if (launch_qgemv_rows(ra, bits, pro, epi, s)) return 1;
    }
    return 0;
}

// The embedding rows of the T ids in prompt_dev into out [T, hidden], in the activation dtype -- the first launches of the batched pass
// and all of omx_qwen3_embed_tokens: a bf16 / float16 table gathered, a packed table straight through qembed_rows_kernel (rows_form:
// the verify pass of a packed model) or gathered and dequantised (pf_xn / pf_h2 as scratch: T <= pf_cap), bit-identical to each other
int embed_rows(omx_qwen3 m, bf16_t* out, int T, bool rows_form) {
    const int hd = m->cfg.hidden_size;
    const bool f16 = m->f16;
    hipStream_t s = m->stream;
    if (m->cfg.quant_bits != 0 && rows_form) {
        const int bits = m->q_embed.bits;      // the embedding's own format
#define OMX_QEMB_ROWS(B) \
        case B: OMX_LAUNCH(qembed_rows_kernel<B>, T, 256, 0, s, out, m->q_embed.w, m->q_embed.scales, m->q_embed.biases, m->prompt_dev, hd, m->q_embed.group); break;
        switch (bits) { OMX_QEMB_ROWS(2) OMX_QEMB_ROWS(3) OMX_QEMB_ROWS(4) OMX_QEMB_ROWS(5) OMX_QEMB_ROWS(6) OMX_QEMB_ROWS(8) }
#undef OMX_QEMB_ROWS
        OMX_LAUNCH_CHECK();
        return 0;
    }
    if (m->cfg.quant_bits != 0) {
        // QuantizedEmbedding::forward: gather the packed rows, dequantise (quantized.rs:192-203)
        const int wpr = hd * m->q_embed.bits / 32, gpr = hd / m->q_embed.group;
        uint32_t* rows_w = (uint32_t*)m->pf_xn;                       // scratch: [T, wpr] u32 fits in [T, hd] bf16
        bf16_t* rows_s = m->pf_h2;
        bf16_t* rows_b = m->pf_h2 + (size_t)T * gpr;
        if (omx_take_rows(rows_w, m->q_embed.w, m->prompt_dev, T, wpr, OMX_FLOAT32, s)) return 1;
        if (omx_take_rows(rows_s, m->q_embed.scales, m->prompt_dev, T, gpr, OMX_BFLOAT16, s)) return 1;
        if (omx_take_rows(rows_b, m->q_embed.biases, m->prompt_dev, T, gpr, OMX_BFLOAT16, s)) return 1;
        return launch_dequantize_bf16(out, (const uint32_t*)rows_w, rows_s, rows_b, T, hd, m->q_embed.group, m->q_embed.bits, f16, s, f16);
    }
    return omx_take_rows(out, m->embed, m->prompt_dev, T, hd, OMX_BFLOAT16, s);
}

static int launch_override_rows(bf16_t* dst, const void* src, omx_dtype dt, int64_t n, bool f16, hipStream_t s) {
    const int grid = (int)std::min<int64_t>((n + 255) / 256, 1024);
#define OMX_OVERRIDE(DT) \
    do { if (f16) OMX_LAUNCH((override_rows_kernel<DT, true>), grid, 256, 0, s, dst, (const Elem<DT>::T*)src, n); \
         else OMX_LAUNCH((override_rows_kernel<DT, false>), grid, 256, 0, s, dst, (const Elem<DT>::T*)src, n); } while (0)
    switch (dt) {
        case OMX_FLOAT32: OMX_OVERRIDE(OMX_FLOAT32); break;
        case OMX_BFLOAT16: OMX_OVERRIDE(OMX_BFLOAT16); break;
        case OMX_FLOAT16: OMX_OVERRIDE(OMX_FLOAT16); break;
        default: OMX_REQUIRE(false, "prompt pass: caller rows of dtype %d (float32, bfloat16 or float16)", (int)dt);
    }
#undef OMX_OVERRIDE
    OMX_LAUNCH_CHECK();
    return 0;
}

// Batched prefill of T prompt tokens (all but the last one, which goes through the decode step so
// that sampling stays in one place): fills the KV slabs of every layer.  Matrix-core path:
//   RMSNorm rows -> q/k/v GEMM -> [per-head norm + RoPE + cache scatter] -> flash attention
//   (causal, bottom-right aligned == the bool mask of utils.rs:134-153) -> o GEMM + residual ->
//   RMSNorm -> gate/up GEMM -> silu*up -> down GEMM + residual.        (model.rs:161-215,263-267,321-332)
// The last layer stops after its cache scatter: nothing downstream of it is consumed for these tokens.
// packed_rows_pass (omx_qwen3_verify only): every packed Linear of a dense single-rank bf16-triplet model through qgemv_rows.hip -- no weight
// is dequantised, neither into the dequant cache nor into its scratch
// kv: the slabs the rows are appended to and attend over (default: the model's own).
// rag (omx_qwen3_batch_decode only): the T rows are T different sequences -- embedding, cache append and attention take their ragged
// form (engine_batch.hip), every Linear is the launch the verify pass makes for T rows
// span (omx_qwen3_prefill_embeds only): rows of the caller's that replace the gathered embedding rows before the first layer
int prefill_prefix_batched(omx_qwen3 m, int T, int off, const EncodeOpts* enc, bool full_last, bool packed_rows_pass, const KvSlabs* kv,
                           const RaggedRows* rag, const RowSpan* span) {
    const EngineConfig& c = m->cfg;
    // float16 checkpoints (round 4): the same pass in float16 -- weights dequantised to float16, the eight-wave GEMM kernel's float16
    // form, float16 norms / RoPE / slabs, the flash attention kernel's float16 form -- for
    // plain prompts of a dense model, also on tensor-parallel shards (each rank's float16 partial products summed in f32); encode /
    // verify and the expert forms stay bfloat16-only
    // (a dense float16 checkpoint takes the same pass on its own float16 weights: nothing to dequantise)
    const bool f16 = m->f16;
    // (round 5: the encoder taps and passes of a handful of rows too -- a tap copies 16-bit rows whatever their format, and the 128-row
    //  float16 GEMM tile predicates its rows.  An encoder PADDING mask stays refused: the reference builds it as (1 - keep) * f16(-1e9) =
    //  0 * -inf = NaN on every kept key, flux-klein-mlx/src/qwen3_encoder.rs:196-198 -- there is no finite result to reproduce.)
    OMX_REQUIRE(!f16 || !(enc && enc->mask), "float16 encoder with an attention_mask: the reference's additive mask is 0 * f16(-1e9) = NaN in "
                "float16 (qwen3_encoder.rs:196-198); pass no mask (causal) or load the bfloat16 checkpoint");
    struct GemmF16Scope { bool on, was = false; explicit GemmF16Scope(bool o) : on(o) { if (on) was = gemm_set_f16(true); } ~GemmF16Scope() { if (on) gemm_set_f16(was); } } f16_scope(f16);
    const omx_dtype act_dt = f16 ? OMX_FLOAT16 : OMX_BFLOAT16;
    hipStream_t s = m->stream;
    const int hd = c.hidden_size, D = c.head_dim, H = m->H, Hkv = m->Hkv, I = m->I;
    const bool prow = packed_rows_pass && c.quant_bits != 0;
    OMX_REQUIRE(!prow || (!f16 && !enc && c.num_experts == 0 && m->allreduce == nullptr && c.tp_size <= 1 && c.ep_size <= 1),
                "packed verify pass: dense single-rank models with bf16 scales only");
    OMX_REQUIRE(!rag || (T <= 8 && full_last && !f16 && !enc && !kv && (prow || !c.quant_bits) && c.num_experts == 0 && m->allreduce == nullptr &&
                         c.tp_size <= 1 && c.ep_size <= 1),
                "ragged pass: up to 8 rows of a dense single-rank model with bf16 weights or bf16-scale packed weights");
    const int cap = kv ? kv->cap : m->cap;
    if (prefill_reserve(m, T, !prow)) return 1;   // (omx_qwen3_prefill has called it ahead of its timed region already)
    // tensor parallel: q/k/v/gate/up are this rank's column shards (local H, Hkv, I), o / down are row
    // shards whose [T, hidden] bf16 partial sums are all-reduced -- two collectives per layer -- before the residual add
    const bool tp = m->allreduce != nullptr && c.ep_size <= 1;
    auto row_split = [&](bf16_t* out, const bf16_t* x, const bf16_t* w, const bf16_t* resid, int K) -> int {
        if (!tp) return launch_gemm_bf16_ex(out, x, w, nullptr, resid, T, hd, K, s);
        bf16_t* part = m->pf_xn;   // free between the projections that read it and the next norm that rewrites it
        if (launch_gemm_bf16(part, x, w, nullptr, T, hd, K, s)) return 1;
        if (f16) {
            // float16: the ranks' float16 partial products widened, summed in f32 by the collective (every communicator reduces f32; none
            // float16) and folded into the float16 residual with the decode step's two roundings
            if (reserve_ep_partial(m, T)) return 1;
            f16_widen_kernel<<<1024, 256, 0, s>>>(m->pf_ep_partial, part, (int64_t)T * hd);
            OMX_LAUNCH_CHECK();
            if (allreduce_sum(m, m->pf_ep_partial, (size_t)T * hd)) return 1;
            return launch_ep_fold(1024, out, resid, m->pf_ep_partial, (int64_t)T * hd, true, s);
        }
        if (rank_allreduce(m, part, (size_t)T * hd, kNcclBfloat16, kNcclSum)) return 1;
        return omx_add(out, resid, part, (int64_t)T * hd, OMX_BFLOAT16, s);
    };
    const bool quant = c.quant_bits != 0;
    // quantized checkpoint: each weight is dequantised into one scratch matrix right before its GEMM (MLX's qmm does
    // the same per tile); K is the contraction width of that weight
    // `at`: element offset inside the scratch, so that the members of one segmented launch (q | k | v, gate | up) coexist
    if (quant && !prow) dq_cache_prepare(m);      // (omx_qwen3_prefill has called it ahead of its timed region already)
    auto W = [&](const bf16_t* dense, const QMat* qm, int K, size_t at = 0) -> const bf16_t* {
        if (!quant) return dense;
        if (m->dq_cache_mode == 1) {
            auto it = m->dq_cache.find(qm->w);
            if (it != m->dq_cache.end()) return it->second;
            const size_t bytes = ((size_t)qm->n * K * 2 + 255) & ~(size_t)255;
            if (m->dq_cache_bytes + bytes <= m->dq_slab_bytes) {
                bf16_t* keep = (bf16_t*)(m->dq_slab + m->dq_cache_bytes);
                if (launch_dequantize_bf16(keep, qm->w, qm->scales, qm->biases, qm->n, K, qm->group, qm->bits, f16, s, f16)) return nullptr;
                m->dq_cache[qm->w] = keep;
                m->dq_cache_bytes += bytes;
                return keep;
            }
            // (the slab is full -- matrices it was not sized for: those go through the scratch every time)
        }
        if (launch_dequantize_bf16(m->dq_buf + at, qm->w, qm->scales, qm->biases, qm->n, K, qm->group, qm->bits, f16, s, f16)) return nullptr;
        return m->dq_buf + at;
    };
    if (rag) {
        if (launch_batch_embed(m, *rag, T, s)) return 1;
    } else if (embed_rows(m, m->pf_h, T, prow)) {
        return 1;
    }
    if (span && span->n > 0) {
        // omx_qwen3_prefill_embeds: rows [first, first + n) replaced by the caller's, in one launch -- everything below reads pf_h
        OMX_REQUIRE(!rag && !enc && span->first >= 0 && span->first + span->n <= T, "prompt pass: caller rows [%d, %d) outside its %d rows",
                    span->first, span->first + span->n, T);
        if (launch_override_rows(m->pf_h + (size_t)span->first * hd, span->rows, span->dtype, (int64_t)span->n * hd, f16, s)) return 1;
    }
    bf16_t* h = m->pf_h;
    bf16_t* h2 = m->pf_h2;
    const float scale = 1.0f / sqrtf((float)D);
    const LayerQ no_q = {};
    const int n_run = enc ? enc->taps[enc->n_taps - 1] + 1 : c.num_hidden_layers;
    int next_tap = 0;
    // an encoder tap after layer l: the layer's output rows copied out as they are -- the raw hidden state, no final norm (:417-420)
    auto tap_out = [&](int l) -> int {
        if (!enc || next_tap >= enc->n_taps || enc->taps[next_tap] != l) return 0;
        copy_rows_strided_kernel<<<1024, 256, 0, s>>>(enc->out + (size_t)next_tap * hd, (int64_t)enc->n_taps * hd, h, hd, T, hd / 8);
        OMX_LAUNCH_CHECK();
        ++next_tap;
        return 0;
    };
    const bool seg_gemm = !env_off("OMX_PREFILL_SEGMENTED");   // 0: one launch per projection (A/B, tests)
    for (int l = 0; l < n_run; ++l) {
        const LayerW& L = m->layers[l];
        const LayerQ& Q = quant ? m->qlayers[l] : no_q;
        const bf16_t* w = nullptr;
        // q, k, v: one segmented launch over the three borrowed weights when the chip is filled that way (the separate k / v
        // grids are 128 tiles on 512 slots), else three launches
        GemmSegs qkv = {};
        qkv.n_plain = 3;
        qkv.plain[0] = {L.q, L.q_bias, m->pf_q, H * D, H * D, 0};
        qkv.plain[1] = {L.k, L.k_bias, m->pf_k, Hkv * D, Hkv * D, 0};
        qkv.plain[2] = {L.v, L.v_bias, m->pf_v, Hkv * D, Hkv * D, 0};
        // (a handful of rows: the weight-streaming launch normalises its staged copy of the rows itself -- no RMSNorm launch)
        const bool qkv_norm = !f16 && seg_gemm && gemm_segmented_preferred(T, hd, qkv) && gemv_rows_takes_norm(T, hd, qkv);
        if (prow) {   // q | k | v with the RMSNorm prologue, each member into its own row buffer
            QGemvArgs a = {};
            a.m[0] = Q.q; a.m[1] = Q.k; a.m[2] = Q.v;
            a.N = (H + 2 * Hkv) * D; a.K = hd; a.group = Q.q.group;
            a.x = h; a.norm_w = L.in_ln; a.eps = c.rms_norm_eps;
            bf16_t* const outs[3] = {m->pf_q, m->pf_k, m->pf_v};
            if (packed_rows(a, T, outs, Q.q.bits, PRO_RMSNORM, EPI_STORE, s)) return 1;
        } else
        if (!qkv_norm && omx_rms_norm(m->pf_xn, h, L.in_ln, T, hd, c.rms_norm_eps, act_dt, s)) return 1;
        if (qkv_norm) { qkv.pre_norm_w = L.in_ln; qkv.pre_norm_eps = c.rms_norm_eps; }
        if (prow) {
        } else if (f16 || (seg_gemm && gemm_segmented_preferred(T, hd, qkv))) {   // (float16: always the segmented 256-row kernel)
            if (quant) {   // the three dequantised matrices side by side in the scratch
                const size_t nq = (size_t)H * D * hd, nk = (size_t)Hkv * D * hd;
                if (!(qkv.plain[0].w = W(nullptr, &Q.q, hd, 0)) || !(qkv.plain[1].w = W(nullptr, &Q.k, hd, nq)) ||
                    !(qkv.plain[2].w = W(nullptr, &Q.v, hd, nq + nk)))
                    return 1;
            }
            if (launch_gemm_bf16_segmented(qkv_norm ? h : m->pf_xn, T, hd, qkv, s)) return 1;
        } else {
            if (!(w = W(L.q, &Q.q, hd)) || launch_gemm_bf16(m->pf_q, m->pf_xn, w, L.q_bias, T, H * D, hd, s)) return 1;
            if (!(w = W(L.k, &Q.k, hd)) || launch_gemm_bf16(m->pf_k, m->pf_xn, w, L.k_bias, T, Hkv * D, hd, s)) return 1;
            if (!(w = W(L.v, &Q.v, hd)) || launch_gemm_bf16(m->pf_v, m->pf_xn, w, L.v_bias, T, Hkv * D, hd, s)) return 1;
        }
        bf16_t* const kc = kv ? kv->k[l] : m->kcache[l];
        bf16_t* const vc = kv ? kv->v[l] : m->vcache[l];
        // (a slot of a kv_bits = 8 batch: what the slot holds of this layer into the staging pair the rows are appended to ...)
        if (kv && kv->packed && launch_kv8_rows(kv->packed[l], kc, vc, Hkv, D, cap, 0, off, /*pack=*/false, s)) return 1;
        if (rag) {
            if (launch_batch_scatter(m, l, *rag, T, s)) return 1;
        } else
        if (launch_qk_norm_rope_scatter(m->pf_q, m->pf_k, m->pf_v, L.q_norm, L.k_norm, m->rope_cos, m->rope_sin, m->pf_qt,
                                        kc, vc, T, H, Hkv, D, cap, off, c.rms_norm_eps, s, f16))
            return 1;
        // (... and the new rows packed into the slot's slabs, their staging copies replaced by what the codes dequantise to)
        if (kv && kv->packed && launch_kv8_rows(kv->packed[l], kc, vc, Hkv, D, cap, off, T, /*pack=*/true, s)) return 1;
        if (!enc && !full_last && l == c.num_hidden_layers - 1) break;   // a prefix only has to leave its K/V rows behind
        const bool skv_off = env_off("OMX_PREFILL_SPLITKV");
        if (f16) {
            // float16: the flash kernel's float16 instantiation (f32 scores / softmax / accumulators, P rounded to float16 for the second
            // product, one rounding of the output) -- MLX's fast SDPA accumulates in f32 the same way
            // (OMX_F16_ATTN=explicit: f32 on widened copies through omx_sdpa, then heads back next to each other per token: the A/B form)
            if (env_is("OMX_F16_ATTN", "explicit")) {
                if (omx_sdpa(m->pf_q, m->pf_qt, kc, vc, 1, H, Hkv, T, off + T, D, 0, (int64_t)cap * D, scale, OMX_MASK_CAUSAL,
                             nullptr, OMX_FLOAT16, s))
                    return 1;
                heads_to_tokens_kernel<<<1024, 256, 0, s>>>(m->pf_attn, m->pf_q, H, T, D);
                OMX_LAUNCH_CHECK();
            } else if (launch_attn_prefill(m->pf_attn, m->pf_qt, kc, vc, 1, H, Hkv, T, off + T, D, 0, (int64_t)cap * D, scale,
                                           OMX_MASK_CAUSAL, nullptr, s, /*out_token_major=*/true, nullptr, /*f16=*/true))
                return 1;
        } else
        if (rag) {   // row r over the first pos + 1 keys of its own slot's slabs
            if (launch_batch_attention(m, l, *rag, T, s)) return 1;
        } else
        if (!enc && T <= 8 && H / Hkv <= 8 && !skv_off) {
            // a handful of new rows over a long cache (speculative verify, a short follow-up prompt): the flash kernel gives them
            // H * ceil(T / 64) blocks that each walk all keys (53 us per layer for 5 rows at 2 k of context); the split-KV decode
            // kernel takes the T rows as batch entries over the ONE cache, row i seeing the first off + i + 1 keys
            AttnDecodeArgs a = {};
            a.q = m->pf_qt; a.q_bs = D; a.q_hs = (int64_t)T * D;                    // q_out[h][t][:] of the scatter kernel
            a.k = kc; a.v = vc;
            a.kv_batch_stride = 0; a.kv_head_stride = (int64_t)cap * D;
            a.B = T; a.H = H; a.Hkv = Hkv; a.Tk = off + T;
            a.scale = scale; a.mask_mode = OMX_MASK_NONE; a.causal_tail = 1;
            a.nsplit = decode_nsplit(off + T, T * Hkv);
            void* aws = nullptr;
            if (get_workspace_aux(&aws, attn_decode_ws_bytes(T * H, a.nsplit, D), s)) return 1;
            a.ws_o = (float*)aws;
            a.ws_ml = a.ws_o + (size_t)T * H * a.nsplit * D;
            a.out = m->pf_attn;                                                       // [T, H * D]
            if (launch_attn_decode(a, D, s)) return 1;
        } else if (launch_attn_prefill(m->pf_attn, m->pf_qt, kc, vc, 1, H, Hkv, T, off + T, D, 0,
                                (int64_t)cap * D, scale, enc && enc->mask ? OMX_MASK_ADDITIVE : OMX_MASK_CAUSAL,
                                enc ? enc->mask : nullptr, s, /*out_token_major=*/true))
            return 1;
        if (prow) {   // o + residual
            QGemvArgs a = {};
            a.m[0] = Q.o; a.N = hd; a.K = H * D; a.group = Q.o.group;
            a.x = m->pf_attn; a.resid = h; a.out = h2;
            if (packed_rows(a, T, nullptr, Q.o.bits, PRO_NONE, EPI_RESIDUAL, s)) return 1;
            // gate / up + nn::silu(gate) * up with the RMSNorm prologue, then down + residual
            a = QGemvArgs{};
            a.m[0] = Q.gate; a.m[1] = Q.up; a.N = I; a.K = hd; a.group = Q.gate.group;
            a.x = h2; a.norm_w = L.post_ln; a.eps = c.rms_norm_eps; a.out = m->pf_g;
            if (packed_rows(a, T, nullptr, Q.gate.bits, PRO_RMSNORM, EPI_SWIGLU, s)) return 1;
            a = QGemvArgs{};
            a.m[0] = Q.down; a.N = hd; a.K = I; a.group = Q.down.group;
            a.x = m->pf_g; a.resid = h2; a.out = h;
            if (packed_rows(a, T, nullptr, Q.down.bits, PRO_NONE, EPI_RESIDUAL, s)) return 1;
            continue;
        }
        if (!(w = W(L.o, &Q.o, H * D)) || row_split(h2, m->pf_attn, w, h, H * D)) return 1;
        GemmSegs gu = {};
        gu.w_gate = L.gate; gu.w_up = L.up; gu.out_act = m->pf_g; gu.half = I; gu.ld_act = I; gu.act_mode = 1;
        const bool gu_norm = !f16 && !layer_is_moe(c, l) && seg_gemm && gemm_segmented_preferred(T, hd, gu) && gemv_rows_takes_norm(T, hd, gu);
        const bool ds_moe = layer_is_moe(c, l) && c.moe_mode == 2;      // (its router launch normalises the rows itself)
        if (!gu_norm && !ds_moe && omx_rms_norm(m->pf_xn, h2, L.post_ln, T, hd, c.rms_norm_eps, act_dt, s)) return 1;
        if (gu_norm) { gu.pre_norm_w = L.post_ln; gu.pre_norm_eps = c.rms_norm_eps; }
        if (ds_moe) {   // DeepSeek-V2 family: float32 router, routed + shared experts, the residual in the combine
            if (omx_moe_deepseek_block_forward(h, h2, h2, L.post_ln, c.rms_norm_eps, m->pf_xn, L.moe_gate, L.moe_wg, L.moe_wu, L.moe_wd, L.moe_tail,
                                               L.sh_gate, L.sh_up, L.sh_down, T, hd, c.moe_intermediate_size, c.num_experts, c.num_experts_per_tok,
                                               c.n_shared_experts, c.norm_topk_prob, c.routed_scaling_factor, s))
                return 1;
            if (tap_out(l)) return 1;
            continue;
        }
        if (layer_is_moe(c, l)) {   // sparse-MoE feed-forward over all T rows (grouped MFMA GEMM route), then the residual
            if (quant && (c.ep_size > 1 || c.tp_size > 1)) {
                // packed stacks under expert parallelism / expert tensor parallelism (round 5): this rank's stacks dequantised per call, the
                // bf16 batched form, ONE all-reduce of the [T, hidden] f32 partial (the exchange combine stays a bf16-checkpoint path)
                const bool etp = c.tp_size > 1;
                const int el = etp ? c.num_experts : c.num_experts / c.ep_size;
                if (reserve_ep_partial(m, T)) return 1;
                if (omx_moe_block_partial_ep_q(m->pf_ep_partial, h2, L.post_ln, c.rms_norm_eps, m->pf_xn, OMX_QMOE_ARGS(Q), T, hd, etp ? m->moe_I : c.moe_intermediate_size,
                                               c.num_experts, c.num_experts_per_tok, c.moe_mode, c.norm_topk_prob, etp ? 0 : c.ep_rank * el, el,
                                               c.quant_group, c.quant_bits, f16 ? 1 : 0, s))
                    return 1;
                if (allreduce_sum(m, m->pf_ep_partial, (size_t)T * hd)) return 1;
                if (launch_ep_fold(1024, h, h2, m->pf_ep_partial, (int64_t)T * hd, f16, s)) return 1;
            } else if (quant) {
                if (omx_moe_block_forward_q_ex(h, h2, h2, L.post_ln, c.rms_norm_eps, m->pf_xn, OMX_QMOE_ARGS(Q), T, hd, c.moe_intermediate_size,
                                               c.num_experts, c.num_experts_per_tok, c.moe_mode, c.norm_topk_prob, c.quant_group,
                                               c.quant_bits, f16 ? 1 : 0, s))
                    return 1;
            } else if (c.ep_size > 1 || c.tp_size > 1) {
                // expert TENSOR parallel: the same launches over ALL experts at this rank's 1 / tp of their intermediate columns -- the f32
                // partial of every token's weighted sum is all-reduced like the expert-parallel one (each rank's partial products rounded
                // to bf16 before the sum: the dense model's row-split rounding, not the decode step's single-device one).
                // expert parallel: attention is replicated, so every rank already holds all T rows -- there is
                // nothing to dispatch.  Each rank routes all rows, multiplies the slots of ITS experts (grouped matrix-core GEMMs over
                // a device-side plan), and ONE all-reduce per layer sums the [T, hidden] f32 partials: the combine half of an
                // all-to-all exchange, with the reduction done by the collective.  (Until round 3 a prompt under EP was T decode steps.)
                const bool etp = c.tp_size > 1;
                const int el = etp ? c.num_experts : c.num_experts / c.ep_size;
                // expert parallel on the peer communicator's exchange path (round 4): the weighted sum as an all-to-all combine of the
                // routed slots' rows to their tokens' owners + an all-gather of the finished residual rows, in ONE kernel
                // (peer_allreduce.hip peer_moe_combine_kernel) -- a rank pushes ~T k / N + T (N - 1) / N rows of bf16 instead of
                // taking part in an all-reduce of [T, hidden] f32.  Same roundings (bit-identical for top-2).  OMX_EP_COMBINE=allreduce
                // keeps the all-reduce; any communicator without the exchange path does too.
                const bool cmb_allreduce = env_is("OMX_EP_COMBINE", "allreduce");
                if (!etp && m->allreduce == (nccl_allreduce_fn)omx_peer_allreduce_fn() && omx_peer_comm_stage_bytes(m->comm) > 0 &&
                    T * c.num_experts_per_tok > 32 &&      // (a handful of rows takes the block's GEMV form, which has no slot tables)
                    !cmb_allreduce) {
                    omx_moe_ep_slots sl = {};
                    if (omx_moe_block_slots_ep(&sl, m->pf_xn, L.moe_gate, L.moe_wg, L.moe_wu, L.moe_wd, T, hd, c.moe_intermediate_size, c.num_experts,
                                               c.num_experts_per_tok, c.moe_mode, c.norm_topk_prob, c.ep_rank * el, el, s))
                        return 1;
                    const int rc = omx_peer_moe_combine(h, h2, &sl, T, hd, c.num_experts_per_tok, c.ep_rank * el, el, m->comm, s);
                    OMX_REQUIRE(rc == 0 || rc == 2, "expert-parallel combine over the peer communicator failed");
                    if (rc == 0) {
                        if (tap_out(l)) return 1;
                        continue;
                    }
                    // (rc 2: this size does not fit the stages -- the slots were computed, the all-reduce form below recomputes them)
                }
                if (reserve_ep_partial(m, T)) return 1;
                if (omx_moe_block_partial_ep(m->pf_ep_partial, m->pf_xn, nullptr, c.rms_norm_eps, nullptr, L.moe_gate, L.moe_wg, L.moe_wu, L.moe_wd,
                                             T, hd, etp ? m->moe_I : c.moe_intermediate_size, c.num_experts, c.num_experts_per_tok, c.moe_mode,
                                             c.norm_topk_prob, etp ? 0 : c.ep_rank * el, el, s))
                    return 1;
                if (allreduce_sum(m, m->pf_ep_partial, (size_t)T * hd)) return 1;
                if (launch_ep_fold(1024, h, h2, m->pf_ep_partial, (int64_t)T * hd, false, s)) return 1;
            } else {
                if (omx_moe_forward(m->pf_attn, m->pf_xn, L.moe_gate, L.moe_wg, L.moe_wu, L.moe_wd, T, hd, c.moe_intermediate_size,
                                    c.num_experts, c.num_experts_per_tok, c.moe_mode, c.norm_topk_prob, nullptr, nullptr, s))
                    return 1;
                if (omx_add(h, h2, m->pf_attn, (int64_t)T * hd, OMX_BFLOAT16, s)) return 1;
            }
            if (tap_out(l)) return 1;
            continue;
        }
        // gate, up and nn::silu(gate) * up: one launch with the activation in the epilogue (768 tiles = 3 full rounds at
        // T = 2048 instead of 2 x 384), else two GEMMs + the elementwise kernel
        if (f16 || (seg_gemm && gemm_segmented_preferred(T, hd, gu))) {
            if (quant && (!(gu.w_gate = W(nullptr, &Q.gate, hd, 0)) || !(gu.w_up = W(nullptr, &Q.up, hd, (size_t)I * hd)))) return 1;
            if (launch_gemm_bf16_segmented(gu_norm ? h2 : m->pf_xn, T, hd, gu, s)) return 1;
        } else {
            if (!(w = W(L.gate, &Q.gate, hd)) || launch_gemm_bf16(m->pf_g, m->pf_xn, w, nullptr, T, I, hd, s)) return 1;
            if (!(w = W(L.up, &Q.up, hd)) || launch_gemm_bf16(m->pf_u, m->pf_xn, w, nullptr, T, I, hd, s)) return 1;
            if (launch_silu_mul(m->pf_g, m->pf_g, m->pf_u, (int64_t)T * I, s)) return 1;
        }
        if (!(w = W(L.down, &Q.down, I)) || row_split(h, m->pf_g, w, h2, I)) return 1;
        if (tap_out(l)) return 1;
    }
    return 0;
}

}  // namespace omx
