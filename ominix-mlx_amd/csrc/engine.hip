// Fused Qwen3 decode engine (see include/omx.h "Fused decode engine").
//
// Host-side mirror, in C++, of the caller of the hot path: qwen3-mlx's Model/Generate
// (qwen3-mlx/src/model.rs:387-433, 473-498, 743-844) driving mlx-rs-core's KVCache
// (mlx-rs-core/src/cache.rs:91-194).  The reference records ~1000 lazy graph nodes per token and
// lets MLX schedule them; here one decode step is 6 launches per layer captured once in a
// hipGraph and replayed per token, with the step state (position, current token, token ring)
// kept in device memory so that replay needs no host patching.
//
// HBM layout (288 GB part: everything resident, nothing paged):
//   weights      borrowed pointers, bf16 [out,in] row-major (checkpoint layout, nn/linear.rs)
//   KV cache     per layer K and V slabs [Hkv_local, cap, D] bf16, cap = max_context rounded up
//                to the 256-token step of cache.rs:110-117 (same API-visible growth semantics,
//                no reallocation + concatenate on growth)
//   rope tables  cos/sin [cap, D/2] f32, built once in fp64
//   step state   pos, cur_token, out ring, argmax partials
#include "engine_model.hpp"

namespace omx {
namespace {

__global__ void rope_table_kernel(float* cos_t, float* sin_t, int cap, int half, double neg_log_base_over_half,
                                  double scale) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= cap * half) return;
    const int t = idx / half, i = idx % half;
    const double ang = ((double)t * scale) * exp((double)i * neg_log_base_over_half);
    double s, c;
    sincos(ang, &s, &c);
    cos_t[idx] = (float)c;
    sin_t[idx] = (float)s;
}

// step state updates (single thread; a few dozen ns of work, they only order the graph); StepState: step_state.hpp

}  // namespace
}  // namespace omx

extern "C" {

int omx_qwen3_create(omx_qwen3* out, const omx_qwen3_config* cfg) { return omx_qwen3_create_deepseek(out, cfg, nullptr); }

int omx_qwen3_create_deepseek(omx_qwen3* out, const omx_qwen3_config* cfg, const omx_qwen3_deepseek_plan* plan) {
    OMX_REQUIRE(out && cfg, "omx_qwen3_create: null argument");
    EngineConfig with_plan;
    static_cast<omx_qwen3_config&>(with_plan) = *cfg;
    if (plan) {
        with_plan.first_k_dense_replace = plan->first_k_dense_replace;
        with_plan.n_shared_experts = plan->n_shared_experts;
        with_plan.routed_scaling_factor = plan->routed_scaling_factor;
    } else if (cfg->num_experts > 0 && cfg->moe_mode == 2) {
        with_plan.routed_scaling_factor = 1.f;
    }
    const EngineConfig& c = with_plan;
    OMX_REQUIRE(c.tp_size >= 1 && c.tp_rank >= 0 && c.tp_rank < c.tp_size, "InvalidConfig: tp rank %d of %d", c.tp_rank, c.tp_size);
    OMX_REQUIRE(c.hidden_size > 0 && c.hidden_size % 64 == 0, "InvalidConfig: hidden_size %d must be a multiple of 64", c.hidden_size);
    OMX_REQUIRE(c.head_dim == 64 || c.head_dim == 128, "InvalidConfig: head_dim %d (64 or 128 supported)", c.head_dim);
    OMX_REQUIRE(c.num_attention_heads % c.num_key_value_heads == 0, "InvalidConfig: heads %d not a multiple of kv heads %d", c.num_attention_heads, c.num_key_value_heads);
    OMX_REQUIRE(c.num_attention_heads % c.tp_size == 0 && c.intermediate_size % c.tp_size == 0 && c.vocab_size % c.tp_size == 0,
                "InvalidConfig: heads %d / intermediate %d / vocab %d must divide by tp_size %d", c.num_attention_heads, c.intermediate_size, c.vocab_size, c.tp_size);
    // KV heads: split over the ranks, or -- with fewer KV heads than ranks -- replicated: tp_size / Hkv ranks share one head
    // (SURVEY.md 8e), which needs that many ranks to divide a query group
    OMX_REQUIRE(c.num_key_value_heads >= c.tp_size ? c.num_key_value_heads % c.tp_size == 0
                    : (c.tp_size % c.num_key_value_heads == 0 &&
                       (c.num_attention_heads / c.num_key_value_heads) % (c.tp_size / c.num_key_value_heads) == 0),
                "InvalidConfig: %d kv heads cannot be split or replicated over tp_size %d", c.num_key_value_heads, c.tp_size);
    OMX_REQUIRE(c.quant_bits == 0 || c.quant_bits == 2 || c.quant_bits == 3 || c.quant_bits == 4 || c.quant_bits == 5 || c.quant_bits == 6 ||
                    c.quant_bits == 8, "InvalidConfig: quantization bits %d (0 = bf16, 2, 3, 4, 5, 6, 8)", c.quant_bits);
    // the widths whose packed kernels exist for the dense single-rank model only (no packed expert stacks, no sharded rows / K slices)
    OMX_REQUIRE(!quant_chunked(c.quant_bits) || (c.num_experts == 0 && c.tp_size <= 1 && c.ep_size <= 1),
                "InvalidConfig: %d-bit quantization runs on dense single-rank models (num_experts %d, tp_size %d, ep_size %d; experts and "
                "tensor / expert parallelism take bits 4 or 8)", c.quant_bits, c.num_experts, c.tp_size, c.ep_size);
    // (round 4) quantized checkpoints under tensor parallelism: the packed rows / K slices of the dense model; (round 5) also the packed
    // expert stacks of a sparse-MoE model, expert parallel or expert tensor parallel, with bf16 triplets
    omx_qwen3 m = new omx_qwen3_();
    m->cfg = c;
    if (m->cfg.rope_scale == 0.f) m->cfg.rope_scale = 1.f;
    if (m->cfg.ep_size < 1) m->cfg.ep_size = 1;
    if (m->cfg.quant_bits && m->cfg.quant_group == 0) m->cfg.quant_group = 64;     // nn/quantized.rs:330-333
    OMX_REQUIRE(!m->cfg.quant_bits || m->cfg.quant_group == 32 || m->cfg.quant_group == 64 || m->cfg.quant_group == 128,
                "InvalidConfig: quantization group_size %d (32, 64, 128)", m->cfg.quant_group);
    // (round 5: float16 sparse-MoE checkpoints also expert parallel / expert tensor parallel -- decode form; their prompts go token by token)
    OMX_REQUIRE(!m->cfg.quant_scales_f16 || (m->cfg.quant_bits && m->cfg.head_dim == 128),
                "InvalidConfig: a float16 checkpoint (quantization scales_dtype float16) runs as a packed model with head_dim 128");
    // dense float16 weights: single rank, dense MLP, no q/k/v bias, head_dim 128 (the float16 attention kernels' width)
    OMX_REQUIRE(!c.float16_weights || !c.quant_bits,
                "InvalidConfig: float16_weights marks a dense checkpoint (quant_bits 0, got %d); a packed float16 checkpoint sets quant_scales_f16", c.quant_bits);
    OMX_REQUIRE(!c.float16_weights || c.num_experts == 0, "InvalidConfig: float16_weights with experts (dense float16 MoE is not supported)");
    OMX_REQUIRE(!c.float16_weights || (c.tp_size <= 1 && m->cfg.ep_size <= 1),
                "InvalidConfig: float16_weights under tensor / expert parallelism (tp_size %d, ep_size %d) is not supported", c.tp_size, m->cfg.ep_size);
    OMX_REQUIRE(!c.float16_weights || !c.attention_bias, "InvalidConfig: float16_weights with attention_bias (dense float16 Qwen2) is not supported");
    OMX_REQUIRE(!c.float16_weights || c.head_dim == 128, "InvalidConfig: float16_weights needs head_dim 128 (got %d)", c.head_dim);
    m->f16 = c.quant_scales_f16 || c.float16_weights;
    // DeepSeek-V2 family (moe_mode 2): a dense prefix, shared experts, a scaled float32 router -- bf16 on one rank
    const bool ds = c.num_experts > 0 && c.moe_mode == 2;
    OMX_REQUIRE(ds || (c.first_k_dense_replace == 0 && c.n_shared_experts == 0 && (c.routed_scaling_factor == 0.f || c.routed_scaling_factor == 1.f)),
                "InvalidConfig: first_k_dense_replace %d, n_shared_experts %d and routed_scaling_factor %g belong to moe_mode 2 (deepseek) with experts",
                c.first_k_dense_replace, c.n_shared_experts, (double)c.routed_scaling_factor);
    OMX_REQUIRE(!ds || !c.quant_bits, "InvalidConfig: moe_mode 2 (deepseek) with quant_bits %d is not supported (bf16 checkpoints)", c.quant_bits);
    OMX_REQUIRE(!ds || !c.float16_weights, "InvalidConfig: moe_mode 2 (deepseek) with float16_weights is not supported");
    OMX_REQUIRE(!ds || !c.attention_bias, "InvalidConfig: moe_mode 2 (deepseek) with attention_bias is not supported");
    OMX_REQUIRE(!ds || c.tp_size <= 1, "InvalidConfig: moe_mode 2 (deepseek) with tp_size %d is not supported (single rank)", c.tp_size);
    OMX_REQUIRE(!ds || m->cfg.ep_size <= 1, "InvalidConfig: moe_mode 2 (deepseek) with ep_size %d is not supported (single rank)", m->cfg.ep_size);
    OMX_REQUIRE(!ds || (c.first_k_dense_replace >= 0 && c.first_k_dense_replace <= c.num_hidden_layers && c.n_shared_experts >= 0 &&
                        c.n_shared_experts <= 8 && c.routed_scaling_factor > 0.f),
                "InvalidConfig: moe_mode 2 (deepseek): first_k_dense_replace %d of %d layers, n_shared_experts %d (0..8), routed_scaling_factor %g (> 0)",
                c.first_k_dense_replace, c.num_hidden_layers, c.n_shared_experts, (double)c.routed_scaling_factor);
    m->H = c.num_attention_heads / c.tp_size;
    m->Hkv = c.num_key_value_heads >= c.tp_size ? c.num_key_value_heads / c.tp_size : 1;
    m->I = c.intermediate_size / c.tp_size;
    m->V = c.vocab_size / c.tp_size;
    OMX_REQUIRE(!any_dense_layer(c) || m->I % 64 == 0, "InvalidConfig: per-rank intermediate %d must be a multiple of 64", m->I);
    OMX_REQUIRE(!c.quant_bits || (c.hidden_size % 512 == 0 && (m->H * c.head_dim) % 512 == 0 && (c.num_experts > 0 || m->I % 512 == 0)),
                "InvalidConfig: quantized checkpoints need hidden %d, attention width %d and intermediate %d to be multiples of 512", c.hidden_size, m->H * c.head_dim, m->I);
    OMX_REQUIRE(!c.attention_bias || !c.quant_bits, "InvalidConfig: attention_bias (Qwen2) runs on bf16 checkpoints");
    const int step = 256;   // cache.rs:110-117
    m->cap = ((c.max_context > 0 ? c.max_context : 4096) + step - 1) / step * step;
    OMX_HIP_CHECK(hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking));
    OMX_HIP_CHECK(hipEventCreate(&m->ev0));
    OMX_HIP_CHECK(hipEventCreate(&m->ev1));
    const int D = c.head_dim, L = c.num_hidden_layers;
    m->kcache.resize(L);
    m->vcache.resize(L);
    for (int l = 0; l < L; ++l) {
        if (dev_alloc(m, &m->kcache[l], (size_t)m->Hkv * m->cap * D)) return 1;
        if (dev_alloc(m, &m->vcache[l], (size_t)m->Hkv * m->cap * D)) return 1;
    }
    if (dev_alloc(m, &m->rope_cos, (size_t)m->cap * D / 2) || dev_alloc(m, &m->rope_sin, (size_t)m->cap * D / 2)) return 1;
    {
        const int n = m->cap * D / 2;
        rope_table_kernel<<<(n + 255) / 256, 256, 0, m->stream>>>(m->rope_cos, m->rope_sin, m->cap, D / 2,
                                                                  -log((double)m->cfg.rope_theta) / (double)(D / 2),
                                                                  (double)m->cfg.rope_scale);
        OMX_LAUNCH_CHECK();
    }
    if (c.num_experts > 0) {
        // tp_size > 1: expert TENSOR parallel -- attention sharded like the dense model, every expert's intermediate columns split over
        // the ranks (decode streams 1 / tp of the two routed experts on every rank; prompts: the expert-parallel batched form over all experts)
        // (packed stacks, round 5: a rank's columns are whole quantisation groups AND whole packed-GEMV steps: multiples of 512)
        OMX_REQUIRE(c.tp_size == 1 || (c.ep_size <= 1 && c.moe_intermediate_size % ((c.quant_bits ? 512 : 64) * c.tp_size) == 0),
                    "InvalidConfig: expert tensor parallelism (tp_size %d with experts) needs ep_size 1 and moe_intermediate_size %d divisible by %d * tp_size",
                    c.tp_size, c.moe_intermediate_size, c.quant_bits ? 512 : 64);
        m->moe_I = c.moe_intermediate_size / c.tp_size;
        OMX_REQUIRE(c.ep_size <= 1 || (c.ep_rank >= 0 && c.ep_rank < c.ep_size && c.num_experts % c.ep_size == 0),
                    "InvalidConfig: expert parallel rank %d of %d over %d experts", c.ep_rank, c.ep_size, c.num_experts);
        OMX_REQUIRE(!c.quant_bits || c.moe_intermediate_size % 512 == 0, "InvalidConfig: quantised experts need moe_intermediate_size %% 512 == 0 (%d)", c.moe_intermediate_size);
        OMX_REQUIRE(c.num_experts_per_tok >= 1 && c.num_experts_per_tok <= c.num_experts && c.moe_intermediate_size > 0 &&
                        c.moe_intermediate_size % 64 == 0 && (c.moe_mode == 0 || c.moe_mode == 1 || c.moe_mode == 2) && (c.tp_size > 1 || m->H * D >= c.hidden_size),
                    "InvalidConfig: experts %d top-%d moe_intermediate_size %d mode %d", c.num_experts, c.num_experts_per_tok,
                    c.moe_intermediate_size, c.moe_mode);
        // the MoE block takes its scratch from the library workspace: size it ONCE for the largest batch (a whole-context
        // prefill) so that the pointers captured in the step graph never move
        size_t need = 0;
        omx_moe_workspace_bytes(m->cap, c.hidden_size, c.moe_intermediate_size, c.num_experts, c.num_experts_per_tok, &need);
        if (ds) omx_moe_deepseek_workspace_bytes(m->cap, c.hidden_size, c.moe_intermediate_size, c.num_experts, c.num_experts_per_tok, c.n_shared_experts, &need);
        void* ws = nullptr;
        if (get_workspace(&ws, need)) return 1;
        if (c.ep_size > 1 && get_workspace_aux(&ws, need, m->stream)) return 1;   // the expert-parallel block's per-stream scratch (moe.hip)
        if (c.tp_size > 1) {   // expert tensor parallel: the batched pass's plan + slot buffers at this rank's column count
            omx_moe_workspace_bytes(m->cap, c.hidden_size, m->moe_I, c.num_experts, c.num_experts_per_tok, &need);
            if (get_workspace_aux(&ws, need, m->stream)) return 1;
        }
        if (dev_alloc(m, &m->moe_xn, (size_t)c.hidden_size) || dev_alloc(m, &m->moe_out, (size_t)c.hidden_size)) return 1;
        if (c.tp_size > 1 && (dev_alloc(m, &m->moe_y, (size_t)c.num_experts_per_tok * c.hidden_size) ||
                              dev_alloc(m, &m->moe_inds, (size_t)c.num_experts_per_tok) || dev_alloc(m, &m->moe_scores, (size_t)c.num_experts_per_tok)))
            return 1;
    }
    if (dev_alloc(m, &m->rope_cur, (size_t)D) || dev_alloc(m, &m->attn_gran, attn_step_ws_granules(m->H, D)) ||
        dev_alloc(m, &m->attn_xg, (size_t)m->H * D / 2 + 8) || dev_alloc(m, &m->chain_gran, (size_t)c.hidden_size / 2 + 8) ||
        dev_alloc(m, &m->gateup_gran, (size_t)c.hidden_size / 2 + 8) || dev_alloc(m, &m->act_gran, (size_t)m->I / 2 + 8))
        return 1;
    if (dev_alloc(m, &m->step_seq, 16) || dev_alloc(m, &m->wait_abort, 16)) return 1;
    {
        int dev = 0;
        hipDeviceProp_t prop;
        OMX_HIP_CHECK(hipGetDevice(&dev));
        OMX_HIP_CHECK(hipGetDeviceProperties(&prop, dev));
        m->cus = prop.multiProcessorCount;
        if (c.num_experts == 0 && !c.quant_bits && dev_alloc(m, &m->se_gran, step_engine_granules(c.hidden_size, m->H, m->Hkv, D, m->I))) return 1;
    }
    if (dev_alloc(m, &m->st, 1) || dev_alloc(m, &m->out_ring, (size_t)m->ring_cap) ||
        dev_alloc(m, &m->h, (size_t)c.hidden_size) || dev_alloc(m, &m->h2, (size_t)c.hidden_size) ||
        dev_alloc(m, &m->qkv, (size_t)(m->H + 2 * m->Hkv) * D) || dev_alloc(m, &m->attn_out, (size_t)m->H * D) ||
        dev_alloc(m, &m->act, (size_t)m->I) || dev_alloc(m, &m->logits, (size_t)m->V) ||
        dev_alloc(m, &m->partial_a, (size_t)c.hidden_size) || dev_alloc(m, &m->partial_b, (size_t)c.hidden_size) ||
        dev_alloc(m, &m->argmax_key, 1))
        return 1;
    if (c.num_experts > 0 && dev_alloc(m, &m->moe_partials, (size_t)c.num_experts_per_tok * c.hidden_size)) return 1;
    m->prompt_cap = m->cap;
    if (dev_alloc(m, &m->prompt_dev, (size_t)m->prompt_cap + 1)) return 1;
    m->n_argmax_partials = m->cfg.quant_bits ? qgemv_grid(m->V) : gemv_grid(m->V, c.hidden_size, EPI_ARGMAX, 0);
    if (dev_alloc(m, &m->argmax_partials, (size_t)m->n_argmax_partials)) return 1;
    OMX_HIP_CHECK(hipStreamSynchronize(m->stream));
    *out = m;
    return 0;
}

int omx_qwen3_destroy(omx_qwen3 m) {
    if (!m) return 0;
    if (m->stream) (void)hipStreamSynchronize(m->stream);
    drop_graphs(m);
    for (const bf16_t* k : m->sb_keys) quant_unregister_sb(k);
    for (void* p : m->owned) (void)hipFree(p);
    if (m->dq_buf) (void)hipFree(m->dq_buf);
    if (m->dq_slab) (void)hipFree(m->dq_slab);
    if (m->verify_logits) (void)hipFree(m->verify_logits);
    if (m->verify_tokens) (void)hipFree(m->verify_tokens);
    score_release(m);
    if (m->pf_ep_partial) (void)hipFree(m->pf_ep_partial);
    for (bf16_t* p : {m->pf_h, m->pf_h2, m->pf_xn, m->pf_q, m->pf_k, m->pf_v, m->pf_qt, m->pf_attn, m->pf_g, m->pf_u})
        if (p) (void)hipFree(p);
    if (m->ev0) (void)hipEventDestroy(m->ev0);
    if (m->ev1) (void)hipEventDestroy(m->ev1);
    if (m->stream) {
        gemm_release_stream(m->stream);
        workspace_release_stream(m->stream);
        (void)hipStreamDestroy(m->stream);
    }
    delete m;
    return 0;
}

int omx_qwen3_set_comm(omx_qwen3 m, void* comm, void* allreduce_fn) {
    OMX_REQUIRE(m, "omx_qwen3_set_comm: null model");
    OMX_REQUIRE(m->g_full == nullptr && !m->eager, "omx_qwen3_set_comm: communicator must be set before the first step");
    m->comm = comm;
    m->allreduce = (nccl_allreduce_fn)allreduce_fn;
    // OMX_PEER_FUSED=1: the O / down GEMVs reduce their own rows over the peers in their epilogue instead of a standalone
    // all-reduce kernel after them.  Opt-in: measured on one GPU (1-rank communicator, Qwen3-8B) the in-GEMV poll costs 6.5 us per
    // GEMV against 4.4 us for the extra launch -- its uncached loads queue behind the other waves' weight stream
    const bool fused = env_on("OMX_PEER_FUSED");
    m->peer_dev = (allreduce_fn == omx_peer_allreduce_fn() && fused && m->cfg.hidden_size <= kPeerMaxWords)
                      ? static_cast<const PeerDev*>(omx_peer_comm_device(comm)) : nullptr;
    return 0;
}

int omx_qwen3_set_sampler(omx_qwen3 m, float temperature, uint64_t seed) {
    OMX_REQUIRE(m, "omx_qwen3_set_sampler: null model");
    OMX_REQUIRE(temperature >= 0.f && temperature == temperature, "omx_qwen3_set_sampler: temperature %f must be >= 0", (double)temperature);
    if (!m->rng && dev_alloc(m, &m->rng, 4)) return 1;
    if (omx_random_key(m->rng, seed, (omx_stream)m->stream)) return 1;
    OMX_HIP_CHECK(hipStreamSynchronize(m->stream));
    if (temperature != m->temperature) {
        // 1/T is a launch argument inside the captured step: drop the graphs, the next step rebuilds them
        recapture_step(m);
        m->temperature = temperature;
    }
    if (m->filter_on) {   // the plain sampler: every filter and penalty off
        recapture_step(m);
        m->filter_on = false;
        m->sampling = {temperature, 0, 1.f, 1.f, 0.f};
    }
    return 0;
}

int omx_qwen3_set_sampling(omx_qwen3 m, const omx_sampling* p, uint64_t seed) {
    OMX_REQUIRE(m && p, "omx_qwen3_set_sampling: null argument");
    OMX_REQUIRE(p->temperature >= 0.f && p->temperature == p->temperature, "omx_qwen3_set_sampling: temperature %f must be >= 0", (double)p->temperature);
    OMX_REQUIRE(p->top_k >= 0, "omx_qwen3_set_sampling: top_k %d must be >= 0 (0 = off)", p->top_k);
    OMX_REQUIRE(p->top_p > 0.f && p->top_p <= 1.f, "omx_qwen3_set_sampling: top_p %f must be in (0, 1] (1 = off)", (double)p->top_p);
    OMX_REQUIRE(p->repetition_penalty > 0.f && p->repetition_penalty < INFINITY,
                "omx_qwen3_set_sampling: repetition_penalty %f must be positive (1 = off)", (double)p->repetition_penalty);
    OMX_REQUIRE(fabsf(p->presence_penalty) < INFINITY, "omx_qwen3_set_sampling: presence_penalty %f must be finite (0 = off)", (double)p->presence_penalty);
    const bool on = sampling_penalised(*p) || (p->temperature != 0.f && (p->top_k > 0 || p->top_p < 1.f));
    if (!on) return omx_qwen3_set_sampler(m, p->temperature, seed);
    OMX_REQUIRE(m->cfg.tp_size <= 1 && m->allreduce == nullptr,
                "omx_qwen3_set_sampling: filtered sampling is not supported under tensor parallelism (tp_size %d): each rank holds a "
                "vocabulary shard, the selection would need a histogram all-reduce", m->cfg.tp_size);
    OMX_REQUIRE(env_int("OMX_STEP_ENGINE", 0) <= 0 && env_int("OMX_STEP_AQL", 0) <= 0,
                "omx_qwen3_set_sampling: filtered sampling is not supported with the OMX_STEP_ENGINE / OMX_STEP_AQL step modes");
    OMX_REQUIRE(m->V <= (1 << 23), "omx_qwen3_set_sampling: vocabulary %d exceeds 2^23 entries", m->V);
    if (!m->rng && dev_alloc(m, &m->rng, 4)) return 1;
    if (!m->seen && dev_alloc(m, &m->seen, (size_t)m->V)) return 1;
    if (!m->sel && dev_alloc(m, &m->sel, sample_select_ws_bytes())) return 1;
    if (omx_random_key(m->rng, seed, (omx_stream)m->stream)) return 1;
    if (reset_sampler_history(m)) return 1;
    OMX_HIP_CHECK(hipStreamSynchronize(m->stream));
    // the parameters are launch arguments inside the captured step: drop the graphs, the next step rebuilds them
    recapture_step(m);
    m->temperature = p->temperature;
    m->sampling = *p;
    m->filter_on = true;
    return 0;
}

/* Per-token log-probabilities inside the step: the two launches of logprob.hip's top-n form behind the finalize of every sampled
 * token (enqueue_step_tail), over the raw logits row.  They are launch sites of the captured step: the graphs are dropped. */
int omx_qwen3_set_logprobs(omx_qwen3 m, int top_n) {
    OMX_REQUIRE(m, "omx_qwen3_set_logprobs: null model");
    const EngineConfig& c = m->cfg;
    OMX_REQUIRE(top_n < 0 || (c.tp_size <= 1 && c.ep_size <= 1 && m->allreduce == nullptr),
                "omx_qwen3_set_logprobs: tensor / expert parallel models are not supported (tp_size %d, ep_size %d: a rank holds a "
                "vocabulary shard, the row's log-sum-exp would need an all-reduce)", c.tp_size, c.ep_size);
    OMX_REQUIRE(top_n < 0 || !(c.num_experts > 0 && c.moe_mode == 2), "omx_qwen3_set_logprobs: moe_mode 2 (deepseek) models are not supported");
    OMX_REQUIRE(top_n < 0 || !m->f16, "omx_qwen3_set_logprobs: float16 models (float16 weights or float16 triplets) are not supported: the row reduction "
                "reads bfloat16 logits");
    OMX_REQUIRE(top_n >= -1 && top_n <= OMX_LOGPROBS_MAX_TOP && top_n <= m->V,
                "omx_qwen3_set_logprobs: top_n = %d is outside -1..min(%d, V = %d) (-1 = off, 0 = the drawn token only)", top_n,
                OMX_LOGPROBS_MAX_TOP, m->V);
    OMX_REQUIRE(top_n < 0 || (m->V % 8 == 0 && m->V <= (1 << 20)),
                "omx_qwen3_set_logprobs: vocabulary %d must be a multiple of 8 and at most 2^20 (omx_logprob_rows' shapes)", m->V);
    if (top_n >= 0 && !m->lp_ring) {
        uint8_t* scratch = nullptr;
        if (dev_alloc(m, &m->lp_ring, (size_t)m->ring_cap) || dev_alloc(m, &m->top_lp_ring, (size_t)m->ring_cap * OMX_LOGPROBS_MAX_TOP) ||
            dev_alloc(m, &m->top_id_ring, (size_t)m->ring_cap * OMX_LOGPROBS_MAX_TOP) ||
            dev_alloc(m, &scratch, logprob_top_scratch_bytes(1, m->V, OMX_LOGPROBS_MAX_TOP)))
            return 1;
        m->lp_scratch = scratch;
        OMX_HIP_CHECK(hipStreamSynchronize(m->stream));
    }
    if (top_n != m->lp_top) {
        recapture_step(m);
        m->lp_top = top_n;
        m->lp_valid = false;
    }
    return 0;
}

/* The sampler's key-sequence state (mlx-rs RandomState: two words).  The reference's speculative loop draws the draft's and the
 * target's tokens from ONE global sequence (speculative.rs:104-109: `categorical!` without a key); two engine models reproduce that by
 * handing this state back and forth.  set != 0 writes `state2` into the model, otherwise the model's state is read out. */
int omx_qwen3_sampler_state(omx_qwen3 m, uint32_t* state2, int set) {
    OMX_REQUIRE(m && state2, "omx_qwen3_sampler_state: null argument");
    OMX_REQUIRE(m->rng, "omx_qwen3_sampler_state: no sampler set (omx_qwen3_set_sampler)");
    if (set) OMX_HIP_CHECK(hipMemcpyAsync(m->rng, state2, 8, hipMemcpyHostToDevice, m->stream));
    else OMX_HIP_CHECK(hipMemcpyAsync(state2, m->rng, 8, hipMemcpyDeviceToHost, m->stream));
    OMX_HIP_CHECK(hipStreamSynchronize(m->stream));
    return 0;
}

int omx_qwen3_encode(omx_qwen3 m, const uint32_t* ids, int n, const uint8_t* attention_mask, const int* tap_layers, int n_taps,
                     void* out_dev) {
    OMX_REQUIRE(m && ids && tap_layers && out_dev, "omx_qwen3_encode: null argument");
    OMX_REQUIRE(n >= 1 && n <= m->cap, "omx_qwen3_encode: %d tokens exceed max_context %d", n, m->cap);
    OMX_REQUIRE(n_taps >= 1 && n_taps <= 16, "omx_qwen3_encode: %d taps (1..16)", n_taps);
    OMX_REQUIRE(m->cfg.tp_size == 1 && !m->allreduce, "omx_qwen3_encode: single-GPU only");
    for (int i = 0; i < n_taps; ++i)
        OMX_REQUIRE(tap_layers[i] >= 0 && tap_layers[i] < m->cfg.num_hidden_layers && (i == 0 || tap_layers[i] > tap_layers[i - 1]),
                    "omx_qwen3_encode: tap layers must be ascending and < %d", m->cfg.num_hidden_layers);
    if (resolve_weights(m)) return 1;
    hipStream_t s = m->stream;
    OMX_HIP_CHECK(hipMemcpyAsync(m->prompt_dev, ids, (size_t)n * 4, hipMemcpyHostToDevice, s));
    bf16_t* mask = nullptr;
    uint8_t* am = nullptr;
    if (attention_mask) {
        OMX_HIP_CHECK(hipMalloc((void**)&mask, (size_t)n * n * 2));
        OMX_HIP_CHECK(hipMalloc((void**)&am, (size_t)n));
        OMX_HIP_CHECK(hipMemcpyAsync(am, attention_mask, (size_t)n, hipMemcpyHostToDevice, s));
        launch_encoder_mask(mask, am, n, s);
    }
    const EncodeOpts enc = {tap_layers, n_taps, (bf16_t*)out_dev, mask};
    OMX_HIP_CHECK(hipEventRecord(m->ev0, s));
    const int rc = prefill_prefix_batched(m, n, 0, &enc);
    OMX_HIP_CHECK(hipEventRecord(m->ev1, s));
    OMX_HIP_CHECK(hipStreamSynchronize(s));
    if (mask) { (void)hipFree(mask); (void)hipFree(am); }
    if (rc) return 1;
    OMX_HIP_CHECK(hipEventElapsedTime(&m->last_prefill_ms, m->ev0, m->ev1));
    return 0;
}

int omx_qwen3_reset(omx_qwen3 m) {
    OMX_REQUIRE(m, "omx_qwen3_reset: null model");
    OMX_HIP_CHECK(hipMemsetAsync(m->st, 0, sizeof(StepState), m->stream));
    m->lp_valid = false;   // the count the rings are indexed by starts again
    if (reset_sampler_history(m)) return 1;
    OMX_HIP_CHECK(hipStreamSynchronize(m->stream));
    return 0;
}

int omx_qwen3_offset(omx_qwen3 m, int* offset) {
    OMX_REQUIRE(m && offset, "omx_qwen3_offset: null argument");
    StepState st;
    if (read_step_state(m, &st)) return 1;
    *offset = st.pos;
    return 0;
}

// omx_qwen3_prefill, and omx_qwen3_prefill_embeds (span: the caller's rows, which only the batched pass can take)
static int prefill_prompt(omx_qwen3 m, const uint32_t* prompt, int n_prompt, uint32_t* first_token, const RowSpan* span) {
    OMX_REQUIRE(n_prompt >= 1, "omx_qwen3_prefill: empty prompt");
    int off = 0;
    if (omx_qwen3_offset(m, &off)) return 1;
    OMX_REQUIRE(off + n_prompt + 1 <= m->cap, "omx_qwen3_prefill: %d cached + %d prompt tokens exceed max_context %d", off, n_prompt, m->cap);
    for (int i = 0; i < n_prompt; ++i) OMX_REQUIRE(prompt[i] < (uint32_t)m->cfg.vocab_size, "omx_qwen3_prefill: token id %u out of range (vocab %d)", prompt[i], m->cfg.vocab_size);
    OMX_REQUIRE(n_prompt <= m->prompt_cap, "omx_qwen3_prefill: prompt of %d tokens exceeds max_context %d", n_prompt, m->prompt_cap);
    const bool serial_on = env_on("OMX_PREFILL_SERIAL");
    if (span) {
        // the token-serial forms read the embedding table inside the decode step: there is no row buffer to put the caller's rows in
        OMX_REQUIRE(!serial_on, "InvalidConfig: omx_qwen3_prefill_embeds: OMX_PREFILL_SERIAL=1 sends the prompt through the decode step, which "
                    "cannot take embedding rows; unset it");
        OMX_REQUIRE(!env_on("OMX_PREFILL_TAIL_STEP"), "InvalidConfig: omx_qwen3_prefill_embeds: OMX_PREFILL_TAIL_STEP=1 sends the last token through "
                    "the decode step, which cannot take embedding rows; unset it");
        OMX_REQUIRE(n_prompt >= 2, "InvalidConfig: omx_qwen3_prefill_embeds: a one-row prompt goes through the decode step, which cannot take "
                    "embedding rows; pass at least 2 rows");
        OMX_REQUIRE(!(m->f16 && n_prompt <= 16), "InvalidConfig: omx_qwen3_prefill_embeds: a float16 model sends prompts of 16 rows or fewer "
                    "through the decode step, which cannot take embedding rows (%d rows); pass at least 17", n_prompt);
    }
    // tensor-parallel engines run the batched matrix-core prefill on their shards with two all-reduces per layer, expert-parallel ones
    // with one all-reduce of the MoE block's [T, hidden] partial per layer (round 3; token-serial before)
    // (float16 models: the batched pass exists for plain prompts -- dense and sparse-MoE models, on one rank or sharded (round 6: the
    //  float16 form of the sharded MoE block); short prompts go through the decode step)
    const bool f16_serial = m->f16 && n_prompt <= 16;
    const bool serial = serial_on || n_prompt < 2 || f16_serial;
    if (prepare_step(m, serial ? off : off + n_prompt - 1)) return 1;   // the first step this call will run (graphs are per context bucket)
    if (!serial && m->cfg.quant_bits) dq_cache_prepare(m);             // (a once-per-model allocation: ahead of the timed region)
    if (!serial && prefill_reserve(m, n_prompt)) return 1;             // (row buffers / scratch of this prompt size: likewise)
    OMX_HIP_CHECK(hipMemcpyAsync(m->prompt_dev, prompt, (size_t)n_prompt * 4, hipMemcpyHostToDevice, m->stream));
    if (reset_sampler_history(m)) return 1;   // the penalties' history: tokens sampled since this prefill
    StepState st;
    if (read_step_state(m, &st)) return 1;
    st.cur_token = prompt[0];
    st.prompt_idx = 0;
    const int count_before = st.out_count;
    OMX_HIP_CHECK(hipEventRecord(m->ev0, m->stream));
    bool batched_head = false;
    if (serial) {
        // token-serial prefill: identical arithmetic to n_prompt decode steps (the lm_head is skipped for
        // all but the last prompt position; the reference computes and discards those logits, model.rs:815)
        if (write_step_state(m, st)) return 1;
        for (int i = 0; i < n_prompt - 1; ++i)
            if (run_step(m, false, st.pos + i)) return 1;
    } else {
        // matrix-core prefill of ALL n tokens, then norm + lm_head + sampler on the last row (one more row in GEMMs whose
        // tile count does not change, instead of a 36-layer GEMV pass); OMX_PREFILL_TAIL_STEP=1: n-1 tokens batched and
        // the decode step for the last one
        // (a tensor-parallel rank's vocabulary shard + the argmax all-reduce: the end of the step on that row does both since round 4 -- until then a
        //  TP prompt ended with a whole decode step, 2 ms of a 24 ms prompt at TP 2)
        const bool tail_step = env_on("OMX_PREFILL_TAIL_STEP");
        const int nb = tail_step ? n_prompt - 1 : n_prompt;
        if (prefill_prefix_batched(m, nb, st.pos, nullptr, !tail_step, false, nullptr, nullptr, span)) return 1;
        st.pos += n_prompt - 1;
        st.prompt_idx = n_prompt - 1;
        st.cur_token = prompt[n_prompt - 1];
        if (write_step_state(m, st)) return 1;
        if (!tail_step) {
            // the last row through the end of a decode step (it is not the step graph's residual buffer; no pending partial: 0 vectors)
            const bool tp = m->allreduce != nullptr && m->cfg.ep_size <= 1;
            if (enqueue_step_tail(m, true, m->pf_h + (size_t)(n_prompt - 1) * m->cfg.hidden_size, nullptr, 0, tp)) return 1;
            batched_head = true;
        }
    }
    if (!batched_head && run_step(m, true, serial ? st.pos + n_prompt - 1 : st.pos)) return 1;
    OMX_HIP_CHECK(hipEventRecord(m->ev1, m->stream));
    OMX_HIP_CHECK(hipMemcpyAsync(first_token, m->out_ring + (count_before % m->ring_cap), 4, hipMemcpyDeviceToHost, m->stream));
    OMX_HIP_CHECK(hipStreamSynchronize(m->stream));
    OMX_HIP_CHECK(hipEventElapsedTime(&m->last_prefill_ms, m->ev0, m->ev1));
    m->lp_valid = m->lp_top >= 0;
    return step_health(m);
}

int omx_qwen3_prefill(omx_qwen3 m, const uint32_t* prompt, int n_prompt, uint32_t* first_token) {
    OMX_REQUIRE(m && prompt && first_token, "omx_qwen3_prefill: null argument");
    return prefill_prompt(m, prompt, n_prompt, first_token, nullptr);
}

/* omx_qwen3_prefill with rows [first_row, first_row + n_rows) of the pass supplied by the caller instead of gathered from the embedding
 * table -- what the reference's multimodal crates do through forward_embeddings(inputs_embeds, cache) (qwen3-asr-mlx/src/model.rs:720-769, 782:
 * the audio tower's rows over the <|audio_pad|> positions).  One more launch in the pass; the ids, the cache append, the sampler, the
 * log-probabilities and the penalty history are omx_qwen3_prefill's.  n_rows = 0 IS omx_qwen3_prefill. */
int omx_qwen3_prefill_embeds(omx_qwen3 m, const uint32_t* prompt, int n_prompt, const void* rows, omx_dtype rows_dtype, int first_row,
                             int n_rows, uint32_t* first_token) {
    OMX_REQUIRE(m && prompt && first_token, "omx_qwen3_prefill_embeds: null argument");
    OMX_REQUIRE(n_rows >= 0, "omx_qwen3_prefill_embeds: n_rows %d is negative", n_rows);
    if (n_rows == 0) return prefill_prompt(m, prompt, n_prompt, first_token, nullptr);
    OMX_REQUIRE(rows != nullptr, "omx_qwen3_prefill_embeds: null rows with n_rows %d", n_rows);
    OMX_REQUIRE(rows_dtype == OMX_FLOAT32 || rows_dtype == OMX_BFLOAT16 || rows_dtype == OMX_FLOAT16,
                "omx_qwen3_prefill_embeds: rows of dtype %d (float32, bfloat16 or float16)", (int)rows_dtype);
    OMX_REQUIRE(first_row >= 0 && first_row <= n_prompt && n_rows <= n_prompt - first_row,
                "omx_qwen3_prefill_embeds: rows [%d, %d + %d) lie outside the prompt of %d tokens", first_row, first_row, n_rows, n_prompt);
    OMX_REQUIRE(m->allreduce == nullptr && m->cfg.tp_size <= 1 && m->cfg.ep_size <= 1,
                "omx_qwen3_prefill_embeds: tensor-parallel / expert-parallel engines are not supported (single-rank models only)");
    // (moe_mode 2, the DeepSeek-V2 family: the decoder of an image-to-text model, whose prompt IS caller rows -- accepted)
    OMX_REQUIRE(m->cfg.num_experts == 0 || m->cfg.moe_mode == 2, "omx_qwen3_prefill_embeds: sparse-MoE models are not supported (dense models only)");
    const RowSpan span = {rows, rows_dtype, first_row, n_rows};
    return prefill_prompt(m, prompt, n_prompt, first_token, &span);
}

/* The model's own embedding rows of n ids, [n, hidden] in the activation dtype (bf16, or float16 for a float16 model), written to DEVICE
 * memory -- the reference's get_token_embeddings (qwen3-asr-mlx/src/model.rs:726, 814).  The launches are the prompt pass's own, so the
 * rows are the bits that pass would put in its row buffer.  The cache and the sampler are not touched. */
int omx_qwen3_embed_tokens(omx_qwen3 m, const uint32_t* ids, int n, void* out_rows) {
    OMX_REQUIRE(m && ids && out_rows, "omx_qwen3_embed_tokens: null argument");
    OMX_REQUIRE(n >= 1 && n <= m->prompt_cap, "omx_qwen3_embed_tokens: %d ids (1..%d, the prompt buffer)", n, m->prompt_cap);
    for (int i = 0; i < n; ++i) OMX_REQUIRE(ids[i] < (uint32_t)m->cfg.vocab_size, "omx_qwen3_embed_tokens: token id %u out of range (vocab %d)", ids[i], m->cfg.vocab_size);
    OMX_REQUIRE(m->allreduce == nullptr && m->cfg.tp_size <= 1 && m->cfg.ep_size <= 1,
                "omx_qwen3_embed_tokens: tensor-parallel / expert-parallel engines are not supported (single-rank models only)");
    if (resolve_weights(m)) return 1;
    if (m->cfg.quant_bits && prefill_reserve(m, n, /*dequant=*/false)) return 1;   // (the gather's scratch lies in the row buffers)
    OMX_HIP_CHECK(hipMemcpyAsync(m->prompt_dev, ids, (size_t)n * 4, hipMemcpyHostToDevice, m->stream));
    if (embed_rows(m, (bf16_t*)out_rows, n, /*rows_form=*/false)) return 1;
    OMX_HIP_CHECK(hipStreamSynchronize(m->stream));
    return 0;
}

/* Speculative decoding (mlx-rs-core/src/speculative.rs).  `verify` is verify_draft_tokens (:132-161): the target model runs ALL n
 * tokens [last accepted, draft 1 .. draft n-1] in one batched pass on top of its cache (their K/V rows are appended) and returns the
 * greedy token of every position -- the weights stream once for all rows: bf16 weights through the matrix-core GEMMs (the lm_head one
 * [n, V] GEMM), packed weights (2/3/4/5/6/8-bit, bf16 scales) through the few-row packed GEMV of qgemv_rows.hip in blocks of <= 8
 * rows, lm_head included, with no weight dequantised.  Afterwards the cache holds n more tokens and the next step's input token is
 * greedy_out[n-1]; the caller then drops the rejected tail with omx_qwen3_trim.  Single-rank dense models (a vocabulary-sharded head
 * has no batched form here; packed experts and float16 triplets are refused). */
int omx_qwen3_verify(omx_qwen3 m, const uint32_t* tokens, int n, uint32_t* greedy_out) {
    OMX_REQUIRE(m && tokens && greedy_out, "omx_qwen3_verify: null argument");
    OMX_REQUIRE(n >= 1 && n <= 64, "omx_qwen3_verify: %d tokens (1..64 per call)", n);
    OMX_REQUIRE(!m->filter_on, "omx_qwen3_verify: filtered sampling (top-k / top-p / penalties, omx_qwen3_set_sampling) is on: speculative "
                "verify draws from unfiltered rows; call omx_qwen3_set_sampler first");
    OMX_REQUIRE(m->allreduce == nullptr && m->cfg.tp_size <= 1 && m->cfg.ep_size <= 1,
                "omx_qwen3_verify: tensor / expert parallel models are not supported (single-rank models only)");
    const bool packed = m->cfg.quant_bits != 0;
    OMX_REQUIRE(!(m->cfg.num_experts > 0 && m->cfg.moe_mode == 2), "omx_qwen3_verify: moe_mode 2 (deepseek) models are not supported");
    OMX_REQUIRE(!m->cfg.float16_weights, "omx_qwen3_verify: dense float16 models (float16_weights) are not supported; speculative verify runs "
                "on bf16 weights or bf16-scale packed weights");
    OMX_REQUIRE(!packed || !m->cfg.quant_scales_f16,
                "omx_qwen3_verify: float16 triplets (scales_dtype float16) are not supported on packed models; bf16 scales only");
    OMX_REQUIRE(!packed || m->cfg.num_experts == 0, "omx_qwen3_verify: packed models with experts (MoE) are not supported; dense models only");
    for (int i = 0; i < n; ++i) OMX_REQUIRE(tokens[i] < (uint32_t)m->cfg.vocab_size, "omx_qwen3_verify: token id %u out of range (vocab %d)", tokens[i], m->cfg.vocab_size);
    StepState st;
    if (read_step_state(m, &st)) return 1;
    OMX_REQUIRE(st.pos + n + 1 <= m->cap, "omx_qwen3_verify: %d cached + %d tokens exceed max_context %d", st.pos, n, m->cap);
    OMX_REQUIRE(n <= m->prompt_cap, "omx_qwen3_verify: %d tokens exceed the prompt buffer", n);
    if (resolve_weights(m)) return 1;          // (verify may be the first call on a fresh model)
    hipStream_t s = m->stream;
    const int hd = m->cfg.hidden_size, V = m->V;
    if (n > m->verify_cap) {
        OMX_HIP_CHECK(hipStreamSynchronize(s));
        if (m->verify_logits) OMX_HIP_CHECK(hipFree(m->verify_logits));
        if (m->verify_tokens) OMX_HIP_CHECK(hipFree(m->verify_tokens));
        m->verify_logits = nullptr; m->verify_tokens = nullptr; m->verify_cap = 0;
        const int cap = std::max(n, 16);
        OMX_HIP_CHECK(hipMalloc((void**)&m->verify_logits, (size_t)cap * V * sizeof(bf16_t)));
        OMX_HIP_CHECK(hipMalloc((void**)&m->verify_tokens, (size_t)cap * 4));
        m->verify_cap = cap;
    }
    OMX_HIP_CHECK(hipMemcpyAsync(m->prompt_dev, tokens, (size_t)n * 4, hipMemcpyHostToDevice, s));
    if (prefill_prefix_batched(m, n, st.pos, nullptr, /*full_last=*/true, /*packed_rows_pass=*/packed)) return 1;
    // [final RMSNorm rows] -> [lm_head GEMM, n x V] -> [argmax per row]   (model.rs:423, 480-489; sampler.rs:9-18 at temperature 0)
    if (packed) {   // the packed head (or the tied q_embed table), the final RMSNorm as its prologue
        QGemvArgs a = {};
        a.m[0] = m->q_head; a.m[0].n = V; a.N = V; a.K = hd; a.group = m->q_head.group;   // the head's own format
        a.x = m->pf_h; a.norm_w = m->final_norm; a.eps = m->cfg.rms_norm_eps; a.out = m->verify_logits;
        if (packed_rows(a, n, nullptr, m->q_head.bits, PRO_RMSNORM, EPI_STORE, s)) return 1;
    } else {
        if (omx_rms_norm(m->pf_xn, m->pf_h, m->final_norm, n, hd, m->cfg.rms_norm_eps, OMX_BFLOAT16, s)) return 1;
        if (launch_gemm_bf16(m->verify_logits, m->pf_xn, m->lm_head, nullptr, n, V, hd, s)) return 1;
    }
    if (m->temperature == 0.f) {
        if (omx_argmax(m->verify_tokens, m->verify_logits, n, V, OMX_BFLOAT16, s)) return 1;
    } else {
        // speculative.rs:104-109 + :145-148: every position draws categorical(logits / T) with the NEXT key of the sequence -- one
        // [1, V] draw per row, exactly what a decode step does with its row
        for (int i = 0; i < n; ++i) {
            if (launch_rng_next(m->rng, s)) return 1;
            if (omx_random_categorical(m->verify_tokens + i, m->verify_logits + (size_t)i * V, 1, V, 1, 1.0f / m->temperature, m->rng + 2,
                                       OMX_BFLOAT16, (omx_stream)s))
                return 1;
        }
    }
    OMX_HIP_CHECK(hipMemcpyAsync(greedy_out, m->verify_tokens, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    OMX_HIP_CHECK(hipStreamSynchronize(s));
    st.pos += n;
    st.cur_token = greedy_out[n - 1];
    if (write_step_state(m, st)) return 1;
    OMX_HIP_CHECK(hipStreamSynchronize(s));
    m->verify_rows = n;
    return 0;
}

/* bf16 logits [V] of row `row` of the last omx_qwen3_verify (the caller derives logprobs = logits - logsumexp, speculative.rs:150-152) */
int omx_qwen3_verify_logits(omx_qwen3 m, int row, void* host_bf16, int n) {
    OMX_REQUIRE(m && host_bf16, "omx_qwen3_verify_logits: null argument");
    OMX_REQUIRE(row >= 0 && row < m->verify_rows, "omx_qwen3_verify_logits: row %d of %d", row, m->verify_rows);
    OMX_REQUIRE(n == m->V, "omx_qwen3_verify_logits: expected %d entries, got %d", m->V, n);
    OMX_HIP_CHECK(hipMemcpyAsync(host_bf16, m->verify_logits + (size_t)row * m->V, (size_t)n * 2, hipMemcpyDeviceToHost, m->stream));
    OMX_HIP_CHECK(hipStreamSynchronize(m->stream));
    return 0;
}

/* KeyValueCache::trim -- the operation speculative.rs:165-169 notes the reference's cache trait lacks: forget the last n cached
 * tokens (their slab rows are simply overwritten by later appends) and make `next_token` the next step's input.  n = 0 only
 * replaces the pending input token. */
int omx_qwen3_trim(omx_qwen3 m, int n, uint32_t next_token) {
    OMX_REQUIRE(m, "omx_qwen3_trim: null argument");
    OMX_REQUIRE(!m->filter_on, "omx_qwen3_trim: filtered sampling (top-k / top-p / penalties, omx_qwen3_set_sampling) is on: the token "
                "history on the device cannot be trimmed; call omx_qwen3_set_sampler first");
    OMX_REQUIRE(next_token < (uint32_t)m->cfg.vocab_size, "omx_qwen3_trim: token id %u out of range (vocab %d)", next_token, m->cfg.vocab_size);
    StepState st;
    if (read_step_state(m, &st)) return 1;
    OMX_REQUIRE(n >= 0 && n <= st.pos, "omx_qwen3_trim: cannot drop %d of %d cached tokens", n, st.pos);
    st.pos -= n;
    st.cur_token = next_token;
    if (write_step_state(m, st)) return 1;
    OMX_HIP_CHECK(hipStreamSynchronize(m->stream));
    return 0;
}

/* bytes the engine holds for dequantised weights: the dequant cache's slab plus the scratch of the prompt pass's GEMM operands */
int omx_qwen3_dequant_bytes(omx_qwen3 m, size_t* bytes) {
    OMX_REQUIRE(m && bytes, "omx_qwen3_dequant_bytes: null argument");
    *bytes = (m->dq_slab ? m->dq_slab_bytes : 0) + (m->dq_buf ? m->dq_cap * sizeof(bf16_t) : 0);
    return 0;
}

int omx_qwen3_last_prefill_ms(omx_qwen3 m, float* ms) {
    OMX_REQUIRE(m && ms, "omx_qwen3_last_prefill_ms: null argument");
    *ms = m->last_prefill_ms;
    return 0;
}

// n decode steps; logprobs != null: also the rings' entries of those steps (omx_qwen3_decode_logprobs, which has checked that they exist)
static int decode_steps(omx_qwen3 m, int n, uint32_t* tokens_out, float* logprobs, uint32_t* top_ids, float* top_logprobs) {
    OMX_REQUIRE(n >= 0 && n <= m->ring_cap, "omx_qwen3_decode: n=%d out of range (1..%d per call)", n, m->ring_cap);
    if (n == 0) return 0;
    StepState st;
    if (read_step_state(m, &st)) return 1;
    if (prepare_step(m, st.pos)) return 1;
    OMX_REQUIRE(st.pos + n <= m->cap, "omx_qwen3_decode: %d cached + %d new tokens exceed max_context %d", st.pos, n, m->cap);
    for (;;) {
        // all n steps stay inside one split plan (one captured form)?  then the AQL program, if there is one, replays them
        const bool aql = m->aql_full && step_aql_mode(m) && context_bucket(m, st.pos + n) == m->graph_tk_max;
        if (aql) {
            double ms = 0.0;
            if (aql_replay(m->aql_full, n, &ms)) {   // the queue is unusable: the error stands, later calls use the graph
                m->aql_disabled = true;
                return 1;
            }
            m->last_decode_ms = (float)ms;
        } else {
            OMX_HIP_CHECK(hipEventRecord(m->ev0, m->stream));
            for (int i = 0; i < n; ++i)
                if (run_step(m, true, st.pos + i)) return 1;
            OMX_HIP_CHECK(hipEventRecord(m->ev1, m->stream));
            OMX_HIP_CHECK(hipStreamSynchronize(m->stream));
            OMX_HIP_CHECK(hipEventElapsedTime(&m->last_decode_ms, m->ev0, m->ev1));
        }
        unsigned gave_up = 0;
        if (step_gave_up(m, &gave_up)) return 1;
        if (!gave_up) break;
        if (step_fallback(m, st)) return step_health(m);   // no form with less co-residency left: report
        if (prepare_step(m, st.pos)) return 1;
    }
    std::vector<uint32_t> ring(m->ring_cap);
    OMX_HIP_CHECK(hipMemcpy(ring.data(), m->out_ring, (size_t)m->ring_cap * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) tokens_out[i] = ring[(st.out_count + i) % m->ring_cap];
    m->lp_valid = m->lp_top >= 0;
    if (!logprobs) return 0;
    const size_t top = (size_t)m->lp_top;
    std::vector<float> lp(m->ring_cap), tlp(top_logprobs ? m->ring_cap * top : 0);
    std::vector<uint32_t> ids(top_ids ? m->ring_cap * top : 0);
    OMX_HIP_CHECK(hipMemcpy(lp.data(), m->lp_ring, lp.size() * 4, hipMemcpyDeviceToHost));
    if (!tlp.empty()) OMX_HIP_CHECK(hipMemcpy(tlp.data(), m->top_lp_ring, tlp.size() * 4, hipMemcpyDeviceToHost));
    if (!ids.empty()) OMX_HIP_CHECK(hipMemcpy(ids.data(), m->top_id_ring, ids.size() * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) {
        const size_t at = (size_t)((st.out_count + i) % m->ring_cap);
        logprobs[i] = lp[at];
        if (!tlp.empty()) memcpy(top_logprobs + i * top, tlp.data() + at * top, top * 4);
        if (!ids.empty()) memcpy(top_ids + i * top, ids.data() + at * top, top * 4);
    }
    return 0;
}

int omx_qwen3_decode(omx_qwen3 m, int n, uint32_t* tokens_out) {
    OMX_REQUIRE(m && tokens_out, "omx_qwen3_decode: null argument");
    return decode_steps(m, n, tokens_out, nullptr, nullptr, nullptr);
}

int omx_qwen3_decode_logprobs(omx_qwen3 m, int n, uint32_t* tokens_out, float* logprobs, uint32_t* top_ids, float* top_logprobs) {
    OMX_REQUIRE(m && tokens_out && logprobs, "omx_qwen3_decode_logprobs: null argument");
    OMX_REQUIRE(m->lp_top >= 0, "omx_qwen3_decode_logprobs: log-probabilities are off (omx_qwen3_set_logprobs)");
    return decode_steps(m, n, tokens_out, logprobs, top_ids, top_logprobs);
}

int omx_qwen3_last_logprobs(omx_qwen3 m, float* logprob, uint32_t* top_ids, float* top_logprobs) {
    OMX_REQUIRE(m && logprob, "omx_qwen3_last_logprobs: null argument");
    OMX_REQUIRE(m->lp_top >= 0, "omx_qwen3_last_logprobs: log-probabilities are off (omx_qwen3_set_logprobs)");
    OMX_REQUIRE(m->lp_valid, "omx_qwen3_last_logprobs: no token has been sampled since omx_qwen3_set_logprobs / omx_qwen3_reset");
    StepState st;
    if (read_step_state(m, &st)) return 1;
    OMX_REQUIRE(st.out_count >= 1, "omx_qwen3_last_logprobs: no token has been sampled yet");
    const size_t at = (size_t)((st.out_count - 1) % m->ring_cap), top = (size_t)m->lp_top;
    OMX_HIP_CHECK(hipMemcpy(logprob, m->lp_ring + at, 4, hipMemcpyDeviceToHost));
    if (top_ids && top) OMX_HIP_CHECK(hipMemcpy(top_ids, m->top_id_ring + at * top, top * 4, hipMemcpyDeviceToHost));
    if (top_logprobs && top) OMX_HIP_CHECK(hipMemcpy(top_logprobs, m->top_lp_ring + at * top, top * 4, hipMemcpyDeviceToHost));
    return 0;
}

int omx_qwen3_last_logits(omx_qwen3 m, void* host_bf16, int n) {
    OMX_REQUIRE(m && host_bf16, "omx_qwen3_last_logits: null argument");
    OMX_REQUIRE(n == m->V, "omx_qwen3_last_logits: expected %d entries, got %d", m->V, n);
    OMX_HIP_CHECK(hipMemcpyAsync(host_bf16, m->logits, (size_t)n * 2, hipMemcpyDeviceToHost, m->stream));
    OMX_HIP_CHECK(hipStreamSynchronize(m->stream));
    return 0;
}

// the device buffer a debug name stands for (omx_qwen3_debug_read / _write); null: unknown name or layer
static void* debug_buffer(omx_qwen3 m, const char* name) {
    void* src = nullptr;
    const std::string s(name);
    if (s == "h") src = m->h;
    else if (s == "h2") src = m->h2;
    else if (s == "qkv") src = m->qkv;
    else if (s == "attn_out") src = m->attn_out;
    else if (s == "act") src = m->act;
    else if (s.rfind("g_", 0) == 0 && m->se_gran) {   // granule buffers of the persistent step (8 bytes each: n_elems = 4 x granules)
        const size_t hd = m->cfg.hidden_size, D = m->cfg.head_dim;
        uint64_t* g = m->se_gran;
        if (s == "g_x") src = g;
        else if (s == "g_x1") src = g + hd / 2;
        else if (s == "g_qkv") src = g + hd;
        else if (s == "g_attn") src = g + hd + (size_t)(m->H + 2 * m->Hkv) * D / 2;
        else if (s == "g_act") src = g + hd + (size_t)(m->H + 2 * m->Hkv) * D / 2 + (size_t)m->H * D / 2;
    }
    else if (s.size() > 1 && (s[0] == 'k' || s[0] == 'v')) {
        const int l = atoi(s.c_str() + 1);
        if (l >= 0 && l < (int)m->kcache.size()) src = s[0] == 'k' ? m->kcache[l] : m->vcache[l];
    }
    return src;
}

/* test/debug hook: copy an internal bf16 buffer to the host ("h","h2","qkv","attn_out","act","k<l>","v<l>") */
int omx_qwen3_debug_read(omx_qwen3 m, const char* name, void* host, size_t n_elems) {
    OMX_REQUIRE(m && name && host, "omx_qwen3_debug_read: null argument");
    const void* src = debug_buffer(m, name);
    OMX_REQUIRE(src != nullptr, "omx_qwen3_debug_read: unknown buffer or layer %s", name);
    OMX_HIP_CHECK(hipMemcpyAsync(host, src, n_elems * 2, hipMemcpyDeviceToHost, m->stream));
    OMX_HIP_CHECK(hipStreamSynchronize(m->stream));
    return 0;
}

/* ... and the other way: n_elems 16-bit patterns from the host into the buffer (a test poisons `act` to see every element rewritten) */
int omx_qwen3_debug_write(omx_qwen3 m, const char* name, const void* host, size_t n_elems) {
    OMX_REQUIRE(m && name && host, "omx_qwen3_debug_write: null argument");
    void* dst = debug_buffer(m, name);
    OMX_REQUIRE(dst != nullptr, "omx_qwen3_debug_write: unknown buffer %s", name);
    OMX_HIP_CHECK(hipMemcpyAsync(dst, host, n_elems * 2, hipMemcpyHostToDevice, m->stream));
    OMX_HIP_CHECK(hipStreamSynchronize(m->stream));
    return 0;
}

int omx_qwen3_last_decode_ms(omx_qwen3 m, float* ms) {
    OMX_REQUIRE(m && ms, "omx_qwen3_last_decode_ms: null argument");
    *ms = m->last_decode_ms;
    return 0;
}

int omx_qwen3_stream(omx_qwen3 m, omx_stream* s) {
    OMX_REQUIRE(m && s, "omx_qwen3_stream: null argument");
    *s = (omx_stream)m->stream;
    return 0;
}

/* debug hook (tools/attn_step_trace.py): run ONE decode step eagerly with the attention launches stamping the 100 MHz wall clock:
 * host receives [layers][attn splits][kv heads][16] = {block start, loads landed + q/k normed and roped, own chunk done, granules
 * stored, gathered and merged (consumer blocks), attention vector swept, O rows stored, partials parked; with gate/up in the launch
 * (csrc/attn_step.hip gateup_phase): [4] of an O block the hidden row swept, [7] first pair reduced, [8] / [9] last pair of wave 0 / of
 * wave 7 reduced, [10] NOT a stamp: the pairs the block's waves reduced (48 each); with down + the next q/k/v in the launch as well
 * (down_qkv_phase): [11] activation vector swept, [12] first down unit of wave 0 reduced, [13] residual row swept, [14] q/k/v rows stored,
 * [15] NOT a stamp: the down units the block reduced (32) | the q/k/v rows it stored (24) << 32; the rest 0}; *blocks = splits * kv heads */
int omx_qwen3_debug_trace_step(omx_qwen3 m, unsigned long long* host, size_t n_words, int* blocks) {
    OMX_REQUIRE(m && host && blocks, "omx_qwen3_debug_trace_step: null argument");
    StepState st;
    if (read_step_state(m, &st)) return 1;
    if (prepare_step(m, st.pos)) return 1;
    const size_t per_layer = (size_t)m->attn_nsplit * m->Hkv * kAttnTraceWords, need = per_layer * m->cfg.num_hidden_layers;
    OMX_REQUIRE(n_words >= need, "omx_qwen3_debug_trace_step: buffer of %zu words, need %zu", n_words, need);
    unsigned long long* dev = nullptr;
    OMX_HIP_CHECK(hipMalloc(&dev, need * 8));
    OMX_HIP_CHECK(hipMemsetAsync(dev, 0, need * 8, m->stream));
    m->attn_trace = dev;
    const int rc = enqueue_step(m, true);
    m->attn_trace = nullptr;
    if (!rc) {
        OMX_HIP_CHECK(hipStreamSynchronize(m->stream));
        OMX_HIP_CHECK(hipMemcpy(host, dev, need * 8, hipMemcpyDeviceToHost));
    }
    (void)hipFree(dev);
    *blocks = m->attn_nsplit * m->Hkv;
    return rc ? 1 : step_health(m);
}

/* measurement hook (bench.py roofline.achieved): runs `steps` REAL decode steps (they advance the context like any other) eagerly, each
 * launch of the five per-layer kernels and the lm_head carrying its own HIP event pair (hipExtLaunchKernelGGL start / stop events: the
 * dispatch's begin / end timestamps on the step's stream, launch_timing.hpp).  us[6] = average of {QKV GEMV, attention, O GEMV,
 * gate/up + SwiGLU GEMV, down GEMV, lm_head} over layers and steps.  Dense bf16 single-rank models only.
 * Where down and the next layer's q/k/v are one launch (gemv_chain.hip, layers 0 .. L-2), that launch is booked on the down class of its
 * layer and its duration is split between `down` and `qkv` in proportion to their algorithmic bytes: the q/k/v pairs of layers 1 .. L-1
 * are never armed and never read, no class comes back as 0 and the classes still sum to the step.
 * Where gate/up + SwiGLU rides in the attention launch (attention_takes_gateup), that launch is booked on the attention class and its
 * duration is split the same way between `attention` (the K/V rows read at this position + the O matrix) and `gate_up`.
 * Where that launch is the layer's only one (attention_takes_down: + down + the next layer's q/k/v), the down pair of the layer is never
 * armed either and the duration is split four ways, `down` and `qkv` taking their bytes' share as well. */
int omx_qwen3_time_step_kernels(omx_qwen3 m, int steps, float* us) {
    OMX_REQUIRE(m && us && steps > 0, "omx_qwen3_time_step_kernels: bad arguments");
    OMX_REQUIRE(!m->cfg.quant_bits && m->cfg.num_experts == 0 && m->allreduce == nullptr, "omx_qwen3_time_step_kernels: dense bf16 single-rank models only");
    const int L = m->cfg.num_hidden_layers;
    std::vector<hipEvent_t> ev((size_t)(L * kLayerClasses + 2) * 2);
    for (auto& e : ev) OMX_HIP_CHECK(hipEventCreate(&e));
    double sum[KC_COUNT] = {};
    int rc = 0;
    bool fused_o = false, engine = false, hybrid = false, chain = false;
    const double o_bytes = (double)m->H * m->cfg.head_dim * m->cfg.hidden_size, gu_bytes = 2.0 * m->cfg.hidden_size * m->I;
    const double qkv_bytes = (double)(m->H + 2 * m->Hkv) * m->cfg.head_dim * m->cfg.hidden_size, down_bytes = (double)m->cfg.hidden_size * m->I;
    arm_launch_events(nullptr, nullptr);
    for (int it = 0; it < steps && !rc; ++it) {
        StepState st;
        if (read_step_state(m, &st)) { rc = 1; break; }
        if (st.pos + 1 > m->cap) { set_error("omx_qwen3_time_step_kernels: context full"); rc = 1; break; }
        if (prepare_step(m, st.pos)) { rc = 1; break; }
        fused_o = any_layer_takes_oproj(m);
        engine = step_engine_mode(m) == 1;
        hybrid = step_engine_mode(m) == 2;
        chain = !engine && !hybrid && down_takes_qkv(m);
        m->kernel_events = &ev;
        rc = enqueue_step(m, true);
        m->kernel_events = nullptr;
        if (rc) break;
        OMX_HIP_CHECK(hipStreamSynchronize(m->stream));
        for (int l = (engine ? L : 0); l <= L; ++l)
            for (int k = 0; k < (l == L ? (engine ? 2 : 1) : kLayerClasses); ++k) {
                float ms = 0.f;
                const size_t i = ((size_t)l * kLayerClasses + k) * 2;
                if (l < L && k == KC_O && fused_o) continue;     // that pair was never armed
                if (hybrid && l < L && (k == KC_GATE_UP || (k == KC_DOWN && l != L - 1))) continue;   // one segment launch covers them
                if (chain && l > 0 && l < L && k == KC_QKV) continue;   // done inside the previous layer's down launch
                const bool gateup = l < L && !engine && !hybrid && attention_takes_gateup(m, l);
                if (gateup && k == KC_GATE_UP) continue;         // done inside the layer's attention launch
                const bool down = gateup && chain && attention_takes_down(m, l);
                if (down && k == KC_DOWN) continue;              // likewise
                OMX_HIP_CHECK(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
                if (gateup && k == KC_ATTN) {   // one launch for two classes: shared by bytes
                    const double attn_bytes = 2.0 * m->Hkv * m->cfg.head_dim * (st.pos + 1) + o_bytes;
                    const double all_bytes = gu_bytes + attn_bytes + (down ? down_bytes + qkv_bytes : 0.0);
                    sum[KC_GATE_UP] += ms * 1e3 * (gu_bytes / all_bytes);
                    if (down) {
                        sum[KC_DOWN] += ms * 1e3 * (down_bytes / all_bytes);
                        sum[KC_QKV] += ms * 1e3 * (qkv_bytes / all_bytes);
                    }
                    ms *= (float)(attn_bytes / all_bytes);
                }
                if (chain && l < L - 1 && k == KC_DOWN) {   // one launch for two classes: shared by bytes
                    sum[KC_QKV] += ms * 1e3 * (qkv_bytes / (qkv_bytes + down_bytes));
                    ms *= (float)(down_bytes / (qkv_bytes + down_bytes));
                }
                sum[l == L ? (k == 0 ? KC_HEAD : KC_ENGINE) : k] += ms * 1e3;
            }
        rc = step_health(m);
    }
    arm_launch_events(nullptr, nullptr);   // (a pair armed for a launch that never happened must not outlive its events)
    for (auto& e : ev) (void)hipEventDestroy(e);
    if (rc) return 1;
    for (int k = 0; k < KC_COUNT; ++k) us[k] = (float)(sum[k] / ((k == KC_HEAD || k == KC_ENGINE ? 1.0 : (double)L) * steps));
    if (fused_o) us[KC_O] = 0.f;   // no separate launch: its work is inside the attention figure
    return 0;
}

/* debug hook (tools/step_engine_trace.py): ONE eager decode step on the persistent engine with per-CU wall-clock stamps:
 * host receives [CUs][64] words (12 per layer for the first four layers: layer start, x ready, qkv done, partials out, attention done,
 * attention vector ready, o done, x1 ready, gate/up done, act ready, down done); *cus_out = CUs */
int omx_qwen3_debug_trace_engine(omx_qwen3 m, unsigned long long* host, size_t n_words, int* cus_out) {
    OMX_REQUIRE(m && host && cus_out, "omx_qwen3_debug_trace_engine: null argument");
    StepState st;
    if (read_step_state(m, &st)) return 1;
    if (prepare_step(m, st.pos)) return 1;
    OMX_REQUIRE(step_engine_takes(m), "omx_qwen3_debug_trace_engine: the persistent step is off or the model does not qualify");
    const size_t need = (size_t)m->cus * kStepEngineTraceWords;
    OMX_REQUIRE(n_words >= need, "omx_qwen3_debug_trace_engine: buffer of %zu words, need %zu", n_words, need);
    unsigned long long* dev = nullptr;
    OMX_HIP_CHECK(hipMalloc(&dev, need * 8));
    OMX_HIP_CHECK(hipMemsetAsync(dev, 0, need * 8, m->stream));
    m->se_trace = dev;
    const int rc = enqueue_step(m, true);
    m->se_trace = nullptr;
    if (!rc) {
        OMX_HIP_CHECK(hipStreamSynchronize(m->stream));
        OMX_HIP_CHECK(hipMemcpy(host, dev, need * 8, hipMemcpyDeviceToHost));
    }
    (void)hipFree(dev);
    *cus_out = m->cus;
    return rc ? 1 : step_health(m);
}

int omx_qwen3_decode_path(omx_qwen3 m, int* path) {
    OMX_REQUIRE(m && path, "omx_qwen3_decode_path: null argument");
    *path = m->eager ? 2 : (m->aql_full && step_aql_mode(m)) ? 3 : m->g_full ? 1 : 0;   // 3: AQL replay on the engine's own queue
    // bits 8..11: the rungs of step_fallback's ladder this engine has gone down, in the ladder's order
    *path |= (m->gateup_disabled ? 1 : 0) << 8 | (m->chain_disabled ? 1 : 0) << 9 | (m->se_disabled ? 1 : 0) << 10 | (m->oproj_disabled ? 1 : 0) << 11;
    return 0;
}

int omx_qwen3_step_bytes(omx_qwen3 m, int ctx, double* bytes) {
    OMX_REQUIRE(m && bytes, "omx_qwen3_step_bytes: null argument");
    const EngineConfig& c = m->cfg;
    const double D = c.head_dim, hd = c.hidden_size;
    // 2 B x [L (h H D + 2 h Hkv D + H D h + 3 h I) + V h] + ctx (2 L Hkv D 2 B) + KV write
    // sparse MoE: the router plus the top-k experts' three matrices are what one token streams
    const double moe_i = c.tp_size > 1 && c.num_experts > 0 ? m->moe_I : c.moe_intermediate_size;   // (expert tensor parallel: this rank's columns)
    // (mode 2: the shared experts stream with every token, and the first first_k_dense_replace layers are dense)
    const double ffn_moe = hd * c.num_experts + 3.0 * hd * moe_i * (c.num_experts_per_tok + (c.moe_mode == 2 ? c.n_shared_experts : 0));
    const double n_dense = c.num_experts == 0 ? c.num_hidden_layers : (c.moe_mode == 2 ? c.first_k_dense_replace : 0);
    const double ffn = (n_dense * 3.0 * hd * m->I + (c.num_hidden_layers - n_dense) * ffn_moe) / c.num_hidden_layers;   // mean over the layer plan
    const double per_layer = hd * m->H * D + 2.0 * hd * m->Hkv * D + m->H * D * hd + ffn;
    // bytes per weight element: bf16 = 2; quantized = bits/8 packed + (scale + bias) bf16 per group
    const double bpe = c.quant_bits ? c.quant_bits / 8.0 + 4.0 / c.quant_group : 2.0;
    double w = bpe * (c.num_hidden_layers * per_layer + (double)m->V * hd);
    if (c.quant_bits && c.num_experts == 0 && !m->quant_formats.empty()) {   // per-matrix formats: every matrix at its own width
        auto at = [&](const std::string& prefix, double n, double k) {
            const std::pair<int, int> f = quant_format_of(m, prefix);
            return n * k * (f.first / 8.0 + 4.0 / f.second);
        };
        w = at(c.tie_word_embeddings ? "model.embed_tokens" : "lm_head", m->V, hd);
        for (int l = 0; l < c.num_hidden_layers; ++l) {
            const std::string p = "model.layers." + std::to_string(l) + ".";
            w += at(p + "self_attn.q_proj", m->H * D, hd) + at(p + "self_attn.k_proj", m->Hkv * D, hd) + at(p + "self_attn.v_proj", m->Hkv * D, hd) +
                 at(p + "self_attn.o_proj", hd, m->H * D) + at(p + "mlp.gate_proj", m->I, hd) + at(p + "mlp.up_proj", m->I, hd) + at(p + "mlp.down_proj", hd, m->I);
        }
    }
    const double kv = (double)ctx * (2.0 * c.num_hidden_layers * m->Hkv * D * 2.0) + 2.0 * c.num_hidden_layers * m->Hkv * D * 2.0;
    *bytes = w + kv;
    return 0;
}

}  // extern "C"
