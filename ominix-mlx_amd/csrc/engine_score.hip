// omx_qwen3_score: per-token log-probabilities of a text from ONE batched prompt pass (include/omx.h "Score a text").
//
// The reference applies lm_head to all L positions (qwen3-mlx/src/model.rs:480-490) and a caller log-softmaxes the [B, L, V] logits; at
// Qwen3-8B's vocabulary that tensor is 622 MB per 2 048 tokens.  Here the head runs over all n rows in vocabulary PANELS:
//
//   [final RMSNorm, n rows] -> per panel of P columns: ([dequantise the panel's head rows, packed heads]
//                                                      [panel GEMM n x P' x hidden] [chunk partials, logprob.hip]) -> [merge, n rows]
//
// One panel buffer [n, P] bf16 is written and read once per panel (2 * n * V * 2 bytes of traffic in total, none of it a [n, V] tensor);
// the logits are the GEMM's bf16 outputs, the rounding point the engine's logits have everywhere.  The chunk grid of the statistics is a
// function of V alone, so the panel width changes no bit of them; it can change which GEMM kernel a panel takes.
// Bookkeeping is omx_qwen3_verify's (engine.hip): the rows are appended to the cache, the pending token is the last row's argmax.
#include "engine_model.hpp"

namespace omx {

void score_release(omx_qwen3 m) {
    if (m->score_panel_buf) (void)hipFree(m->score_panel_buf);
    if (m->score_dq) (void)hipFree(m->score_dq);
    if (m->score_part) (void)hipFree(m->score_part);
    for (hipEvent_t& e : m->score_ev)
        if (e) { (void)hipEventDestroy(e); e = nullptr; }
    m->score_panel_buf = m->score_dq = nullptr;
    m->score_part = m->score_tgt = m->score_lp = nullptr;
    m->score_arg = m->score_targets = m->score_greedy = nullptr;
    m->score_rows = m->score_panel = 0;
    m->score_dq_on = false;
}

namespace {

// panel [rows, P] bf16; one allocation of f32 / u32 words: partials [rows, nch, 2] | part_arg [rows, nch] | tgt | logprobs | targets |
// greedy [rows] each; packed heads: the panel's dequantised rows [P, hidden].  Allocated on first use, reallocated on growth.
int score_reserve(omx_qwen3 m, int n, int P, bool packed) {
    if (n <= m->score_rows && P <= m->score_panel && (!packed || m->score_dq_on)) return 0;
    OMX_HIP_CHECK(hipStreamSynchronize(m->stream));
    const int rows = std::max(std::max(n, m->score_rows), 16), panel = std::max(P, m->score_panel);
    hipEvent_t ev[3] = {m->score_ev[0], m->score_ev[1], m->score_ev[2]};
    for (hipEvent_t& e : m->score_ev) e = nullptr;   // (kept across the reallocation)
    score_release(m);
    for (int i = 0; i < 3; ++i) m->score_ev[i] = ev[i];
    const size_t nch = (size_t)(m->V + OMX_LOGPROB_CHUNK - 1) / OMX_LOGPROB_CHUNK;
    OMX_HIP_CHECK(hipMalloc((void**)&m->score_panel_buf, (size_t)rows * panel * sizeof(bf16_t)));
    OMX_HIP_CHECK(hipMalloc((void**)&m->score_part, ((size_t)rows * nch * 3 + (size_t)rows * 4) * 4));
    m->score_arg = (uint32_t*)(m->score_part + (size_t)rows * nch * 2);
    m->score_tgt = (float*)(m->score_arg + (size_t)rows * nch);
    m->score_lp = m->score_tgt + rows;
    m->score_targets = (uint32_t*)(m->score_lp + rows);
    m->score_greedy = m->score_targets + rows;
    if (packed) {
        OMX_HIP_CHECK(hipMalloc((void**)&m->score_dq, (size_t)panel * m->cfg.hidden_size * sizeof(bf16_t)));
        m->score_dq_on = true;
    }
    m->score_rows = rows;
    m->score_panel = panel;
    return 0;
}

}  // namespace
}  // namespace omx

extern "C" {

int omx_qwen3_score(omx_qwen3 m, const uint32_t* tokens, int n, const uint32_t* targets, float* logprobs, uint32_t* greedy) {
    OMX_REQUIRE(m, "omx_qwen3_score: null model");
    OMX_REQUIRE(m->allreduce == nullptr && m->cfg.tp_size <= 1 && m->cfg.ep_size <= 1,
                "omx_qwen3_score: tensor / expert parallel models are not supported (the vocabulary is sharded; single-rank models only)");
    OMX_REQUIRE(!(m->cfg.num_experts > 0 && m->cfg.moe_mode == 2), "omx_qwen3_score: moe_mode 2 (deepseek) models are not supported");
    OMX_REQUIRE(!m->f16, "omx_qwen3_score: float16 models (float16 weights or float16 triplets) are not supported; bf16 activations only");
    OMX_REQUIRE(n >= 1, "omx_qwen3_score: %d tokens (at least 1)", n);
    OMX_REQUIRE(tokens && targets && logprobs, "omx_qwen3_score: null argument");
    OMX_REQUIRE(n <= m->prompt_cap, "omx_qwen3_score: %d tokens exceed max_context %d", n, m->prompt_cap);
    const int V = m->V, hd = m->cfg.hidden_size;
    OMX_REQUIRE(V % 8 == 0 && V <= (1 << 20), "omx_qwen3_score: vocabulary %d must be a multiple of 8 and at most 2^20", V);
    for (int i = 0; i < n; ++i) {
        OMX_REQUIRE(tokens[i] < (uint32_t)V, "omx_qwen3_score: token id %u out of range (vocab %d)", tokens[i], V);
        OMX_REQUIRE(targets[i] < (uint32_t)V || targets[i] == OMX_NO_TARGET, "omx_qwen3_score: target id %u out of range (vocab %d)", targets[i], V);
    }
    // OMX_SCORE_PANEL=<multiple of 1024>: columns per vocabulary panel (read per call, as OMX_PREFILL_SERIAL)
    // (default: Qwen3-8B's head over 2 048 rows measured 2.37 ms at 4096, 2.02 at 8192, 1.98 at 16384, 1.95 at 32768 with twice the buffers: DESIGN 4.10)
    const int P_env = env_int("OMX_SCORE_PANEL", 16384);
    OMX_REQUIRE(P_env >= OMX_LOGPROB_CHUNK && P_env % OMX_LOGPROB_CHUNK == 0, "omx_qwen3_score: OMX_SCORE_PANEL=%d must be a positive multiple of %d",
                P_env, OMX_LOGPROB_CHUNK);
    const int P = std::min(P_env, (V + OMX_LOGPROB_CHUNK - 1) / OMX_LOGPROB_CHUNK * OMX_LOGPROB_CHUNK);
    StepState st;
    if (read_step_state(m, &st)) return 1;
    OMX_REQUIRE(st.pos + n + 1 <= m->cap, "omx_qwen3_score: %d cached + %d tokens exceed max_context %d", st.pos, n, m->cap);
    if (resolve_weights(m)) return 1;          // (score may be the first call on a fresh model)
    const bool packed = m->cfg.quant_bits != 0;
    hipStream_t s = m->stream;
    for (hipEvent_t& e : m->score_ev)
        if (!e) OMX_HIP_CHECK(hipEventCreate(&e));
    // allocations ahead of the timed region, as omx_qwen3_prefill makes them
    if (packed) dq_cache_prepare(m);
    if (prefill_reserve(m, n)) return 1;
    if (score_reserve(m, n, P, packed)) return 1;
    OMX_HIP_CHECK(hipMemcpyAsync(m->prompt_dev, tokens, (size_t)n * 4, hipMemcpyHostToDevice, s));
    OMX_HIP_CHECK(hipMemcpyAsync(m->score_targets, targets, (size_t)n * 4, hipMemcpyHostToDevice, s));
    OMX_HIP_CHECK(hipEventRecord(m->score_ev[0], s));
    if (prefill_prefix_batched(m, n, st.pos, nullptr, /*full_last=*/true, /*packed_rows_pass=*/false)) return 1;
    OMX_HIP_CHECK(hipEventRecord(m->score_ev[1], s));
    // [final RMSNorm rows] -> per panel [head rows dequantised] [GEMM] [chunk partials] -> [merge]   (model.rs:423, 480-490)
    if (omx_rms_norm(m->pf_xn, m->pf_h, m->final_norm, n, hd, m->cfg.rms_norm_eps, OMX_BFLOAT16, s)) return 1;
    for (int p0 = 0; p0 < V; p0 += P) {
        const int Pn = std::min(P, V - p0);
        const bf16_t* w = nullptr;
        if (packed) {   // the panel's rows of the head's triplet (or of the tied table's), in the head's own format
            const QMat& q = m->q_head;
            const size_t wpr = (size_t)hd * q.bits / 32, gpr = (size_t)hd / q.group;
            if (launch_dequantize_bf16(m->score_dq, q.w + p0 * wpr, q.scales + p0 * gpr, q.biases ? q.biases + p0 * gpr : nullptr, Pn, hd,
                                       q.group, q.bits, false, s))
                return 1;
            w = m->score_dq;
        } else {
            w = m->lm_head + (size_t)p0 * hd;
        }
        if (launch_gemm_bf16(m->score_panel_buf, m->pf_xn, w, nullptr, n, Pn, hd, s)) return 1;
        if (omx_logprob_partial(m->score_part, m->score_arg, m->score_tgt, m->score_panel_buf, Pn, p0, Pn, m->score_targets, n, V,
                                OMX_BFLOAT16, (omx_stream)s))
            return 1;
    }
    if (omx_logprob_merge(m->score_lp, m->score_greedy, nullptr, m->score_part, m->score_arg, m->score_tgt, m->score_targets, n, V, (omx_stream)s))
        return 1;
    OMX_HIP_CHECK(hipEventRecord(m->score_ev[2], s));
    std::vector<uint32_t> g((size_t)n);
    OMX_HIP_CHECK(hipMemcpyAsync(logprobs, m->score_lp, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    OMX_HIP_CHECK(hipMemcpyAsync(g.data(), m->score_greedy, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    OMX_HIP_CHECK(hipStreamSynchronize(s));
    OMX_HIP_CHECK(hipEventElapsedTime(&m->last_score_pass_ms, m->score_ev[0], m->score_ev[1]));
    OMX_HIP_CHECK(hipEventElapsedTime(&m->last_score_head_ms, m->score_ev[1], m->score_ev[2]));
    if (greedy) memcpy(greedy, g.data(), (size_t)n * 4);
    st.pos += n;
    st.cur_token = g[(size_t)n - 1];
    if (write_step_state(m, st)) return 1;
    OMX_HIP_CHECK(hipStreamSynchronize(s));
    return 0;
}

int omx_qwen3_last_score_ms(omx_qwen3 m, float* pass_ms, float* head_ms) {
    OMX_REQUIRE(m && pass_ms && head_ms, "omx_qwen3_last_score_ms: null argument");
    *pass_ms = m->last_score_pass_ms;
    *head_ms = m->last_score_head_ms;
    return 0;
}

}  // extern "C"
