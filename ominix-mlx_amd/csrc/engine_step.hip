// The decode step of the Qwen3 engine (engine.hip): its small kernels, the dense / packed / hybrid launch sequences and their shared
// end, the sampler's launches, the captured forms (hipGraph, AQL program) and the fallback when a launch gave up waiting.
#include "engine_model.hpp"

namespace omx {
namespace {

// dequantise ONE embedding row (QuantizedEmbedding::forward, mlx-rs/src/nn/quantized.rs:192-203) chosen by the step state
// the step's first kernel also refreshes what the rest of the step reads instead of chasing the position: the step sequence
// number (granule tags of attn_step.hip) and the RoPE row of the current position, rope_cur = cos[pos, :] | sin[pos, :]
__device__ __forceinline__ void step_begin(const StepState* st, unsigned* seq, float* rope_cur, const float* rope_cos,
                                           const float* rope_sin, int half) {
    if (blockIdx.x != 0) return;
    if (seq && threadIdx.x == 0) *seq += 1u;
    if (rope_cur && (int)threadIdx.x < 2 * half) {
        const int t = threadIdx.x, pos = st->pos;
        rope_cur[t] = t < half ? rope_cos[(size_t)pos * half + t] : rope_sin[(size_t)pos * half + t - half];
    }
}

template <int BITS>
__global__ __launch_bounds__(256) void qembed_kernel(bf16_t* __restrict__ h, const uint32_t* __restrict__ w,
                                                     const bf16_t* __restrict__ scales, const bf16_t* __restrict__ biases,
                                                     const StepState* st, int hidden, int group, unsigned* seq, float* rope_cur,
                                                     const float* rope_cos, const float* rope_sin, int half, bool scales_f16) {
    constexpr int EPW = 32 / BITS;
    step_begin(st, seq, rope_cur, rope_cos, rope_sin, half);
    const size_t row = st->cur_token;
    const int words = hidden / EPW;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < words; i += gridDim.x * blockDim.x) {
        const uint32_t wd = w[row * words + i];
        const int g = i * EPW / group;
        const bf16_t sb16 = scales[row * (hidden / group) + g], bb16 = biases ? biases[row * (hidden / group) + g] : (bf16_t)0;
        const float sc = scales_f16 ? __half2float(__ushort_as_half(sb16)) : bf16_to_f32(sb16);
        const float bi = scales_f16 ? __half2float(__ushort_as_half(bb16)) : bf16_to_f32(bb16);
#pragma unroll
        for (int e = 0; e < EPW; ++e) {   // (dequantise: the result has the scales' dtype, quantized.rs:192-203)
            const float v = (float)((wd >> (e * BITS)) & ((1u << BITS) - 1u)) * sc + bi;
            h[i * EPW + e] = scales_f16 ? Act16<true>::bits(v) : f32_to_bf16(v);
        }
    }
}

// ... 2 / 3 / 5 / 6 bits: one thread per run of 32 elements (BITS words, quant_chunked in quant.hpp), the same element expression
template <int BITS>
__global__ __launch_bounds__(256) void qembed_chunk_kernel(bf16_t* __restrict__ h, const uint32_t* __restrict__ w,
                                                           const bf16_t* __restrict__ scales, const bf16_t* __restrict__ biases,
                                                           const StepState* st, int hidden, int group, unsigned* seq, float* rope_cur,
                                                           const float* rope_cos, const float* rope_sin, int half, bool scales_f16) {
    step_begin(st, seq, rope_cur, rope_cos, rope_sin, half);
    const size_t row = st->cur_token;
    const int chunks = hidden / 32;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < chunks; i += gridDim.x * blockDim.x) {
        uint32_t wd[BITS];
#pragma unroll
        for (int k = 0; k < BITS; ++k) wd[k] = w[(row * chunks + i) * BITS + k];
        const int g = i * 32 / group;
        const bf16_t sb16 = scales[row * (hidden / group) + g], bb16 = biases ? biases[row * (hidden / group) + g] : (bf16_t)0;
        const float sc = scales_f16 ? __half2float(__ushort_as_half(sb16)) : bf16_to_f32(sb16);
        const float bi = scales_f16 ? __half2float(__ushort_as_half(bb16)) : bf16_to_f32(bb16);
#pragma unroll
        for (int e = 0; e < 32; ++e) {
            const float v = (float)qfield<BITS>(wd, e) * sc + bi;
            h[i * 32 + e] = scales_f16 ? Act16<true>::bits(v) : f32_to_bf16(v);
        }
    }
}

// h = bf16(resid + bf16(all-reduced partial)): the residual of a block whose output arrives as an f32 sum over the ranks, in the step
// and in the expert-parallel batched prompt pass (the residual of mixtral model.rs:343-344)
// (f16: a float16 model -- the same two roundings in float16)
__global__ void ep_fold_kernel(bf16_t* __restrict__ out, const bf16_t* __restrict__ resid, const float* __restrict__ partial, int64_t n, bool f16 = false) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        if (f16) out[i] = Act16<true>::bits(Act16<true>::val(resid[i]) + Act16<true>::rnd(partial[i]));
        else out[i] = f32_to_bf16(bf16_to_f32(resid[i]) + round_bf16(partial[i]));
    }
}

__global__ void feed_prompt_kernel(StepState* st, const uint32_t* prompt) {
    // after a no-head prefill step: advance and feed the next prompt token
    st->pos += 1;
    st->prompt_idx += 1;
    st->cur_token = prompt[st->prompt_idx];
}

__global__ __launch_bounds__(256) void sample_finalize_kernel(StepState* st, const unsigned long long* partials,
                                                               int n_partials, uint32_t* out_ring, int ring_cap,
                                                               unsigned long long* key_out) {
    __shared__ unsigned long long red[4];
    unsigned long long best = 0;
    // a batch of a thread's keys is in flight before the first compare (one load + wait per iteration was 19 dependent round trips at
    // Qwen3's 4748 partials, in a one-block launch the whole chip waits for); past the end the last key is read again: a maximum
    constexpr int kInFlight = 20;   // (20 x 256 >= 4748: one round)
    for (int i0 = threadIdx.x; i0 < n_partials; i0 += 256 * kInFlight) {
        unsigned long long k[kInFlight];
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) k[u] = partials[min(i0 + u * 256, n_partials - 1)];
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) best = k[u] > best ? k[u] : best;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(best, o, 64);
        best = other > best ? other : best;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) best = red[w] > best ? red[w] : best;
        if (key_out) {
            *key_out = best;   // TP: all-reduced (max) across ranks before apply_token_kernel
        } else {
            const uint32_t tok = ~(uint32_t)(best & 0xFFFFFFFFull);
            out_ring[st->out_count % ring_cap] = tok;
            st->out_count += 1;
            st->cur_token = tok;
            st->pos += 1;
        }
    }
}

__global__ void apply_token_kernel(StepState* st, const unsigned long long* key, uint32_t* out_ring, int ring_cap) {
    const uint32_t tok = ~(uint32_t)(*key & 0xFFFFFFFFull);
    out_ring[st->out_count % ring_cap] = tok;
    st->out_count += 1;
    st->cur_token = tok;
    st->pos += 1;
}

__global__ __launch_bounds__(256) void embed_kernel(bf16_t* __restrict__ h, const bf16_t* __restrict__ table,
                                                    const StepState* st, int hidden, unsigned* seq, float* rope_cur,
                                                    const float* rope_cos, const float* rope_sin, int half) {
    step_begin(st, seq, rope_cur, rope_cos, rope_sin, half);
    const u32x4* src = reinterpret_cast<const u32x4*>(table + (size_t)st->cur_token * hidden);
    u32x4* dst = reinterpret_cast<u32x4*>(h);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < hidden / 8; i += gridDim.x * blockDim.x) dst[i] = src[i];
}

}  // namespace

int launch_ep_fold(int grid, bf16_t* out, const bf16_t* resid, const float* partial, int64_t n, bool f16, hipStream_t s) {
    ep_fold_kernel<<<grid, 256, 0, s>>>(out, resid, partial, n, f16);
    OMX_LAUNCH_CHECK();
    return 0;
}

// the captured forms of the step (hipGraph executables, the AQL program) hold the split plan and every pointer: dropped together
void drop_graphs(omx_qwen3 m) {
    if (m->g_full) { (void)hipGraphExecDestroy(m->g_full); m->g_full = nullptr; }
    if (m->g_nohead) { (void)hipGraphExecDestroy(m->g_nohead); m->g_nohead = nullptr; }
    if (m->aql_full) { aql_destroy(m->aql_full); m->aql_full = nullptr; }
    if (m->cfg.num_experts > 0 && (m->cfg.ep_size > 1 || m->cfg.tp_size > 1) && m->stream) workspace_aux_pin(m->stream, false);
}

// ... and the next step captures them again (a launch argument of the captured step changed)
void recapture_step(omx_qwen3 m) {
    drop_graphs(m);
    m->eager = false;
}

// all-reduce `n` elements of `buf` in place over the ranks, on the engine's stream
int rank_allreduce(omx_qwen3 m, void* buf, size_t n, int dtype, int op) {
    OMX_REQUIRE(m->allreduce != nullptr, "more than one rank (tp_size / ep_size) but no communicator set (omx_qwen3_set_comm)");
    OMX_REQUIRE(m->allreduce(buf, buf, n, dtype, op, m->comm, m->stream) == 0, "ncclAllReduce failed");
    return 0;
}

int allreduce_sum(omx_qwen3 m, float* buf, size_t n) { return rank_allreduce(m, buf, n, kNcclFloat32, kNcclSum); }

// the step state on the host: read (waits for the stream) / written back (asynchronous: a caller that needs it landed synchronises)
int read_step_state(omx_qwen3 m, StepState* st) {
    OMX_HIP_CHECK(hipMemcpyAsync(st, m->st, sizeof(*st), hipMemcpyDeviceToHost, m->stream));
    OMX_HIP_CHECK(hipStreamSynchronize(m->stream));
    return 0;
}

int write_step_state(omx_qwen3 m, const StepState& st) {
    OMX_HIP_CHECK(hipMemcpyAsync(m->st, &st, sizeof(st), hipMemcpyHostToDevice, m->stream));
    return 0;
}

// the sampler's history starts from zero: the tokens the penalties have seen, the selection's histograms
int reset_sampler_history(omx_qwen3 m) {
    if (m->seen) OMX_HIP_CHECK(hipMemsetAsync(m->seen, 0, (size_t)m->V, m->stream));
    if (m->sel) OMX_HIP_CHECK(hipMemsetAsync(m->sel, 0, sample_select_ws_bytes(), m->stream));
    return 0;
}

// a penalty reads the history of sampled tokens
bool sampling_penalised(const omx_sampling& p) { return p.repetition_penalty != 1.f || p.presence_penalty != 0.f; }

// filtered sampling: [key] [select: a launch per level of the descent, histograms in m->sel] [noise over the kept set -> the partials]; temperature 0 with a
// penalty is the argmax of the penalised logits (the noise launch without noise).  Single rank (omx_qwen3_set_sampling refuses TP).
static int add_filtered_sampling(omx_qwen3 m, hipStream_t s) {
    const omx_sampling& p = m->sampling;
    const bool greedy = p.temperature == 0.f;
    const uint8_t* seen = sampling_penalised(p) ? m->seen : nullptr;
    if (!greedy && launch_rng_next(m->rng, s)) return 1;
    if (launch_sample_select(m->sel, m->logits, m->f16, m->V, p, seen, s)) return 1;
    return launch_sample_filtered_noise(m->argmax_partials, m->n_argmax_partials, m->logits, m->f16, m->V, p, seen, m->sel, m->rng + 2, s);
}

// after the finalize: the sampled token joins the history the penalties read
static int mark_sampled_token(omx_qwen3 m, hipStream_t s) {
    if (!m->filter_on || !sampling_penalised(m->sampling)) return 0;
    return launch_mark_seen(m->seen, m->V, m->st, s);
}

// after that: the log-probability of the token the finalize just wrote (and the row's alternatives) over the step's raw logits, into the
// rings' entry of that token (omx_qwen3_set_logprobs).  Every argument is fixed: the target is the step state's word, the entry is
// derived on the device from its count.
static int add_step_logprobs(omx_qwen3 m, hipStream_t s) {
    if (m->lp_top < 0) return 0;
    LogprobTopOut o = {};
    o.logprobs = m->lp_ring; o.top_ids = m->top_id_ring; o.top_lp = m->top_lp_ring;
    o.ring_count = &m->st->out_count; o.ring_cap = m->ring_cap;
    return launch_logprob_top(o, m->lp_scratch, m->logits, m->V, &m->st->cur_token, 1, m->V, m->lp_top, s);
}

// temperature sampling: replace the greedy per-block partials by those of logits / T + Gumbel noise, the noise
// of vocabulary row v being word v of a V-word draw from the step's key (random.hip).  The greedy partials the
// lm_head epilogue wrote are simply overwritten; sample_finalize_kernel / the TP max all-reduce are unchanged.
static int add_sampling_noise(omx_qwen3 m, hipStream_t s) {
    if (m->filter_on) return add_filtered_sampling(m, s);
    if (m->temperature == 0.f) return 0;
    const EngineConfig& c = m->cfg;
    const int tp = c.tp_size > 1 ? c.tp_size : 1;
    if (launch_rng_next(m->rng, s)) return 1;
    return launch_sample_noise(m->argmax_partials, m->n_argmax_partials, m->logits, m->rng + 2, m->V, c.tp_rank * m->V,
                               m->V * tp, 1.0f / m->temperature, m->f16, s);
}

// O projection inside the attention launch of layer `layer` (csrc/attn_step.hip): bf16 weights -- or a packed checkpoint's layer whose OWN
// O matrix is 4-bit --, single rank, a shape the kernel has a register layout for; OMX_ATTN_OPROJ=0 keeps the two launches
bool attention_takes_oproj(omx_qwen3 m, int layer) {
    const bool off = env_off("OMX_ATTN_OPROJ");        // (read per call: tests flip it between engines of one process)
    const EngineConfig& c = m->cfg;
    // (tensor parallel: the rank's heads and columns -- the launch then leaves the f32 partial for the all-reduce)
    // every block of that launch waits on others: all Hkv * nsplit of them must be resident, one per CU
    if (off || m->oproj_disabled || m->Hkv * m->attn_nsplit > m->cus) return false;
    if (c.quant_bits) {
        // the packed O matrix in ITS format, with its interleaved scale | bias words (built at load for K % 2048 == 0)
        if (c.ep_size > 1 || c.tp_size > 1 || c.quant_scales_f16 || layer < 0 || layer >= (int)m->qlayers.size()) return false;
        const QMat& o = m->qlayers[layer].o;
        return o.bits == 4 && o.sb != nullptr && attn_step_oproj_q4_ok(m->H, m->Hkv, c.head_dim, m->attn_nsplit, c.hidden_size, o.group);
    }
    // (a dense float16 model: the O projection stays its own launch -- the attention launch's O phase is bf16-only; every layer alike)
    return !m->f16 && attn_step_oproj_ok(m->H, m->Hkv, c.head_dim, m->attn_nsplit, c.hidden_size);
}

// ... of ANY layer: what the fallback ladder and the step-forms hook ask (a mixed-precision checkpoint's layers may differ)
bool any_layer_takes_oproj(omx_qwen3 m) {
    for (int l = 0; l < m->cfg.num_hidden_layers; ++l)
        if (attention_takes_oproj(m, l)) return true;
    return false;
}

// what the folds of the dense step share: dense bf16 weights, a single rank without a communicator, no experts, the launch-per-op form
static bool dense_bf16_single_rank_per_op(omx_qwen3 m) {
    const EngineConfig& c = m->cfg;
    if (c.quant_bits != 0 || m->f16 || c.num_experts > 0 || c.tp_size > 1 || c.ep_size > 1 || m->allreduce != nullptr) return false;
    return step_engine_mode(m) == 0;
}

// a layer's stacked q | k | v matrices as the kernels that stream them take them
static StackedRows qkv_rows(omx_qwen3 m, int layer) {
    const LayerW& L = m->layers[layer];
    const int D = m->cfg.head_dim;
    return StackedRows{L.q, L.k, L.v, m->H * D, m->Hkv * D, (m->H + 2 * m->Hkv) * D};
}

// down + residual of a layer and [RMSNorm + q/k/v] of the next one as ONE launch (csrc/gemv_chain.hip): the dense bf16 step of a single rank
// on its launch-per-op form, no rows-per-wave override of the two GEMVs it stands for, a shape the kernel has a register layout for and a
// grid that is resident as a whole (every workgroup of that launch waits on all others); OMX_DOWN_QKV=0 keeps the two launches
bool down_takes_qkv(omx_qwen3 m) {
    const bool off = env_off("OMX_DOWN_QKV");          // (read per call: tests flip it between engines of one process)
    const EngineConfig& c = m->cfg;
    if (off || m->chain_disabled || !dense_bf16_single_rank_per_op(m)) return false;
    if (env_int("OMX_GEMV_RPW_QKV", 0) != 0 || env_int("OMX_GEMV_RPW_DOWN", 0) != 0) return false;
    if (!m->chain_gran || !gemv_chain_ok(c.hidden_size, m->I, (m->H + 2 * m->Hkv) * c.head_dim)) return false;
    return gemv_chain_grid(c.hidden_size) <= kGemvChainBlocksPerCU * m->cus;
}

// [RMSNorm + gate/up + SwiGLU] of layer `layer` inside its attention + O launch (csrc/attn_step.hip, gateup_phase): the dense bf16 step of a
// single rank on its launch-per-op form with the O projection in the attention launch, no rows-per-wave override of the two GEMVs the
// phase stands for, the one shape the kernel shares out evenly (hidden 4096, intermediate 12288, 32 / 8 heads of 128: every split
// plan of these heads has 256 blocks) and that grid resident as a whole.  A q/k/v bias (Qwen2 wiring) does not touch gate/up and is allowed; OMX_ATTN_GATEUP=0 keeps the two launches
bool attention_takes_gateup(omx_qwen3 m, int layer) {
    const bool off = env_off("OMX_ATTN_GATEUP");       // (read per call: tests flip it between engines of one process)
    const EngineConfig& c = m->cfg;
    if (off || m->gateup_disabled || !dense_bf16_single_rank_per_op(m)) return false;
    if (env_int("OMX_GEMV_RPW_O", 0) != 0 || env_int("OMX_GEMV_RPW_GU", 0) != 0) return false;
    if (!m->gateup_gran || m->cus < 256 || !attention_takes_oproj(m, layer)) return false;
    return attn_step_gateup_ok(m->H, m->Hkv, c.head_dim, m->attn_nsplit, c.hidden_size, m->I);
}

// [down + residual] of layer `layer` and [RMSNorm + q/k/v] of layer + 1 inside that launch as well (csrc/attn_step.hip, down_qkv_phase): layers
// 0 .. L-2 are ONE launch each.  Both folds it joins must be on -- it inherits their gates: dense bf16, single rank, the launch-per-op form,
// no rows-per-wave override, the 4096 / 12288 / 32 / 8 / 128 shape on 256 resident blocks, a q/k/v bias allowed -- and a give-up that
// switches either off switches this off with it; OMX_ATTN_DOWN=0 keeps the two launches per layer
bool attention_takes_down(omx_qwen3 m, int layer) {
    const bool off = env_off("OMX_ATTN_DOWN");         // (read per call: tests flip it between engines of one process)
    const EngineConfig& c = m->cfg;
    if (off || !m->act_gran || layer + 1 >= c.num_hidden_layers || !attention_takes_gateup(m, layer) || !down_takes_qkv(m)) return false;
    return attn_step_down_ok(c.hidden_size, m->I, (m->H + 2 * m->Hkv) * c.head_dim);
}

// OMX_PEER_FUSED: a GEMV whose blocks poll their peers' stores must be resident as a whole -- a block waiting for a peer's row while
// that peer's matching block waits for a free CU behind OUR unscheduled blocks never finishes (it gives up after 2^23 polls and voids
// the step).  The streaming kernels hold at least two 4-wave blocks per CU (<= 256 VGPRs, a few KB of LDS); beyond that the standalone
// all-reduce launch follows the GEMV as usual.
static bool peer_fused_fits(omx_qwen3 m, int N, int K) {
    return m->peer_dev != nullptr && gemv_grid(N, K, EPI_F32, 0) <= 2 * m->cus;
}

// the attention launch of layer l of a decode step (both the bf16 and the packed-weight step use the bf16 KV kernels);
// resid / out != null: the layer's O projection + residual rides in the same launch (attention_takes_oproj); gateup: and its
// [RMSNorm + gate/up + SwiGLU] behind that (attention_takes_gateup)
// down: and the layer's [down + residual] (into `resid`'s buffer: the ping-pong partner of the row the O projection leaves) + the next
// layer's [RMSNorm + q/k/v] behind that (attention_takes_down)
static int enqueue_attention(omx_qwen3 m, int l, hipStream_t s, const bf16_t* resid = nullptr, bf16_t* out = nullptr, float* out_f32 = nullptr,
                             bool gateup = false, bool down = false) {
    const EngineConfig& c = m->cfg;
    const int D = c.head_dim;
    const LayerW& L = m->layers[l];
    AttnStepArgs a = {};
    a.qkv = m->qkv;
    a.k = m->kcache[l]; a.v = m->vcache[l];
    a.kv_head_stride = (int64_t)m->cap * D;
    a.H = m->H; a.Hkv = m->Hkv; a.cap = m->cap;
    a.scale = 1.0f / sqrtf((float)D);
    a.eps = c.rms_norm_eps;
    a.q_norm_w = L.q_norm; a.k_norm_w = L.k_norm;
    a.rope_cur = m->rope_cur;
    a.pos_ptr = &m->st->pos;
    a.seq_ptr = m->step_seq;
    a.tag_mul = (unsigned)c.num_hidden_layers; a.tag_add = (unsigned)l + 1u;
    a.chunk = m->attn_chunk; a.nsplit = m->attn_nsplit;
    a.ws = m->attn_gran;
    a.out = m->attn_out;
    a.abort_flag = m->wait_abort;
    a.trace = m->attn_trace ? m->attn_trace + (size_t)l * m->attn_nsplit * m->Hkv * kAttnTraceWords : nullptr;
    a.f16 = m->f16;   // a float16 checkpoint runs in float16 end to end
    if (resid && (out || out_f32)) {
        a.o_resid = resid; a.o_out = out; a.o_out_f32 = out_f32; a.o_rows = c.hidden_size; a.xg = m->attn_xg;
        if (c.quant_bits) {
            const QMat& o = m->qlayers[l].o;
            a.o_wq = o.w; a.o_sb = o.sb; a.o_group = o.group;
        } else {
            a.o_w = L.o;
        }
    }
    if (gateup) {
        a.gu_gate = L.gate; a.gu_up = L.up; a.gu_norm_w = L.post_ln; a.gu_out = m->act; a.gu_rows = m->I;
        a.hg = m->gateup_gran;
    }
    if (down) {
        const LayerW& Ln = m->layers[l + 1];
        a.dn_w = L.down; a.dn_out = const_cast<bf16_t*>(resid);   // every O row has consumed its residual before the first down row exists
        a.ag = m->act_gran; a.rg = m->chain_gran;
        a.nq = qkv_rows(m, l + 1);
        a.nq_norm_w = Ln.in_ln; a.nq_bias = Ln.qkv_bias; a.nq_out = m->qkv;
    }
    return launch_attn_step(a, D, s);
}

// The end of a step on the hidden row `h` (plus the pending f32 partial(s) the dense step has not folded into it yet) -- the residual
// stream of a decode step, or the last row of a batched prompt (model.rs:423, 480-489, 733-735):
// [final RMSNorm + lm_head GEMV + argmax partials] [sampler noise / filter] [finalize], then on one rank the sampled token joins the
// penalties' history and, where asked for, its log-probability is taken from the row; tp: a rank holds a vocabulary shard -- its rows are numbered from its offset and the ranks' packed (logit, index)
// keys meet in one unsigned max.  with_head = false (a prompt token whose logits nobody reads): advance to the next prompt token.
// Every launch is a recording site: the AQL replay refuses a step with a launch that is none.
int enqueue_step_tail(omx_qwen3 m, bool with_head, const bf16_t* h, const float* pending, int pending_n, bool tp) {
    const EngineConfig& c = m->cfg;
    hipStream_t s = m->stream;
    if (!with_head) {
        OMX_LAUNCH(feed_prompt_kernel, 1, 1, 0, s, m->st, m->prompt_dev);
        OMX_LAUNCH_CHECK();
        return 0;
    }
    if (c.quant_bits) {
        QGemvArgs a = {};
        a.m[0] = m->q_head; a.m[0].n = m->V; a.N = m->V; a.K = c.hidden_size; a.group = m->q_head.group;   // the head's own format
        a.x = h; a.norm_w = m->final_norm; a.eps = c.rms_norm_eps; a.out = m->logits; a.scales_f16 = c.quant_scales_f16 != 0;
        a.argmax_slot = m->argmax_partials;
        a.row_offset = c.tp_rank * m->V;                 // this rank's vocabulary shard
        if (launch_qgemv(a, m->q_head.bits, PRO_RMSNORM, EPI_ARGMAX, s)) return 1;
    } else {
        GemvArgs a = {};
        a.w0 = m->lm_head; a.n0 = m->V; a.N = m->V; a.K = c.hidden_size;
        a.x = h; a.x_partial = pending; a.x_partial_n = pending_n;
        a.norm_w = m->final_norm; a.eps = c.rms_norm_eps;
        a.out = m->logits;
        a.argmax_slot = m->argmax_partials;
        a.row_offset = c.tp_rank * m->V;
        a.f16 = m->f16;
        if (launch_gemv(a, PRO_RMSNORM, EPI_ARGMAX, s)) return 1;
    }
    if (add_sampling_noise(m, s)) return 1;
    OMX_LAUNCH(sample_finalize_kernel, 1, 256, 0, s, m->st, m->argmax_partials, m->n_argmax_partials, m->out_ring,
               m->ring_cap, tp ? m->argmax_key : nullptr);
    OMX_LAUNCH_CHECK();
    if (!tp) return mark_sampled_token(m, s) || add_step_logprobs(m, s);
    if (rank_allreduce(m, m->argmax_key, 1, kNcclUint64, kNcclMax)) return 1;
    OMX_LAUNCH(apply_token_kernel, 1, 1, 0, s, m->st, m->argmax_key, m->out_ring, m->ring_cap);
    OMX_LAUNCH_CHECK();
    return 0;
}

// the same step on a quantized checkpoint: packed-weight GEMVs (quant.hip) with the prologues / epilogues of the bf16 step
static int enqueue_step_quant(omx_qwen3 m, bool with_head) {
    const EngineConfig& c = m->cfg;
    hipStream_t s = m->stream;
    const int hd = c.hidden_size, D = c.head_dim;
    const bool sf16 = c.quant_scales_f16 != 0;
    // every launch takes its format from its members (QMat::bits / group, written by resolve_weights): a checkpoint's matrices may differ
    // 4 / 8 bits: whole fields per word; 2 / 3 / 5 / 6: runs of 32 elements (quant_chunked)
#define OMX_QEMBED(KERNEL, B)                                                                                                      \
    case B: OMX_LAUNCH(KERNEL<B>, 4, 256, 0, s, m->h, m->q_embed.w, m->q_embed.scales, m->q_embed.biases, m->st, hd, m->q_embed.group, m->step_seq, \
                       m->rope_cur, m->rope_cos, m->rope_sin, D / 2, sf16); break;
    switch (m->q_embed.bits) {
        OMX_QEMBED(qembed_chunk_kernel, 2) OMX_QEMBED(qembed_chunk_kernel, 3) OMX_QEMBED(qembed_kernel, 4)
        OMX_QEMBED(qembed_chunk_kernel, 5) OMX_QEMBED(qembed_chunk_kernel, 6) OMX_QEMBED(qembed_kernel, 8)
    }
#undef OMX_QEMBED
    OMX_LAUNCH_CHECK();
    bf16_t* h = m->h;
    bf16_t* hn = m->h2;
    // tensor parallel (round 4): q / k / v / gate / up / lm_head are this rank's packed rows, o / down its K slices (whole groups) --
    // their unrounded f32 row sums are all-reduced and folded into the residual by a launch of their own (the bf16 step folds them in
    // the next GEMV's prologue: the packed kernels' prologues are left alone)
    const bool tp = c.ep_size <= 1 && (c.tp_size > 1 || m->allreduce != nullptr);
    auto reduce_fold = [&](float* partial) -> int {
        if (allreduce_sum(m, partial, hd)) return 1;
        ep_fold_kernel<<<8, 256, 0, s>>>(hn, h, partial, (int64_t)hd, sf16);
        OMX_LAUNCH_CHECK();
        std::swap(h, hn);
        return 0;
    };
    for (int l = 0; l < c.num_hidden_layers; ++l) {
        const LayerW& L = m->layers[l];
        const LayerQ& Q = m->qlayers[l];
        {   // [RMSNorm + QKV]
            QGemvArgs a = {};
            a.m[0] = Q.q; a.m[1] = Q.k; a.m[2] = Q.v;
            a.N = (m->H + 2 * m->Hkv) * D; a.K = hd; a.group = Q.q.group;
            a.x = h; a.norm_w = L.in_ln; a.eps = c.rms_norm_eps; a.out = m->qkv; a.scales_f16 = sf16;
            if (launch_qgemv(a, Q.q.bits, PRO_RMSNORM, EPI_STORE, s)) return 1;
        }
        const bool fused_o = !tp && attention_takes_oproj(m, l);
        // [q/k RMSNorm + RoPE + cache append + split-KV SDPA + merge]: the bf16 kernel (+ [O + residual] on the packed matrix)
        if (enqueue_attention(m, l, s, fused_o ? h : nullptr, fused_o ? hn : nullptr)) return 1;
        if (fused_o) {
            std::swap(h, hn);
        } else if (tp) {   // [O partial] [all-reduce] [+ residual]
            QGemvArgs a = {};
            a.m[0] = Q.o; a.N = hd; a.K = m->H * D; a.group = Q.o.group;
            a.x = m->attn_out; a.out_f32 = m->partial_a; a.scales_f16 = sf16;
            if (launch_qgemv(a, Q.o.bits, PRO_NONE, EPI_F32, s) || reduce_fold(m->partial_a)) return 1;
        } else {   // [O + residual]
            QGemvArgs a = {};
            a.m[0] = Q.o; a.N = hd; a.K = m->H * D; a.group = Q.o.group;
            a.x = m->attn_out; a.resid = h; a.out = hn; a.scales_f16 = sf16;
            if (launch_qgemv(a, Q.o.bits, PRO_NONE, EPI_RESIDUAL, s)) return 1;
            std::swap(h, hn);
        }
        if (c.num_experts > 0 && c.tp_size > 1) {
            // expert tensor parallel on packed stacks (round 5): [replicated packed router + this rank's columns of the routed experts]
            // [all-reduce of the slots' f32 partials] [weighted sum + residual with the single-device roundings]
            if (omx_moe_block_partial_tp_q(m->moe_y, m->moe_inds, m->moe_scores, h, L.post_ln, c.rms_norm_eps, OMX_QMOE_ARGS(Q), 1, hd, m->moe_I, c.num_experts, c.num_experts_per_tok, c.moe_mode,
                                           c.norm_topk_prob, c.quant_group, c.quant_bits, sf16 ? 1 : 0, s))
                return 1;
            if (allreduce_sum(m, m->moe_y, (size_t)c.num_experts_per_tok * hd)) return 1;
            if (omx_moe_combine_slots_ex(hn, m->moe_y, m->moe_scores, h, 1, hd, c.num_experts_per_tok, sf16 ? 1 : 0, s)) return 1;
            std::swap(h, hn);
            continue;
        }
        if (c.num_experts > 0 && c.ep_size > 1) {
            // expert parallel on packed stacks (round 5): this rank's experts only, the f32 partial all-reduced and folded into the residual
            const int el = c.num_experts / c.ep_size;
            if (omx_moe_block_partial_ep_q(m->partial_b, h, L.post_ln, c.rms_norm_eps, m->moe_xn, OMX_QMOE_ARGS(Q), 1, hd, c.moe_intermediate_size, c.num_experts,
                                           c.num_experts_per_tok, c.moe_mode, c.norm_topk_prob, c.ep_rank * el, el, c.quant_group, c.quant_bits, sf16 ? 1 : 0, s))
                return 1;
            if (reduce_fold(m->partial_b)) return 1;
            continue;
        }
        if (c.num_experts > 0) {   // [RMSNorm + router] [selection] [RMSNorm + expert gate/up + SwiGLU] [expert down] [sum + residual]
            if (omx_moe_block_forward_q_ex(hn, h, h, L.post_ln, c.rms_norm_eps, m->moe_xn, OMX_QMOE_ARGS(Q), 1, hd, c.moe_intermediate_size,
                                           c.num_experts, c.num_experts_per_tok, c.moe_mode, c.norm_topk_prob, c.quant_group, c.quant_bits, sf16 ? 1 : 0, s))
                return 1;
            std::swap(h, hn);
            continue;
        }
        {   // [RMSNorm + gate/up + SwiGLU]
            QGemvArgs a = {};
            a.m[0] = Q.gate; a.m[1] = Q.up; a.N = m->I; a.K = hd; a.group = Q.gate.group;
            a.x = h; a.norm_w = L.post_ln; a.eps = c.rms_norm_eps; a.out = m->act; a.scales_f16 = sf16;
            if (launch_qgemv(a, Q.gate.bits, PRO_RMSNORM, EPI_SWIGLU, s)) return 1;
        }
        if (tp) {   // [down partial] [all-reduce] [+ residual]
            QGemvArgs a = {};
            a.m[0] = Q.down; a.N = hd; a.K = m->I; a.group = Q.down.group;
            a.x = m->act; a.out_f32 = m->partial_b; a.scales_f16 = sf16;
            if (launch_qgemv(a, Q.down.bits, PRO_NONE, EPI_F32, s) || reduce_fold(m->partial_b)) return 1;
        } else {   // [down + residual]
            QGemvArgs a = {};
            a.m[0] = Q.down; a.N = hd; a.K = m->I; a.group = Q.down.group;
            a.x = m->act; a.resid = h; a.out = hn; a.scales_f16 = sf16;
            if (launch_qgemv(a, Q.down.bits, PRO_NONE, EPI_RESIDUAL, s)) return 1;
            std::swap(h, hn);
        }
    }
    return enqueue_step_tail(m, with_head, h, nullptr, 1, tp);
}

// The layers of the step as ONE persistent launch (csrc/step_engine.hip): dense bf16 model on a single rank, a shape the engine's
// consumers reproduce bit for bit, every CU of the device free for one resident workgroup.  OMX_STEP_ENGINE=0 keeps one launch per op.
// OMX_STEP_ENGINE=2: the hybrid step -- attention + o stay their own launch (attn_step.hip: a chain of three all-to-all hand-offs that a
// launch boundary serves as well as granules do), everything between two attention launches ([gate/up] [down] [next layer's q/k/v]) is one
// segment of the engine: two launches per layer instead of four, the weight stream of three ops crossing its two edges without a stop.
int step_engine_mode(omx_qwen3 m) {
    const int mode = env_int("OMX_STEP_ENGINE", 0);    // (read per call: tests flip it between engines of one process)
    const EngineConfig& c = m->cfg;
    const bool ok = mode > 0 && !m->se_disabled && !m->filter_on && m->lp_top < 0 && c.quant_bits == 0 && !m->f16 && c.num_experts == 0 && c.tp_size == 1 && c.ep_size <= 1 && m->allreduce == nullptr &&
           !c.attention_bias && m->se_gran != nullptr && m->cus > 0 &&
           step_engine_ok(c.hidden_size, m->H, m->Hkv, c.head_dim, m->I, m->attn_nsplit, m->cus);
    return ok ? (mode == 2 ? 2 : 1) : 0;
}

bool step_engine_takes(omx_qwen3 m) { return step_engine_mode(m) != 0; }

// seg_layer < 0: [embedding + every layer] in one launch; the residual stream after the last layer lands in m->h2.
// seg_layer = i: one segment of the hybrid step -- [gate/up, down] of layer i - 1 on the post-attention residual in m->h2, the new residual
// to m->h; [RMSNorm + q/k/v] of layer i into m->qkv
static int enqueue_step_engine(omx_qwen3 m, hipStream_t s, int seg_layer = -1) {
    const EngineConfig& c = m->cfg;
    const int D = c.head_dim, hd = c.hidden_size;
    StepEngineArgs a = {};
    a.layers = m->se_layers;
    a.L = c.num_hidden_layers; a.hidden = hd; a.H = m->H; a.Hkv = m->Hkv; a.D = D; a.I = m->I; a.cap = m->cap;
    a.eps = c.rms_norm_eps; a.scale = 1.0f / sqrtf((float)D);
    a.embed = m->embed; a.st = m->st; a.seq_ptr = m->step_seq;
    a.rope_cos = m->rope_cos; a.rope_sin = m->rope_sin;
    a.chunk = m->attn_chunk; a.nsplit = m->attn_nsplit;
    uint64_t* g = m->se_gran;
    a.g_x = g; g += hd / 2;
    a.g_x1 = g; g += hd / 2;
    a.g_qkv = g; g += (size_t)(m->H + 2 * m->Hkv) * D / 2;
    a.g_attn = g; g += (size_t)m->H * D / 2;
    a.g_act = g;
    a.g_part = m->attn_gran;
    a.h_out = seg_layer < 0 ? m->h2 : m->h;
    a.seg_layer = seg_layer;
    a.x_in = m->h; a.x1_in = m->h2; a.qkv_out = m->qkv;
    if (seg_layer > 0) a.seg_m = m->se_layers_host[seg_layer - 1];
    if (seg_layer >= 0 && seg_layer < c.num_hidden_layers) a.seg_a = m->se_layers_host[seg_layer];
    a.xcd_major = env_int("OMX_SE_XCD_MAJOR", 1);
    a.abort_flag = m->wait_abort;
    a.nsweep = env_int("OMX_SE_NSWEEP", 1);
    a.inflight = env_int("OMX_SE_INFLIGHT", 2);
    a.thin_gather = env_int("OMX_SE_THIN", 1);
    a.trace = m->se_trace;
    return launch_step_engine(a, m->cus, s);
}

inline void time_next_launch(omx_qwen3 m, int layer, int cls) {
    if (g_launch_recorder) g_launch_recorder->next_tag = cls;
    if (!m->kernel_events) return;
    const size_t i = (cls == KC_HEAD ? (size_t)m->cfg.num_hidden_layers * kLayerClasses
                      : cls == KC_ENGINE ? (size_t)m->cfg.num_hidden_layers * kLayerClasses + 1 : (size_t)layer * kLayerClasses + cls) * 2;
    arm_launch_events((*m->kernel_events)[i], (*m->kernel_events)[i + 1]);
}

// the hybrid step (step_engine_mode == 2): per layer [engine segment] [attention + o]; m->h = residual entering a layer, m->h2 = after attention
static int enqueue_step_hybrid(omx_qwen3 m, bool with_head) {
    const EngineConfig& c = m->cfg;
    hipStream_t s = m->stream;
    const int hd = c.hidden_size, D = c.head_dim, L = c.num_hidden_layers;
    OMX_LAUNCH(embed_kernel, 2, 256, 0, s, m->h, m->embed, m->st, hd, m->step_seq, m->rope_cur, m->rope_cos, m->rope_sin, D / 2);
    OMX_LAUNCH_CHECK();
    for (int l = 0; l < L; ++l) {
        time_next_launch(m, l, KC_QKV);                      // (the segment's time is booked on the q/k/v class of the layer it ends in)
        if (enqueue_step_engine(m, s, l)) return 1;
        const bool fused_o = attention_takes_oproj(m, l);
        time_next_launch(m, l, KC_ATTN);
        if (enqueue_attention(m, l, s, fused_o ? m->h : nullptr, fused_o ? m->h2 : nullptr, nullptr)) return 1;
        if (!fused_o) {
            GemvArgs a = {};
            a.w0 = m->layers[l].o; a.n0 = hd; a.N = hd; a.K = m->H * D;
            a.x = m->attn_out; a.resid = m->h; a.out = m->h2;
            time_next_launch(m, l, KC_O);
            if (launch_gemv(a, PRO_NONE, EPI_RESIDUAL, s)) return 1;
        }
    }
    time_next_launch(m, L - 1, KC_DOWN);
    if (enqueue_step_engine(m, s, L)) return 1;
    if (with_head) time_next_launch(m, 0, KC_HEAD);
    return enqueue_step_tail(m, with_head, m->h, nullptr, 1, false);
}

// enqueue one decode step on m->stream.  with_head=false: prompt token whose logits nobody reads.
// tuning knob: OMX_GEMV_RPW_<QKV|O|GU|DOWN>=n overrides the rows-per-wave (per block for K-split kernels) heuristic of gemv.hip
int enqueue_step(omx_qwen3 m, bool with_head) {
    if (m->cfg.quant_bits) return enqueue_step_quant(m, with_head);
    const EngineConfig& c = m->cfg;
    hipStream_t s = m->stream;
    const int hd = c.hidden_size, D = c.head_dim;
    const bool ep = c.ep_size > 1;                               // expert parallel: attention replicated, one all-reduce per MoE block
    const bool tp = !ep && (c.tp_size > 1 || m->allreduce != nullptr);   // a 1-rank communicator exercises the TP path
    const int engine_mode = step_engine_mode(m);
    if (engine_mode == 2) return enqueue_step_hybrid(m, with_head);
    const bool engine = engine_mode == 1;
    if (engine) {
        time_next_launch(m, 0, KC_ENGINE);
        if (enqueue_step_engine(m, s)) return 1;
    } else {
        OMX_LAUNCH(embed_kernel, 2, 256, 0, s, m->h, m->embed, m->st, hd, m->step_seq, m->rope_cur, m->rope_cos, m->rope_sin, D / 2);
        OMX_LAUNCH_CHECK();
    }
    bf16_t* h = engine ? m->h2 : m->h;      // residual stream entering the layer
    bf16_t* hn = engine ? m->h : m->h2;     // ping-pong partner
    const float* pending = nullptr;   // TP: all-reduced f32 partial not yet folded into h; MoE: the experts' weighted outputs
    int pending_n = 1;                //   ... how many f32 vectors `pending` holds (summed in order by the consumer's prologue)
    // MoE block without its weighted-sum launch (the next GEMV folds the experts' outputs in): every block of that GEMV reads top_k
    // extra f32 vectors, so by default only for top-2 routing (Mixtral-8x7B: 206.4 -> 207.9 tok/s); OMX_MOE_FOLD=1 forces it, 0 disables
    // (not mode 2: its combine adds the shared experts and rounds at other points)
    const bool moe_fold = env_on("OMX_MOE_FOLD", c.num_experts_per_tok <= 2) && c.num_experts > 0 && c.moe_mode != 2 && !ep && !tp;
    // layers 0 .. L-2 end with [down + residual + the next layer's RMSNorm + q/k/v] in one launch: layers 1 .. L-1 find their q/k/v done
    const bool chain = !engine && down_takes_qkv(m);
    for (int l = 0; l < (engine ? 0 : c.num_hidden_layers); ++l) {
        const LayerW& L = m->layers[l];
        if (!(chain && l > 0)) {   // [RMSNorm + QKV GEMV]  model.rs:168-170,324
            GemvArgs a = {};
            const StackedRows q = qkv_rows(m, l);
            a.w0 = q.w0; a.w1 = q.w1; a.w2 = q.w2;
            a.n0 = q.n0; a.n1 = q.n1; a.n2 = q.rows - q.n0 - q.n1;
            a.N = q.rows;
            a.K = hd;
            a.x = h; a.x_partial = pending; a.x_partial_n = pending_n; a.x_out = pending ? hn : nullptr;
            a.norm_w = L.in_ln; a.eps = c.rms_norm_eps;
            a.out = m->qkv;
            a.out_bias = L.qkv_bias;
            a.f16 = m->f16;
            a.rows_per_wave = env_int("OMX_GEMV_RPW_QKV", 0);
            time_next_launch(m, l, KC_QKV);
            if (launch_gemv(a, PRO_RMSNORM, EPI_STORE, s)) return 1;
            if (pending) { std::swap(h, hn); pending = nullptr; pending_n = 1; }
        }
        const bool fused_o = attention_takes_oproj(m, l);
        time_next_launch(m, l, KC_ATTN);
        // [q/k RMSNorm + RoPE + cache append + split-KV SDPA + merge]  model.rs:172-210
        const bool gateup = fused_o && !tp && !pending && attention_takes_gateup(m, l);
        const bool down = gateup && chain && attention_takes_down(m, l);   // ... + down + the next layer's q/k/v: the layer's only launch
        if (enqueue_attention(m, l, s, fused_o ? h : nullptr, fused_o && !tp ? hn : nullptr, fused_o && tp ? m->partial_a : nullptr, gateup, down)) return 1;
        if (down) continue;   // h: the residual stream leaving the layer (the down rows went into the buffer the layer entered on)
        if (fused_o && tp) {   // the rank's f32 partial of the O projection came out of the attention launch
            if (allreduce_sum(m, m->partial_a, hd)) return 1;
            pending = m->partial_a;
        } else if (fused_o) {   // [O projection + residual] happened in the attention launch
            std::swap(h, hn);
        } else {   // [O GEMV + residual]  model.rs:214,325
            GemvArgs a = {};
            a.w0 = L.o; a.n0 = hd; a.N = hd; a.K = m->H * D;
            a.x = m->attn_out;
            a.f16 = m->f16;
            a.rows_per_wave = env_int("OMX_GEMV_RPW_O", 0);
            if (!tp) {
                a.resid = h; a.out = hn;
                time_next_launch(m, l, KC_O);
                if (launch_gemv(a, PRO_NONE, EPI_RESIDUAL, s)) return 1;
                std::swap(h, hn);
            } else {
                a.out = m->partial_a;
                a.peer = peer_fused_fits(m, a.N, a.K) ? m->peer_dev : nullptr;   // peer-store communicator: the rows are reduced over the ranks inside this launch
                if (launch_gemv(a, PRO_NONE, EPI_F32, s)) return 1;
                if (!a.peer && allreduce_sum(m, m->partial_a, hd)) return 1;
                pending = m->partial_a;
            }
        }
        if (c.num_experts > 0 && tp && c.tp_size > 1) {
            // expert tensor parallel: [fold the all-reduced O partial into the residual] [replicated router + this rank's columns of the
            // routed experts] [all-reduce of the slots' f32 partials] [weighted sum + residual with the single-device roundings]
            ep_fold_kernel<<<8, 256, 0, s>>>(hn, h, pending, (int64_t)hd);
            OMX_LAUNCH_CHECK();
            std::swap(h, hn); pending = nullptr; pending_n = 1;
            if (omx_moe_block_partial_tp(m->moe_y, m->moe_inds, m->moe_scores, h, L.post_ln, c.rms_norm_eps, m->moe_xn, L.moe_gate, L.moe_wg,
                                         L.moe_wu, L.moe_wd, 1, hd, m->moe_I, c.num_experts, c.num_experts_per_tok, c.moe_mode, c.norm_topk_prob, s))
                return 1;
            if (allreduce_sum(m, m->moe_y, (size_t)c.num_experts_per_tok * hd)) return 1;
            if (omx_moe_combine_slots(hn, m->moe_y, m->moe_scores, h, 1, hd, c.num_experts_per_tok, s)) return 1;
            std::swap(h, hn);
            continue;
        }
        if (c.num_experts > 0 && ep) {
            // expert parallel: this rank's experts only, partial sums all-reduced, residual folded into the next prologue
            const int el = c.num_experts / c.ep_size;
            if (omx_moe_block_partial_ep(m->partial_b, h, L.post_ln, c.rms_norm_eps, m->moe_xn, L.moe_gate, L.moe_wg, L.moe_wu, L.moe_wd,
                                         1, hd, c.moe_intermediate_size, c.num_experts, c.num_experts_per_tok, c.moe_mode,
                                         c.norm_topk_prob, c.ep_rank * el, el, s))
                return 1;
            if (allreduce_sum(m, m->partial_b, hd)) return 1;
            pending = m->partial_b;
            continue;
        }
        if (layer_is_moe(c, l) && c.moe_mode == 2) {
            // DeepSeek-V2 family: [RMSNorm + float32 router] [gate/up + SwiGLU over top_k + n_shared slots] [down, float32 rows]
            // [weighted sum + shared experts + residual]  (deepseek-ocr2-mlx/src/lib.rs:224-298); a dense layer of the plan falls through
            if (omx_moe_deepseek_block_forward(hn, h, h, L.post_ln, c.rms_norm_eps, m->moe_xn, L.moe_gate, L.moe_wg, L.moe_wu, L.moe_wd,
                                               L.moe_tail, L.sh_gate, L.sh_up, L.sh_down, 1, hd, c.moe_intermediate_size, c.num_experts,
                                               c.num_experts_per_tok, c.n_shared_experts, c.norm_topk_prob, c.routed_scaling_factor, s))
                return 1;
            std::swap(h, hn);
            continue;
        }
        if (layer_is_moe(c, l)) {
            // [RMSNorm] [router] [expert gate/up + SwiGLU] [expert down] [weighted sum] [+ residual]
            // (qwen3_moe.rs:475-503 / mixtral model.rs:296-308, :343-344)
            if (moe_fold) {   // ... without the last two launches: the down GEMVs store the weighted outputs, the next GEMV folds them in
                const int rc = omx_moe_block_partials(m->moe_partials, h, L.post_ln, c.rms_norm_eps, m->moe_xn, L.moe_gate, L.moe_wg, L.moe_wu,
                                                      L.moe_wd, hd, c.moe_intermediate_size, c.num_experts, c.num_experts_per_tok, c.moe_mode,
                                                      c.norm_topk_prob, s);
                if (rc == 0) { pending = m->moe_partials; pending_n = c.num_experts_per_tok; continue; }
                if (rc != 2) return 1;
            }
            if (omx_moe_block_forward(hn, h, h, L.post_ln, c.rms_norm_eps, m->moe_xn, L.moe_gate, L.moe_wg, L.moe_wu, L.moe_wd, 1, hd,
                                      c.moe_intermediate_size, c.num_experts, c.num_experts_per_tok, c.moe_mode, c.norm_topk_prob, s))
                return 1;
            std::swap(h, hn);
            continue;
        }
        if (!gateup) {   // [RMSNorm + gate/up GEMV + SwiGLU]  model.rs:263-265,326 (gateup: happened in the attention launch)
            GemvArgs a = {};
            a.w0 = L.gate; a.w1 = L.up; a.n0 = m->I; a.N = m->I; a.K = hd;
            a.x = h; a.x_partial = pending; a.x_partial_n = pending_n; a.x_out = pending ? hn : nullptr;
            a.norm_w = L.post_ln; a.eps = c.rms_norm_eps;
            a.out = m->act;
            a.f16 = m->f16;
            a.rows_per_wave = env_int("OMX_GEMV_RPW_GU", 0);
            time_next_launch(m, l, KC_GATE_UP);
            if (launch_gemv(a, PRO_RMSNORM, EPI_SWIGLU, s)) return 1;
            if (pending) { std::swap(h, hn); pending = nullptr; pending_n = 1; }
        }
        if (chain && l + 1 < c.num_hidden_layers) {   // [down GEMV + residual] [RMSNorm + QKV GEMV of layer l + 1]: one launch
            const LayerW& Ln = m->layers[l + 1];
            GemvChainArgs a = {};
            a.w_down = L.down; a.N = hd; a.K = m->I;
            a.x = m->act; a.resid = h; a.out = hn;
            a.xg = m->chain_gran; a.seq_ptr = m->step_seq; a.abort_flag = m->wait_abort;
            a.tag_mul = (unsigned)c.num_hidden_layers; a.tag_add = (unsigned)l + 1u;
            a.qkv = qkv_rows(m, l + 1);
            a.norm_w = Ln.in_ln; a.eps = c.rms_norm_eps;
            a.out_bias = Ln.qkv_bias;
            a.qkv_out = m->qkv;
            time_next_launch(m, l, KC_DOWN);              // (the timing hook splits the figure between the two classes by their bytes)
            if (launch_gemv_chain(a, s)) return 1;
            std::swap(h, hn);
        } else {   // [down GEMV + residual]  model.rs:266,327
            GemvArgs a = {};
            a.w0 = L.down; a.n0 = hd; a.N = hd; a.K = m->I;
            a.x = m->act;
            a.f16 = m->f16;
            a.rows_per_wave = env_int("OMX_GEMV_RPW_DOWN", 0);
            if (!tp) {
                a.resid = h; a.out = hn;
                time_next_launch(m, l, KC_DOWN);
                if (launch_gemv(a, PRO_NONE, EPI_RESIDUAL, s)) return 1;
                std::swap(h, hn);
            } else {
                a.out = m->partial_b;
                a.peer = peer_fused_fits(m, a.N, a.K) ? m->peer_dev : nullptr;
                if (launch_gemv(a, PRO_NONE, EPI_F32, s)) return 1;
                if (!a.peer && allreduce_sum(m, m->partial_b, hd)) return 1;
                pending = m->partial_b;
            }
        }
    }
    if (with_head) time_next_launch(m, 0, KC_HEAD);
    return enqueue_step_tail(m, with_head, h, pending, pending_n, tp);
}

// The with-head step as AQL packets on the engine's own queue (aql_step.hpp): OMX_STEP_AQL=1 (agent-scope fences on every packet, the
// semantics of the stream) or =2 (no fences between the packets of a replay -- the step's kernels hand every cross-kernel value over
// with write-through stores and coherent loads).  Greedy single-rank dense / packed steps only: the sampler's, the log-probability
// launches and the MoE block's are not recording sites.  Any failure leaves the engine on its hipGraph (and says why once on stderr with OMX_STEP_AQL_VERBOSE).
int step_aql_mode(omx_qwen3 m) {
    const int mode = env_int("OMX_STEP_AQL", 0);
    const EngineConfig& c = m->cfg;
    if (mode <= 0 || m->aql_disabled || m->eager || m->allreduce != nullptr || c.tp_size > 1 || c.ep_size > 1 || c.num_experts > 0 ||
        m->temperature != 0.f || m->filter_on || m->lp_top >= 0 || step_engine_mode(m) != 0)
        return 0;
    return mode;
}

static void build_aql(omx_qwen3 m) {
    const int mode = step_aql_mode(m);
    if (!mode || m->aql_full) return;
    // the launches are recorded under a stream capture as well: a launch site that is not a recording site would show up as a graph node
    LaunchRecorder rec;
    hipGraph_t g = nullptr;
    if (hipStreamBeginCapture(m->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) { (void)hipGetLastError(); m->aql_disabled = true; return; }
    g_launch_recorder = &rec;
    const int rc = enqueue_step(m, true);
    g_launch_recorder = nullptr;
    const hipError_t e = hipStreamEndCapture(m->stream, &g);
    size_t nodes = 0;
    if (g) { (void)hipGraphGetNodes(g, nullptr, &nodes); (void)hipGraphDestroy(g); }
    AqlProgram* p = nullptr;
    if (!rc && e == hipSuccess && nodes == 0) {
        const int fence = mode == 2 ? AQL_FENCE_NONE : mode == 3 ? AQL_FENCE_ACQUIRE : mode == 4 ? AQL_FENCE_RELEASE : AQL_FENCE_AGENT;
        p = aql_build(rec, fence);
    } else if (!rc && e == hipSuccess) {
        set_error("aql: %zu launches of the step are not recording sites", nodes);
    }
    if (!p) {
        if (getenv("OMX_STEP_AQL_VERBOSE")) fprintf(stderr, "omx: AQL step unavailable: %s\n", omx_last_error());
        (void)hipGetLastError();
        omx_clear_error();
        m->aql_disabled = true;
        return;
    }
    m->aql_full = p;
}

static int build_graphs(omx_qwen3 m) {
    if (m->g_full || m->eager) return 0;
    if (resolve_weights(m)) return 1;
    if (env_on("OMX_NO_GRAPH")) {
        m->eager = true;
        return 0;
    }
    for (int which = 0; which < 2; ++which) {
        hipGraph_t g = nullptr;
        OMX_HIP_CHECK(hipStreamBeginCapture(m->stream, hipStreamCaptureModeThreadLocal));
        const int rc = enqueue_step(m, which == 0);
        hipError_t e = hipStreamEndCapture(m->stream, &g);
        hipGraphExec_t ge = nullptr;
        if (!rc && e == hipSuccess) e = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
        if (g) (void)hipGraphDestroy(g);
        if (rc || e != hipSuccess) {
            (void)hipGetLastError();
            if (m->allreduce != nullptr) {
                // a captured collective was refused: run the same launches eagerly instead
                if (m->g_full) { (void)hipGraphExecDestroy(m->g_full); m->g_full = nullptr; }
                m->eager = true;
                omx_clear_error();
                return 0;
            }
            return rc ? 1 : set_error("step graph capture failed: %s", hipGetErrorString(e));
        }
        (which == 0 ? m->g_full : m->g_nohead) = ge;
    }
    // the captured MoE block's scratch pointers must not move: the expert-parallel block and the expert-TENSOR-parallel one
    // (omx_moe_block_partial_tp bakes its get_workspace_aux pointer into the graph as well)
    if (m->cfg.num_experts > 0 && (m->cfg.ep_size > 1 || m->cfg.tp_size > 1)) workspace_aux_pin(m->stream, true);
    build_aql(m);
    return 0;
}

// Called with the position the next step will process.  The decode attention's split plan is part of the captured graph
// (attn_step.hip: fixed token ranges per split, so that nothing the kernel loads first depends on the position): one plan per
// context bucket of 1024 tokens (4096 beyond 8 k), the graphs are rebuilt when the position enters another bucket.
int context_bucket(omx_qwen3 m, int tk) {
    const int gran = tk <= 8192 ? 1024 : 4096;
    return std::min(m->cap, (tk + gran - 1) / gran * gran);
}
int prepare_step(omx_qwen3 m, int pos) {
    const int want = context_bucket(m, pos + 1);
    if (want != m->graph_tk_max) {
        drop_graphs(m);
        attn_step_plan(want, m->Hkv, m->H / m->Hkv, m->cfg.head_dim, &m->attn_chunk, &m->attn_nsplit);
        m->graph_tk_max = want;
    }
    return build_graphs(m);
}

int run_step(omx_qwen3 m, bool with_head, int pos) {
    if (prepare_step(m, pos)) return 1;
    if (m->eager) return enqueue_step(m, with_head);
    OMX_HIP_CHECK(hipGraphLaunch(with_head ? m->g_full : m->g_nohead, m->stream));
    return 0;
}

// a device-wide barrier of the persistent kernel gave up (a block never arrived): the step's results are void
int step_gave_up(omx_qwen3 m, unsigned* code) {
    OMX_HIP_CHECK(hipMemcpy(code, m->wait_abort, 4, hipMemcpyDeviceToHost));
    return 0;
}
int step_health(omx_qwen3 m) {
    unsigned gave_up = 0;
    if (step_gave_up(m, &gave_up)) return 1;
    OMX_REQUIRE(gave_up == 0, "decode step: a wait inside a launch gave up (code 0x%x: a workgroup of the launch was not resident?)", gave_up);
    return 0;
}

// A launch whose workgroups wait on each other (gate/up inside the attention launch, down + q/k/v in one launch, the persistent step, the O projection inside the attention launch) gave up: some
// workgroup was not resident -- another process or stream holds CUs.  Drop to the next form that needs less co-residency, restore the
// step state the call started from and let the caller run the steps again (the KV rows they wrote are rewritten).  Returns 0 when a
// retry is possible.  The first rung switches off BOTH launches in which a GEMV's weight rows stream across a granule hop (gate/up inside
// the attention launch, down + q/k/v): the flag does not say which launch gave up, both want every CU's register file for themselves, and
// what they save together (3 %) is nothing against a second voided call.
int step_fallback(omx_qwen3 m, const StepState& st) {
    if (m->temperature != 0.f || m->filter_on) return 1;       // the sampler's key sequence / token history advanced: no silent replay
    // more than one rank: a local replay would re-enqueue every all-reduce of the n steps (and the argmax one) on THIS rank only -- its
    // peers never issue them, so the collectives would pair with the peers' next call (wrong sums or a hang).  Report the abort instead.
    if (m->allreduce != nullptr || m->cfg.tp_size > 1 || m->cfg.ep_size > 1) return 1;
    bool gateup = false;
    for (int l = 0; l < m->cfg.num_hidden_layers && !m->gateup_disabled; ++l) gateup = gateup || attention_takes_gateup(m, l);
    const bool chain = !m->chain_disabled && down_takes_qkv(m);
    if (gateup || chain) {
        m->gateup_disabled = m->gateup_disabled || gateup;
        m->chain_disabled = m->chain_disabled || chain;
    }
    else if (!m->se_disabled && step_engine_takes(m)) m->se_disabled = true;
    else if (!m->oproj_disabled && any_layer_takes_oproj(m)) m->oproj_disabled = true;
    else return 1;
    drop_graphs(m);
    OMX_HIP_CHECK(hipMemsetAsync(m->wait_abort, 0, 4, m->stream));
    if (write_step_state(m, st)) return 1;
    OMX_HIP_CHECK(hipStreamSynchronize(m->stream));
    return 0;
}

}  // namespace omx
