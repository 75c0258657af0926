// The Qwen3 engine's model object and what its translation units share: engine.hip (the C API), engine_weights.hip (checkpoint
// tensors), engine_step.hip (the decode step and its captured forms), engine_prefill.hip (the batched prompt / verify / encoder pass),
// engine_score.hip (omx_qwen3_score: that pass + the head over every row in vocabulary panels).
// The library is built without relocatable device code: a kernel lives in the unit that launches it, another unit reaches it through
// a host launcher declared here.
#pragma once
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "attn.hpp"
#include "workspace.hpp"
#include "step_state.hpp"
#include "gemm.hpp"
#include "gemv.hpp"
#include "random.hpp"
#include "sample_filter.hpp"
#include "logprob.hpp"
#include "prefill.hpp"
#include "quant.hpp"
#include "launch_timing.hpp"
#include "aql_step.hpp"
#include "act16.hpp"
#include "peer.hpp"
#include "step_engine.hpp"
#include <hip/hip_fp16.h>

namespace omx {

typedef int (*nccl_allreduce_fn)(const void*, void*, size_t, int, int, void*, hipStream_t);

constexpr int kNcclFloat32 = 7, kNcclUint64 = 5, kNcclBfloat16 = 9, kNcclSum = 0, kNcclMax = 2;

struct LayerW {
    const bf16_t *q, *k, *v, *o, *gate, *up, *down, *q_norm, *k_norm, *in_ln, *post_ln;
    const bf16_t *moe_gate, *moe_wg, *moe_wu, *moe_wd;   // sparse-MoE feed-forward (router + stacked experts)
    // moe_mode 2: the shared MLP whole (checkpoint tensors), and how many pseudo-experts it contributes behind the routed experts of
    // moe_wg / moe_wu / moe_wd (0: those are the checkpoint's stacks; n_shared_experts: owned copies with the split shared MLP appended)
    const bf16_t *sh_gate, *sh_up, *sh_down;
    int moe_tail;
    const bf16_t *q_bias, *k_bias, *v_bias, *qkv_bias;   // Qwen2: projection biases; qkv_bias = the three concatenated (owned)
};

// quantized checkpoint (config.json "quantization", qwen3-mlx/src/model.rs:621-727): every Linear and the embedding are
// (weight u32, scales, biases) triplets; the norm weights stay bf16 in LayerW
struct LayerQ {
    QMat q, k, v, o, gate, up, down;
    QMat moe_router, moe_g, moe_u, moe_d;   // sparse-MoE feed-forward: quantised router and expert stacks
};

// which feed-forward layer l carries: modes 0 / 1 put experts in every layer, mode 2 (DeepSeek-V2 family) behind a dense prefix
// the engine's configuration: the caller's omx_qwen3_config and, behind it, the DeepSeek-V2 family layer plan of omx_qwen3_create_deepseek
// (zeros for every other model)
struct EngineConfig : omx_qwen3_config {
    int first_k_dense_replace = 0, n_shared_experts = 0;
    float routed_scaling_factor = 0.f;
};
inline bool layer_is_moe(const EngineConfig& c, int l) { return c.num_experts > 0 && (c.moe_mode != 2 || l >= c.first_k_dense_replace); }
inline bool any_dense_layer(const EngineConfig& c) { return c.num_experts == 0 || (c.moe_mode == 2 && c.first_k_dense_replace > 0); }

// kernel classes timed by omx_qwen3_time_step_kernels: an event pair armed for the launch that follows (launch_timing.hpp)
enum { KC_QKV = 0, KC_ATTN, KC_O, KC_GATE_UP, KC_DOWN, KC_HEAD, KC_ENGINE, KC_COUNT };
constexpr int kLayerClasses = KC_HEAD;

// Text-encoder use of the same stack (flux-klein-mlx/src/qwen3_encoder.rs:141-224, 403-455): all T tokens through
// layers 0..last tap, hidden states copied out after the tapped layers, attention under an explicit additive mask.
struct EncodeOpts {
    const int* taps;          // ascending layer indices whose OUTPUT is extracted
    int n_taps;
    bf16_t* out;              // [T, n_taps * hidden]
    const bf16_t* mask;       // optional additive [T, T] (causal + padding), nullptr = causal
};

// (BatchSlot, one slot of a batch object in device memory: step_state.hpp)

// One layer of the 8-bit K/V slabs of a kv_bits = 8 batch (MLX affine codes, group 64 along the head dim; KvAffine8, attn_row.hpp):
// codes [Hkv, cap, D] bytes and one word scale | bias (bf16 low | high) per group [Hkv, cap, D / 64] -- a slot's, or slot 0's of the
// batch's allocation
struct Kv8Layer {
    uint8_t *kq, *vq;
    uint32_t *ksb, *vsb;
};

// KV slabs [Hkv, cap, D] per layer a batched pass appends to and attends over instead of the model's own (a batch slot's).
// packed (a slot of a kv_bits = 8 batch): k / v name the batch's ONE bf16 staging pair at every layer and packed[l] is the slot's
// storage -- before layer l's scatter rows [0, off) are expanded into the pair, after it rows [off, off + T) are packed into packed[l]
// and the pair's rows replaced by their dequantised values (launch_kv8_rows)
struct KvSlabs {
    bf16_t* const* k;
    bf16_t* const* v;
    int cap;
    const Kv8Layer* packed = nullptr;
};

// The ragged form of the batched pass: row r is the pending token of slot row_slot[r], at that slot's position, on that slot's slabs
// (slot s of layer l at kbase[l] + s * slot_stride).  Attention splits are `chunk` tokens wide whatever the other rows' lengths;
// ws_o / ws_ml hold nsplit_cap partials per (row, head), of which a launch fills the first `nsplit` at most.
struct RaggedRows {
    BatchSlot* slots;         // device
    const int* row_slot;      // device [T]
    bf16_t* const* kbase;
    bf16_t* const* vbase;
    size_t slot_stride;
    int cap, chunk, nsplit, nsplit_cap;
    float *ws_o, *ws_ml;
    // shared prefixes (omx_qwen3_batch_fork), per listed row and fixed for the call: row r may read tokens [0, grp_shared[r]) from
    // slot grp_owner[r]'s slabs.  grouped = some split has a group worth a grouped block; group_min / group_rows: the tuning of
    // launch_batch_attention (from how many members a split's rows are grouped, and how many member rows one block takes)
    int grp_owner[8], grp_shared[8];
    bool grouped;
    int group_min, group_rows;
    // a kv_bits = 8 batch: kv8[l] = layer l's 8-bit slabs, slot s at + s * slot_stride codes and + s * sb_stride words (kbase / vbase
    // unused, never grouped)
    const Kv8Layer* kv8;
    size_t sb_stride;
};

// Rows the caller of a prompt pass supplies in place of the embedding gather's (omx_qwen3_prefill_embeds): n rows of `hidden` elements
// in device memory, float32 / bf16 / float16, for rows [first, first + n) of the pass
struct RowSpan {
    const void* rows;
    omx_dtype dtype;
    int first, n;
};

}  // namespace omx

using namespace omx;

struct omx_qwen3_ {
    EngineConfig cfg;
    // float16 activations: a packed checkpoint with float16 triplets, or a dense float16 one -- the model then runs in float16 end to
    // end (embedding row, norms, RoPE, K/V slabs, every rounding point, logits, sampler); every float16 branch keys on this
    bool f16 = false;
    int H, Hkv, I, V;            // local (per-rank) heads / intermediate / vocab
    int cap;                     // KV slab capacity in tokens
    std::map<std::string, const void*> named;
    std::vector<void*> owned;    // allocations made by synth_weights
    std::vector<LayerW> layers;
    std::vector<LayerQ> qlayers;             // quantized mode (cfg.quant_bits != 0)
    QMat q_embed = {}, q_head = {};
    // per-matrix MLX formats (omx_qwen3_set_quant_format): module path -> (bits, group); a matrix without an entry has the base format
    // cfg.quant_bits / quant_group.  resolve_weights writes each matrix's format into its QMat: the passes read it from there.
    std::map<std::string, std::pair<int, int>> quant_formats;
    std::vector<const bf16_t*> sb_keys;   // scales pointers registered with quant_register_sb
    bf16_t* dq_buf = nullptr;                // dequantised weight of the GEMM in flight (batched prefill)
    size_t dq_cap = 0;
    // dequantised copies of the layers' packed matrices kept BETWEEN prompts (round 4): 288 GB of HBM hold a dense 8B model's 14 GB of
    // them next to the packed weights, and every prompt after the first skips the dequantise launches (key: the packed words)
    std::map<const uint32_t*, bf16_t*> dq_cache;
    char* dq_slab = nullptr;                 // ONE allocation for all of them (252 hipMallocs between the launches cost a first prompt up to 240 ms)
    size_t dq_slab_bytes = 0, dq_cache_bytes = 0;
    int dq_cache_mode = -1;                  // -1 undecided, 0 off, 1 on
    const bf16_t *embed = nullptr, *final_norm = nullptr, *lm_head = nullptr;
    bool weights_resolved = false;

    hipStream_t stream = nullptr;
    std::vector<bf16_t*> kcache, vcache;
    float *rope_cos = nullptr, *rope_sin = nullptr;
    StepState* st = nullptr;
    uint32_t *out_ring = nullptr, *prompt_dev = nullptr;
    int ring_cap = 4096, prompt_cap = 0;
    bf16_t *h = nullptr, *h2 = nullptr, *qkv = nullptr, *attn_out = nullptr, *act = nullptr, *logits = nullptr;
    bf16_t *moe_xn = nullptr, *moe_out = nullptr;   // MoE feed-forward: normalised input row, block output
    float *partial_a = nullptr, *partial_b = nullptr;   // TP: f32 partial sums awaiting all-reduce
    float* moe_partials = nullptr;                      // MoE decode: [top_k, hidden] weighted expert outputs awaiting the next GEMV's fold
    // expert TENSOR parallel (tp_size > 1 with experts): every expert's intermediate columns sharded over the ranks
    int moe_I = 0;                                      // per-rank expert intermediate width
    float* moe_y = nullptr;                             // [top_k, hidden] f32 partial down projections of the routed slots (all-reduced)
    uint32_t* moe_inds = nullptr;                       // the replicated router's choice, kept for the combine after the all-reduce
    bf16_t* moe_scores = nullptr;
    unsigned long long *argmax_partials = nullptr, *argmax_key = nullptr;
    int n_argmax_partials = 0;
    unsigned *step_seq = nullptr, *wait_abort = nullptr;   // step sequence number (granule tags), word a gather that gave up raises
    // attention of the decode step (attn_step.hip): the split plan is fixed per captured graph and covers positions < graph_tk_max;
    // the graphs are rebuilt when the context outgrows that bucket
    float* rope_cur = nullptr;            // [D] cos | sin of the current position
    uint64_t* attn_gran = nullptr;        // split partials as tagged granules
    uint64_t* attn_xg = nullptr;          // the merged attention vector as granules (O projection in the attention launch)
    uint64_t* chain_gran = nullptr;       // the residual row as granules (down + the next layer's q/k/v in one launch, gemv_chain.hip)
    uint64_t* gateup_gran = nullptr;      // the hidden row behind the O projection as granules (gate/up inside the attention launch)
    uint64_t* act_gran = nullptr;         // the activation vector as granules (down + the next layer's q/k/v inside the attention launch)
    int attn_chunk = 0, attn_nsplit = 0, graph_tk_max = 0;
    unsigned long long* attn_trace = nullptr;   // set for one eager step by omx_qwen3_debug_trace_step
    bf16_t* verify_logits = nullptr;            // [verify_cap, V]: every row's logits of the last omx_qwen3_verify
    uint32_t* verify_tokens = nullptr;
    int verify_cap = 0, verify_rows = 0;
    // omx_qwen3_score (engine_score.hip): one vocabulary panel of logits [score_rows, score_panel], the chunk partials of every row,
    // and (packed head) the panel's dequantised head rows [score_panel, hidden]; allocated on first use and on growth
    bf16_t *score_panel_buf = nullptr, *score_dq = nullptr;
    float *score_part = nullptr, *score_tgt = nullptr, *score_lp = nullptr;
    uint32_t *score_arg = nullptr, *score_targets = nullptr, *score_greedy = nullptr;
    int score_rows = 0, score_panel = 0;
    bool score_dq_on = false;
    hipEvent_t score_ev[3] = {nullptr, nullptr, nullptr};
    float last_score_pass_ms = 0.f, last_score_head_ms = 0.f;
    std::vector<hipEvent_t>* kernel_events = nullptr;   // set for eager steps by omx_qwen3_time_step_kernels: [layer][class][begin, end]

    void* comm = nullptr;
    nccl_allreduce_fn allreduce = nullptr;
    const PeerDev* peer_dev = nullptr;   // the communicator is a peer-store one (peer_allreduce.hip): O / down reduce inside their GEMV

    // sampler (sampler.rs:9-18): 0 = greedy; otherwise categorical(logits / temperature) with the key sequence
    // of mlx-rs RandomState kept on the device: rng[0..1] = state, rng[2..3] = the key of the current draw
    float temperature = 0.f;
    uint32_t* rng = nullptr;
    // filtered sampling (omx_qwen3_set_sampling, sample_filter.hip): penalties / top-k / top-p in front of the draw.  seen [V] bytes = the
    // tokens sampled since the last prefill, marked inside the step; sel = the selection's scratch (per-level histograms)
    bool filter_on = false;
    omx_sampling sampling = {0.f, 0, 1.f, 1.f, 0.f};
    uint8_t* seen = nullptr;
    uint8_t* sel = nullptr;

    // per-token log-probabilities inside the step (omx_qwen3_set_logprobs): lp_top = -1 off, else the alternatives per token.  The rings
    // lie beside out_ring ([ring_cap] and [ring_cap, lp_top]); they and the scratch of the two launches are allocated at the first
    // switch-on, for OMX_LOGPROBS_MAX_TOP.  lp_valid: a token has been sampled since the setting changed
    int lp_top = -1;
    float *lp_ring = nullptr, *top_lp_ring = nullptr;
    uint32_t* top_id_ring = nullptr;
    void* lp_scratch = nullptr;
    bool lp_valid = false;

    // batched-prefill activations (allocated on first use, sized for pf_cap tokens)
    int pf_cap = 0;
    bf16_t *pf_h = nullptr, *pf_h2 = nullptr, *pf_xn = nullptr, *pf_q = nullptr, *pf_k = nullptr, *pf_v = nullptr,
           *pf_qt = nullptr, *pf_attn = nullptr, *pf_g = nullptr, *pf_u = nullptr;
    float* pf_ep_partial = nullptr;      // expert-parallel batched prefill: [pf_ep_cap, hidden] f32 partial of the MoE block
    int pf_ep_cap = 0;
    float last_prefill_ms = 0.f;

    // persistent decode step (step_engine.hip): the layers of a token in one launch
    int cus = 0;                               // compute units of the device: one resident workgroup each
    std::vector<StepEngineLayer> se_layers_host;
    StepEngineLayer* se_layers = nullptr;
    uint64_t* se_gran = nullptr;               // granule buffers of the five vector edges
    unsigned long long* se_trace = nullptr;    // set for one eager step by omx_qwen3_debug_trace_engine
    bool se_disabled = false;                  // a step gave up waiting (a workgroup was not resident): back to one launch per op
    bool oproj_disabled = false;               // the same for the O projection inside the attention launch
    bool chain_disabled = false;               // ... and for down + the next layer's q/k/v in one launch
    bool gateup_disabled = false;              // ... and for gate/up + SwiGLU inside the attention launch

    hipGraphExec_t g_full = nullptr, g_nohead = nullptr;
    AqlProgram* aql_full = nullptr;            // the with-head step as AQL packets on the engine's own HSA queue (aql_step.hpp)
    bool aql_disabled = false;                 // building or replaying it failed once: hipGraph from then on
    bool eager = false;          // fallback when stream capture is unavailable (e.g. a collective refuses capture)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float last_decode_ms = 0.f;
};

namespace omx {

// environment switches: "NAME=1..." turns a switch on (unset: dflt), "NAME=0..." turns one off, NAME=<int> is a number
inline bool env_on(const char* name, bool dflt = false) {
    const char* e = getenv(name);
    return e ? e[0] == '1' : dflt;
}

inline bool env_off(const char* name) {
    const char* e = getenv(name);
    return e && e[0] == '0';
}

inline int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}

inline bool env_is(const char* name, const char* value) {
    const char* e = getenv(name);
    return e && strcmp(e, value) == 0;
}

// a packed MoE layer as the twelve pointers the C entry points of moe.hip take: router, gate, up, down x (words, scales, biases)
#define OMX_QMAT3(q) (q).w, (q).scales, (q).biases
#define OMX_QMOE_ARGS(Q) OMX_QMAT3((Q).moe_router), OMX_QMAT3((Q).moe_g), OMX_QMAT3((Q).moe_u), OMX_QMAT3((Q).moe_d)

template <class T>
inline int dev_alloc(omx_qwen3 m, T** p, size_t n) {
    void* q = nullptr;
    OMX_HIP_CHECK(hipMalloc(&q, n * sizeof(T) + 64));
    // same stream as every later writer: a null-stream hipMemset is not ordered against the
    // engine's non-blocking stream and could zero a buffer after it was filled
    OMX_HIP_CHECK(hipMemsetAsync(q, 0, n * sizeof(T) + 64, m->stream));
    *p = (T*)q;
    m->owned.push_back(q);
    return 0;
}

// engine_weights.hip
int resolve_weights(omx_qwen3 m);
// (bits, group) of the packed matrix at module path `prefix`: its own entry, else the base format
std::pair<int, int> quant_format_of(omx_qwen3 m, const std::string& prefix);

// engine_step.hip
void drop_graphs(omx_qwen3 m);
void recapture_step(omx_qwen3 m);
int rank_allreduce(omx_qwen3 m, void* buf, size_t n, int dtype, int op);
int allreduce_sum(omx_qwen3 m, float* buf, size_t n);
int read_step_state(omx_qwen3 m, StepState* st);
int write_step_state(omx_qwen3 m, const StepState& st);
int reset_sampler_history(omx_qwen3 m);
bool sampling_penalised(const omx_sampling& p);
bool attention_takes_oproj(omx_qwen3 m, int layer);
bool any_layer_takes_oproj(omx_qwen3 m);
bool down_takes_qkv(omx_qwen3 m);
bool attention_takes_gateup(omx_qwen3 m, int layer);
bool attention_takes_down(omx_qwen3 m, int layer);
int step_engine_mode(omx_qwen3 m);
bool step_engine_takes(omx_qwen3 m);
int step_aql_mode(omx_qwen3 m);
int enqueue_step(omx_qwen3 m, bool with_head);
int enqueue_step_tail(omx_qwen3 m, bool with_head, const bf16_t* h, const float* pending, int pending_n, bool tp);
int context_bucket(omx_qwen3 m, int tk);
int prepare_step(omx_qwen3 m, int pos);
int run_step(omx_qwen3 m, bool with_head, int pos);
int step_gave_up(omx_qwen3 m, unsigned* code);
int step_health(omx_qwen3 m);
int step_fallback(omx_qwen3 m, const StepState& st);
int launch_ep_fold(int grid, bf16_t* out, const bf16_t* resid, const float* partial, int64_t n, bool f16, hipStream_t s);

// engine_prefill.hip
int prefill_reserve(omx_qwen3 m, int T, bool dequant = true);
void dq_cache_prepare(omx_qwen3 m);
int packed_rows(const QGemvArgs& g, int T, bf16_t* const* mout, int bits, int pro, int epi, hipStream_t s);
int prefill_prefix_batched(omx_qwen3 m, int T, int off, const EncodeOpts* enc = nullptr, bool full_last = false, bool packed_rows_pass = false,
                           const KvSlabs* kv = nullptr, const RaggedRows* rag = nullptr, const RowSpan* span = nullptr);
int embed_rows(omx_qwen3 m, bf16_t* out, int T, bool rows_form);
void launch_encoder_mask(bf16_t* mask, const uint8_t* am, int T, hipStream_t s);

// engine_score.hip
void score_release(omx_qwen3 m);   // the buffers and events of omx_qwen3_score (destroy)

// the ragged launches of a batched decode step over T <= 8 rows (RaggedRows; engine_batch.hip, the scatter beside its prompt form in
// prefill.hip); q rows go to pf_qt as [T, H, D], the attention output to pf_attn as [T, H * D]
int launch_batch_embed(omx_qwen3 m, const RaggedRows& rag, int T, hipStream_t s);
int launch_batch_scatter(omx_qwen3 m, int layer, const RaggedRows& rag, int T, hipStream_t s);
int launch_batch_attention(omx_qwen3 m, int layer, const RaggedRows& rag, int T, hipStream_t s);
int launch_kv8_rows(const Kv8Layer& L, bf16_t* ks, bf16_t* vs, int Hkv, int D, int cap, int r0, int n, bool pack, hipStream_t s);

}  // namespace omx
