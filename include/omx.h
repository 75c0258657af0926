/*
 * omx.h -- C ABI of libomx_hip.so: the MI355X (gfx950) implementation of the
 * mlx-rs-core inference hot path of OminiX-MLX.
 *
 * This is the drop-in boundary.  The reference's Rust
 * crates reach their arithmetic through the mlx-c C shim (mlx-sys bindgen,
 * mlx-rs/mlx-sys/build.rs:390-399).  Two layers are exported:
 *
 *   1. omx_*  (this file): eager, raw-pointer kernels.  Plain device pointers,
 *      sizes and a hipStream_t (passed as void*; NULL = the null stream).  Each
 *      entry cites the mlx-c function (header:line under
 *      mlx-rs/mlx-sys/src/mlx-c/mlx/c/) and the Rust call site it replaces.
 *   2. mlx_*  (omx_mlx_c.h): the handle-based subset of the mlx-c ABI with the
 *      reference's ownership / status / error-handler conventions, implemented
 *      on top of layer 1, so `mlx-sys` can link against libomx_hip.so.
 *
 * Conventions (same as mlx-c, error.cpp:37-54, fast.cpp:614-632):
 *   - every function returns int: 0 = ok, 1 = error;
 *   - on error the registered handler (omx_set_error_handler == mlx_set_error_handler)
 *     is invoked on the calling thread with a NUL-terminated message; the default
 *     handler stores it in a thread-local slot readable with omx_last_error();
 *   - all tensor arguments are DEVICE pointers, row-major contiguous unless a
 *     stride argument says otherwise; dtype codes are the mlx_dtype values
 *     (array.h:37-52);
 *   - no function allocates, frees or synchronises unless its name says so:
 *     everything is enqueued on `stream` and is hipGraph-capturable.
 */
#ifndef OMX_H
#define OMX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* mlx_dtype numbering (mlx/c/array.h:37-52) */
typedef enum omx_dtype_ {
    OMX_BOOL = 0, OMX_UINT8 = 1, OMX_UINT16 = 2, OMX_UINT32 = 3, OMX_UINT64 = 4,
    OMX_INT8 = 5, OMX_INT16 = 6, OMX_INT32 = 7, OMX_INT64 = 8,
    OMX_FLOAT16 = 9, OMX_FLOAT32 = 10, OMX_FLOAT64 = 11, OMX_BFLOAT16 = 12, OMX_COMPLEX64 = 13
} omx_dtype;

typedef void* omx_stream; /* hipStream_t */

/* ---- library / error plumbing (mlx/c/error.h:15-23, stream.h:63, memory.h:30) ---- */
const char* omx_version(void);
int omx_experiments_built(void);           /* 1: built with `make EXPERIMENTS=1` (persistent step, AQL replay, 32x32 two-phase / stream-K attention) */
typedef void (*omx_error_handler_func)(const char* msg, void* data);
void omx_set_error_handler(omx_error_handler_func handler, void* data, void (*dtor)(void*));
const char* omx_last_error(void);          /* thread-local; "" when none */
void omx_clear_error(void);
int omx_device_count(int* count);
int omx_device_name(char* buf, size_t buflen);
int omx_synchronize(omx_stream stream);    /* mlx_synchronize */

/* device memory (what mlx_array_new_data / mlx_array_data_* do underneath) */
int omx_malloc(void** ptr, size_t bytes);
int omx_free(void* ptr);
int omx_memcpy_h2d(void* dst, const void* src, size_t bytes, omx_stream stream);
int omx_memcpy_d2h(void* dst, const void* src, size_t bytes, omx_stream stream);
int omx_memcpy_d2d(void* dst, const void* src, size_t bytes, omx_stream stream);
int omx_memset(void* dst, int value, size_t bytes, omx_stream stream);

/* synthetic tensors: value(i) = offset + amp*(2*u24(hash(seed,i))-1), RNE to dtype */
int omx_fill_uniform(void* dst, size_t n, uint32_t seed, float amp, float offset, omx_dtype dtype, omx_stream stream);

/* ---- a4: norms.  mlx_fast_rms_norm fast.h:163-168 (mlx-rs/src/fast.rs:165-180),
 *           mlx_fast_layer_norm fast.h:93-99 (fast.rs:204-218).  weight/bias may be NULL.
 *      x, out: [rows, dim] contiguous.                                                      */
int omx_rms_norm(void* out, const void* x, const void* weight, int64_t rows, int dim, float eps,
                 omx_dtype dtype, omx_stream stream);
int omx_layer_norm(void* out, const void* x, const void* weight, const void* bias, int64_t rows, int dim,
                   float eps, omx_dtype dtype, omx_stream stream);

/* ---- a3: RoPE.  mlx_fast_rope fast.h:169-178 (fast.rs:15-46; nn/positional_encoding.rs:112-137).
 *      x,out: [batch(=B*H), T, D] contiguous, position = axis -2, positions offset..offset+T-1.
 *      traditional=0: pairs (i, i+dims/2); =1: pairs (2i, 2i+1).  theta_i = base^(-2i/dims).  */
int omx_rope(void* out, const void* x, int64_t batch, int T, int D, int dims, int traditional, float base,
             float scale, int offset, omx_dtype dtype, omx_stream stream);
/* ... with custom frequencies instead of a base (mlx-rs/src/fast.rs:15-46 `freqs`, mlx-c fast.h mlx_fast_rope): freqs = dims / 2
 * float32 values on the device; the angle of pair j at position p is (p + offset) * scale / freqs[j] */
int omx_rope_freqs(void* out, const void* x, int64_t batch, int T, int D, int dims, int traditional, const float* freqs, float scale,
                   int offset, omx_dtype dtype, omx_stream stream);

/* ---- a8/a9: the two mlx-rs-core fused kernels (metal_kernels.rs:188-236, 260-339), which the
 *      reference JIT-compiles from Metal source through mlx_fast_metal_kernel_apply (fast.h:156).
 *      omx_fused_swiglu(out, x=up, gate): silu(gate)*x.   omx_fused_modulate: (1+scale)*LN(x)+shift,
 *      x [B,S,H], shift/scale [B,H].                                                           */
int omx_fused_swiglu(void* out, const void* x, const void* gate, int64_t n, omx_dtype dtype, omx_stream stream);
int omx_fused_modulate(void* out, const void* x, const void* shift, const void* scale, int B, int S, int H,
                       float eps, omx_dtype dtype, omx_stream stream);

/* ---- a5: Linear.  mlx_matmul ops.h:598-602 / mlx_addmm ops.h:36-43 as used by nn::Linear
 *      (mlx-rs/src/nn/linear.rs:87-92): out[M,N] = x[M,K] . W[N,K]^T (+ bias[N]).
 *      M <= 8 takes the HBM-streaming GEMV path, larger M the MFMA GEMM path.
 *      float16: M <= 8 with K % 8 == 0 (the GEMV's float16 form, bias or not), M > 8 with K % 64 == 0; other shapes fail.  */
int omx_linear(void* out, const void* x, const void* w, const void* bias, int M, int N, int K,
               omx_dtype dtype, omx_stream stream);
/* Linear whose trailing 2*half output features are a [gate | up] pair consumed by fused_swiglu
 * (metal_kernels.rs:188-236) -- the FLUX blocks' mlp_in / to_qkv_mlp projections (klein_model.rs:489-493,
 * 905-916).  W [n_plain + 2*half, K].  out_plain [M, n_plain] = x . W[:n_plain]^T,
 * out_act [M, half] = silu(g) * u with g, u the bf16-rounded gate / up features: the same bits as
 * omx_linear followed by omx_fused_swiglu, without the 2*half wide intermediate in HBM.
 * n_plain % 4 == 0, half % 4 == 0, K % 64 == 0; other widths fail (use omx_linear + omx_fused_swiglu).   */
int omx_linear_swiglu(void* out_plain, void* out_act, const void* x, const void* w, int M, int n_plain,
                      int half, int K, omx_dtype dtype, omx_stream stream);

/* ---- a1: SDPA.  mlx_fast_scaled_dot_product_attention fast.h:189-198 (fast.rs:121-151;
 *      mlx-rs-core/src/utils.rs:191-209).  q [B,H,Tq,D]; k,v [B,Hkv,Tk,D] with explicit element
 *      strides so that the [..,:offset,:] views of the step-256 KV buffer (cache.rs:190-193) are
 *      passed without a copy: kv_batch_stride, kv_head_stride (row stride is D).
 *      mask_mode: 0 none, 1 "causal" (bottom-right aligned), 2 bool array [Tq,Tk] (keep-true),
 *      3 additive array [Tq,Tk] of `dtype`.  out [B,H,Tq,D].                                   */
enum { OMX_MASK_NONE = 0, OMX_MASK_CAUSAL = 1, OMX_MASK_BOOL = 2, OMX_MASK_ADDITIVE = 3 };
int omx_sdpa(void* out, const void* q, const void* k, const void* v, int B, int H, int Hkv, int Tq, int Tk,
             int D, int64_t kv_batch_stride, int64_t kv_head_stride, float scale, int mask_mode,
             const void* mask, omx_dtype dtype, omx_stream stream);
/* bytes of scratch omx_sdpa needs for the split-KV decode path (0 for prefill) */
size_t omx_sdpa_workspace_bytes(int B, int H, int Tq, int D);
int omx_set_workspace(void* ws, size_t bytes);   /* caller-provided scratch used by split kernels */

/* ---- a10: greedy sampler.  mlx_argmax_axis ops.h:106-111 (mlx-rs-core/src/sampler.rs:9-12):
 *      out[r] = first index of the maximum of logits[r, :]  (u32).                              */
int omx_argmax(uint32_t* out, const void* logits, int64_t rows, int n, omx_dtype dtype, omx_stream stream);

/* ---- per-row log-probability of a target column (csrc/logprob.hip): what a text's log-likelihood is made of.  The reference gets it
 *      from the [B, L, V] logits of qwen3-mlx/src/model.rs:480-490 by log_softmax + take; here no softmax row is ever written.
 *      logits: bf16 [rows, ld] (ld >= V, the row stride in elements), targets: DEVICE u32 [rows].
 *        lse[r]      = log sum_v exp(logits[r, v])                       (f32; nullable)
 *        logprobs[r] = f32(logits[r, targets[r]]) - lse[r]               (0 where targets[r] == OMX_NO_TARGET)
 *        greedy[r]   = first index of the row's maximum, omx_argmax's rule  (nullable)
 *      A target >= V that is not OMX_NO_TARGET gives logprobs[r] = NaN (no chunk holds it); nothing is read out of bounds.
 *      The rule: a row is cut into 1024-column chunks counted from column 0; one wave reduces one (row, chunk) to
 *      (m = max, l = sum exp(x - m) in f32: 16 terms per lane in index order, then a fixed lane tree, arg = first index of m);
 *      a second launch merges a row's ceil(V/1024) partials in ascending chunk order: M = max m_j, L = sum l_j * exp(m_j - M),
 *      lse = M + log L.  Chunk grid and every summation order are functions of V alone, so a row's bits depend on neither the
 *      number of rows, the rows it shares a launch with, nor the panel widths of the two-phase form.
 *      Refused: V % 8 != 0, ld % 8 != 0 (16-byte loads), a dtype other than OMX_BFLOAT16, V > 2^20.
 *      omx_logprob_rows: the whole row as one panel, the partials in the library workspace.
 *      The two-phase form the engine uses: omx_logprob_partial reduces the chunks of columns [c0, c0 + P) of the row, read from a
 *      panel [rows, ld] whose column 0 is the row's column c0 (c0 % 1024 == 0; P % 1024 == 0 unless c0 + P == V), into
 *      partials [rows, ceil(V/1024), 2] f32 (m, l) + part_arg [rows, ceil(V/1024)] u32 and tgt [rows] f32 (written by the one chunk
 *      that holds the target); omx_logprob_merge, once every chunk has been written, produces the three outputs.              */
#define OMX_NO_TARGET 0xFFFFFFFFu
#define OMX_LOGPROB_CHUNK 1024
int omx_logprob_rows(float* logprobs, uint32_t* greedy /*nullable*/, float* lse /*nullable*/, const void* logits, int64_t ld,
                     const uint32_t* targets, int64_t rows, int V, omx_dtype dtype /*OMX_BFLOAT16*/, omx_stream stream);
int omx_logprob_partial(float* partials, uint32_t* part_arg, float* tgt, const void* panel, int64_t ld, int c0, int P,
                        const uint32_t* targets, int64_t rows, int V, omx_dtype dtype, omx_stream stream);
int omx_logprob_merge(float* logprobs, uint32_t* greedy /*nullable*/, float* lse /*nullable*/, const float* partials,
                      const uint32_t* part_arg, const float* tgt, const uint32_t* targets, int64_t rows, int V, omx_stream stream);
/* ---- ... with the row's top_n alternatives beside it: what a decode step reports about the token it drew (omx_qwen3_set_logprobs).
 *      logprobs, greedy and lse are BIT FOR BIT what omx_logprob_rows writes for the same inputs: the chunk grid, the summation orders
 *      and the arithmetic above are the same text.  Besides them
 *        top_ids[r, j]      = the j-th column of row r in the order (logit descending, column index ascending) -- the order of the 64-bit
 *                             key the samplers draw with (+0 above -0, NaN below everything), so top_ids[r, 0] == greedy[r] always
 *        top_logprobs[r, j] = f32(logits[r, top_ids[r, j]]) - lse[r]      (one f32 subtraction from the row's own lse)
 *      Only columns < V take part; the padding up to ld is never read as a logit.  1 <= top_n <= min(OMX_LOGPROBS_MAX_TOP, V); anything
 *      else is refused, as are the dtypes and shapes omx_logprob_rows refuses.  Two launches for all rows whatever top_n is: the chunk
 *      wave also leaves the chunk's own best top_n (top_n rounds of a wave-wide maximum over its 1024 keys, in registers), the merge
 *      block picks the row's top_n from the heads of the ceil(V/1024) descending lists.  A row's outputs depend on neither the number
 *      of rows, the rows beside it, nor the panel widths of the two-phase form.
 *      Two-phase form: omx_logprob_top_partial = omx_logprob_partial + cand [rows, ceil(V/1024), top_n] u32 (a chunk's candidates, an
 *      internal encoding); omx_logprob_top_merge, once every chunk has been written.                                              */
#define OMX_LOGPROBS_MAX_TOP 20
int omx_logprob_rows_top(float* logprobs, uint32_t* greedy /*nullable*/, float* lse /*nullable*/, uint32_t* top_ids /*[rows, top_n]*/,
                         float* top_logprobs /*[rows, top_n]*/, const void* logits, int64_t ld, const uint32_t* targets, int64_t rows,
                         int V, int top_n, omx_dtype dtype /*OMX_BFLOAT16*/, omx_stream stream);
int omx_logprob_top_partial(float* partials, uint32_t* part_arg, float* tgt, uint32_t* cand, const void* panel, int64_t ld, int c0, int P,
                            const uint32_t* targets, int64_t rows, int V, int top_n, omx_dtype dtype, omx_stream stream);
int omx_logprob_top_merge(float* logprobs, uint32_t* greedy /*nullable*/, float* lse /*nullable*/, uint32_t* top_ids, float* top_logprobs,
                          const float* partials, const uint32_t* part_arg, const float* tgt, const uint32_t* cand,
                          const uint32_t* targets, int64_t rows, int V, int top_n, omx_stream stream);

/* ---- a10, temperature branch: MLX's keyed generator + categorical sampler.
 *      mlx/c/random.h:37-72,129-139,149-157 (mlx_random_bits / _categorical* / _gumbel / _key / _split* / _uniform),
 *      called by mlx-rs/src/random.rs:98-115 (key, split), :397-414 (gumbel), :456-497 (categorical) and through
 *      them by mlx-rs-core/src/sampler.rs:13-16.  Keys are 2 x u32 in device memory; word i of an n-word draw is
 *      Threefry-2x32(key, counter pair of i) in MLX's layout, so results reproduce MLX's for the same key.
 *      categorical: out[r, s] = argmax_v( f32(logits[r, v]) * inv_temp + gumbel[r, v, s] ), first index on ties.   */
int omx_random_key(uint32_t* key, uint64_t seed, omx_stream stream);
int omx_random_split(uint32_t* out /*[num,2]*/, const uint32_t* key, int num, omx_stream stream);
int omx_random_bits(uint32_t* out, const uint32_t* key, int64_t n, omx_stream stream);
int omx_random_uniform(float* out, const uint32_t* key, int64_t n, float lo, float hi, omx_stream stream);
int omx_random_gumbel(float* out, const uint32_t* key, int64_t n, omx_stream stream);
/* mlx_random_normal (random.h:100-108; mlx-rs/src/random.rs:186-212): sqrt(2) * erfinv(uniform(-1, 1)) * scale + loc, f32 */
int omx_random_normal(float* out, const uint32_t* key, int64_t n, float loc, float scale, omx_stream stream);
int omx_random_categorical(uint32_t* out, const void* logits, int64_t rows, int n, int num_samples, float inv_temp,
                           const uint32_t* key, omx_dtype dtype, omx_stream stream);

/* ---- filtered sampling (csrc/sample_filter.hip): what the reference's generation loops do beside the 19-line sampler --
 *      funasr-qwen4b-mlx/src/model.rs:1333-1383 (sample_top_k_p: presence penalty, top-k), step-audio2-mlx/src/llm.rs:440-474
 *      (apply_repetition_penalty), gpt-sovits-mlx/src/sampling.rs:122-215 (repetition penalty, top-p, temperature, top-k).
 *      The rule, one IEEE float32 operation per element and step, for a row of V logits and a set `seen` of token ids:
 *        1. x = f32(logit)
 *        2. repetition_penalty r != 1, v seen:  x = x > 0 ? x / r : x * r          (step-audio2)
 *        3. presence_penalty q != 0, v seen:    x = x - q                          (funasr-qwen4b; with both set: 2 then 3, this
 *                                                                                   project's choice -- the reference never sets both)
 *        4. y = x * (1/T), 1/T rounded to f32 first (as omx_random_categorical)
 *        5. top_k (0 or >= V: off): keep y >= the k-th largest y; ties at the threshold are ALL kept (the reference's `ge`)
 *        6. top_p (1: off) on the survivors of 5 (temperature, top-k, top-p: the HF / vLLM order): with Z = sum exp(y - max) over
 *           them, keep v iff the mass of survivors with y STRICTLY greater than y_v is < top_p * Z.  A tie group stays or goes whole,
 *           the maximum always stays.  (gpt-sovits-mlx/src/sampling.rs:180-203 drops a token when the INCLUSIVE mass exceeds p,
 *           which depends on the order of equal values and can drop every token: not reproduced, on purpose.)
 *        7. token = argmax over the kept set of y + gumbel(word r*V + v of a rows*V-word draw from key), first index on ties:
 *           with every filter and penalty off, omx_random_categorical bit for bit.
 *      temperature 0: argmax of x after steps 2-3 (no key needed).  Masses are summed exactly (2^-40 fixed point, 64-bit).       */
typedef struct omx_sampling_ {
    float temperature;          /* >= 0 */
    int32_t top_k;              /* 0 = off */
    float top_p;                /* in (0, 1]; 1 = off */
    float repetition_penalty;   /* > 0; 1 = off */
    float presence_penalty;     /* 0 = off */
} omx_sampling;
/* seen: V bytes, non-zero = the id was generated (NULL: none).  thr_out [rows] (nullable): the final threshold on y, -inf when
 * nothing is filtered; kept_out [rows] (nullable): the number of entries with y >= that threshold.
 * One launch, one block per row; a single row of 16 384 entries or more: a launch per level of the selection over many blocks, with its
 * histograms in the library's workspace (omx_set_workspace / grown outside graph capture, like the split kernels').              */
int omx_sample_filtered(uint32_t* out_token, const void* logits, omx_dtype dtype, int64_t rows, int V, const omx_sampling* p,
                        const uint8_t* seen, const uint32_t* key, float* thr_out, int32_t* kept_out, omx_stream stream);
/* mlx_topk_axis (ops.h; funasr-qwen4b-mlx/src/model.rs:1357) on the same selection: out [rows, k] = the k largest of x [rows, V] in
 * ascending order, dtype of x.  k <= 4096.                                                                                      */
int omx_topk_values(void* out, const void* x, omx_dtype dtype, int64_t rows, int V, int k, omx_stream stream);

/* embedding gather (mlx_take_axis ops.h:1109, nn/embedding.rs): out[r,:] = table[ids[r],:] */
int omx_take_rows(void* out, const void* table, const uint32_t* ids, int64_t n_ids, int dim, omx_dtype dtype,
                  omx_stream stream);
/* elementwise add (mlx_add): residual connections */
int omx_add(void* out, const void* a, const void* b, int64_t n, omx_dtype dtype, omx_stream stream);

/* 2-D synthetic fill of a shard of a logical [*, ld_full] tensor: element (r,c) of dst[rows,cols]
 * takes the value of logical index (row0+r)*ld_full + (col0+c) -- tensor-parallel shards of the
 * same logical weight are bit-identical to slices of the single-GPU tensor.                        */
int omx_fill_uniform_2d(void* dst, int64_t rows, int64_t cols, int64_t ld_full, int64_t row0, int64_t col0,
                        uint32_t seed, float amp, float offset, omx_dtype dtype, omx_stream stream);

/* =====================================================================================
 * Fused decode engine: the qwen3-mlx dense decoder + greedy Generate loop as ONE captured
 * hipGraph per token (qwen3-mlx/src/model.rs:161-215, 263-267, 321-332,
 * 394-424, 480-490, 733-741, 804-843).  Per layer: [RMSNorm+QKV GEMV] [q/k-norm+RoPE+cache
 * write+split-KV attention] [combine] [O GEMV+residual] [RMSNorm+gate/up GEMV+SwiGLU]
 * [down GEMV+residual]; then [RMSNorm+lm_head GEMV+argmax].  Weights are borrowed device
 * pointers registered under their HF checkpoint key names (model.rs:631-716).
 * ===================================================================================== */
typedef struct omx_qwen3_config_ {
    int hidden_size, num_hidden_layers, intermediate_size, num_attention_heads, num_key_value_heads, head_dim,
        vocab_size;
    float rms_norm_eps, rope_theta, rope_scale;   /* rope_scale = 1/factor for "linear" (utils.rs:70-85) */
    int tie_word_embeddings;
    int max_context;                              /* KV slab capacity (rounded up to the 256 step of cache.rs) */
    int tp_rank, tp_size;                         /* tensor parallel shard of this process (1 process per GPU) */
    /* config.json "quantization" {bits, group_size} (qwen3-mlx/src/model.rs:63, 621-727): 0 = bf16 checkpoint;
     * 4 / 8 = every Linear and the embedding are MLX (weight u32, scales, biases) triplets registered as
     * "<prefix>.weight" / ".scales" / ".biases"; the decode step then streams the PACKED weights (csrc/quant.hip) */
    int quant_bits, quant_group;
    /* sparse-MoE feed-forward in every layer (0 experts = dense MLP): Qwen3-MoE (qwen3-mlx/src/qwen3_moe.rs:440-508, mode 1,
     * weights "model.layers.N.mlp.gate.weight" [E, hidden] and "...mlp.switch_mlp.{gate,up,down}_proj.weight" stacked
     * [E, moe_intermediate_size, hidden] / [E, hidden, moe_intermediate_size]) or Mixtral (mixtral-mlx/src/model.rs:280-347,
     * mode 0, the same names under "block_sparse_moe.").  no_qk_norm: attention without q/k RMSNorm (Mixtral, :120-160). */
    int num_experts, num_experts_per_tok, moe_intermediate_size, moe_mode, norm_topk_prob, no_qk_norm;
    /* expert parallelism (one process per GPU): this rank holds experts [ep_rank*E/ep_size, ...) -- the stacked
     * expert tensors registered are ITS slices -- attention and router replicated; one all-reduce per layer (omx_qwen3_set_comm) */
    int ep_rank, ep_size;
    /* Qwen2 wiring (qwen3-mlx/src/qwen2.rs:100-218): q/k/v projections carry a bias ("self_attn.{q,k,v}_proj.bias") and the
     * attention has no q/k norm (set no_qk_norm too); bf16; under tensor parallelism the biases are sharded like their rows */
    int attention_bias;
    /* quantized checkpoints only: scales / biases are float16 (an MLX float16 checkpoint; nn/quantized.rs:361-385 takes any float).
     * They enter the arithmetic as their exact float32 values; activations and outputs stay bf16.  Dense decoders (not with experts). */
    int quant_scales_f16;
    /* dense (quant_bits 0) checkpoints only: the weights are float16 (MLX keeps a model in the dtype it was saved in), and the model runs
     * in float16 end to end -- embedding, norms, RoPE, K/V, every rounding point and the logits.  Single rank, no experts, no
     * attention_bias, head_dim 128; omx_qwen3_verify refuses such a model.  0 = bfloat16 weights. */
    int float16_weights;
} omx_qwen3_config;
typedef struct omx_qwen3_* omx_qwen3;

int omx_qwen3_create(omx_qwen3* out, const omx_qwen3_config* cfg);
/* DeepSeek-V2 family layer plan (cfg->moe_mode 2; deepseek-ocr2-mlx/src/lib.rs:988): layers [0, first_k_dense_replace) carry a dense SwiGLU
 * MLP of intermediate_size ("mlp.{gate,up,down}_proj"), the rest the float32 router "mlp.gate", the stacks "mlp.switch_mlp.*" and --
 * n_shared_experts > 0 -- one shared MLP "mlp.shared_experts.{gate,up,down}_proj" of width n_shared_experts * moe_intermediate_size
 * added to the routed sum; the router's weights are multiplied by routed_scaling_factor (omx_moe_deepseek_forward).  bf16, single
 * rank, no attention_bias.  The plan travels beside omx_qwen3_config, whose layout stays as it is; omx_qwen3_create on a mode-2 config
 * is the plan {0, 0, 1.0} (every layer routes, no shared experts).  Modes 0 / 1 take no plan: all three zero (the factor 0 or 1). */
typedef struct omx_qwen3_deepseek_plan_ {
    int first_k_dense_replace, n_shared_experts;
    float routed_scaling_factor;
} omx_qwen3_deepseek_plan;
int omx_qwen3_create_deepseek(omx_qwen3* out, const omx_qwen3_config* cfg, const omx_qwen3_deepseek_plan* plan);
int omx_qwen3_destroy(omx_qwen3 m);
/* register a weight by HF key name; `ptr` is this rank's shard (column-split q/k/v/gate/up/lm_head rows,
 * row-split o/down columns), bf16 (packed u32 / bf16 scales, biases for a quantized checkpoint), contiguous, `nbytes` long: the
 * engine reads raw pointers, so a tensor whose size disagrees with the config is refused here ("ShapeMismatch", the reference's
 * load-time shape error) instead of being read past its end                                         */
int omx_qwen3_set_weight(omx_qwen3 m, const char* name, const void* ptr, size_t nbytes);
/* Mixed-precision MLX checkpoints (mlx_lm.convert --quant-predicate mixed_*): config.json's "quantization" block carries, next to the
 * global bits / group_size, an entry per module path ("model.layers.3.mlp.down_proj": {"group_size": 64, "bits": 6}).  The config's
 * quant_bits / quant_group stay the BASE format; this call gives ONE packed matrix its own.  prefix: the module path as in the
 * checkpoint -- model.embed_tokens, lm_head (untied models; a tied head has the embedding's format),
 * model.layers.<i>.self_attn.{q,k,v,o}_proj, model.layers.<i>.mlp.{gate,up,down}_proj.  Legal after omx_qwen3_create and before any tensor
 * of that prefix is set or synthesised.  Refused by name: an unknown prefix, bits outside {2,3,4,5,6,8}, a group outside {32,64,128} or
 * one that does not divide the matrix's contraction width, a model without base quantization, and models with experts, tp_size /
 * ep_size > 1, float16 triplets or attention_bias.  gate_proj and up_proj of a layer must end up in one format (checked when the
 * weights are resolved).  A model without any such call launches exactly what it launched before. */
int omx_qwen3_set_quant_format(omx_qwen3 m, const char* prefix, int bits, int group_size);
/* the format of a packed matrix: its own, or the base format where nothing was set */
int omx_qwen3_quant_format(omx_qwen3 m, const char* prefix, int* bits, int* group_size);
/* device pointer (+ expected byte length; 0 = unknown) of a registered or synthesised tensor by checkpoint name */
int omx_qwen3_get_weight(omx_qwen3 m, const char* name, const void** ptr, size_t* nbytes);
/* allocate + fill every weight with the seeded synthetic generator (seed = base ^ crc32(name))      */
int omx_qwen3_synth_weights(omx_qwen3 m, uint32_t base_seed);
/* ... with PEAKED logits: embedding std 64, lm_head[v] = table[(v + 1) mod V] at std 0.02 -- the greedy successor of token t is t - 1 with
 * a margin two orders of magnitude above the bf16 bound, so full-size parity tests can assert token EQUALITY (bf16, untied head) */
int omx_qwen3_synth_weights_peaked(omx_qwen3 m, uint32_t base_seed);
/* tensor-parallel hook: `allreduce` has the ncclAllReduce signature, `comm` is the ncclComm_t.      */
int omx_qwen3_set_comm(omx_qwen3 m, void* comm, void* allreduce_fn);
/* sampler (mlx-rs-core/src/sampler.rs:9-18, qwen3-mlx/src/model.rs:733-741): temperature 0 = argmax (default);
 * otherwise every sampled token is categorical(logits * (1/temperature)) with the next key of a RandomState
 * seeded like mlx_rs::random::seed(seed) (random.rs:21-41, :88-91).  The draw stays on the device, inside the step. */
int omx_qwen3_set_sampler(omx_qwen3 m, float temperature, uint64_t seed);
/* filtered sampling inside the step (omx_sample_filtered's rule; `seen` = the tokens sampled since the last prefill / reset, the
 * prompt excluded, kept on the device and marked by the step itself).  Every sampled token -- prefill's first one and each decode step,
 * which stays one hipGraph -- goes through [select] [noise over the kept set] [finalize] [mark seen].  omx_qwen3_set_sampler turns
 * every filter and penalty off again.  Refused: tensor-parallel engines (a sharded vocabulary needs a histogram all-reduce);
 * omx_qwen3_verify / _trim refuse while a filter or penalty is on (their rows are not part of the history).                      */
int omx_qwen3_set_sampling(omx_qwen3 m, const omx_sampling* p, uint64_t seed);
/* text-encoder use of the stack (flux-klein-mlx/src/qwen3_encoder.rs:403-455, `forward_with_hidden_states` + `encode`):
 * all n tokens through layers 0..tap_layers[n_taps-1]; out (DEVICE, bf16) [n, n_taps*hidden] = the raw hidden states
 * after the tapped layers, concatenated on the last axis (FLUX.2-klein: taps 8,17,26 -> 7680 of Qwen3-4B).
 * attention_mask (host, [n] of 0/1, may be NULL = causal only) adds the padding mask of qwen3_encoder.rs:172-198.  */
int omx_qwen3_encode(omx_qwen3 m, const uint32_t* ids, int n, const uint8_t* attention_mask, const int* tap_layers, int n_taps,
                     void* out_dev);
int omx_qwen3_reset(omx_qwen3 m);                                  /* KVCache::reset (cache.rs:130-132) */
int omx_qwen3_offset(omx_qwen3 m, int* offset);                    /* KeyValueCache::offset           */
/* Generate: prefill the prompt, return the first sampled token (model.rs:808-827)                   */
int omx_qwen3_prefill(omx_qwen3 m, const uint32_t* prompt, int n_prompt, uint32_t* first_token);
/* A prompt pass whose rows the caller can supply -- the reference's forward_embeddings(inputs_embeds, cache), the door every multimodal
 * crate goes through (qwen3-asr-mlx/src/model.rs:720-769, 782: audio rows over the <|audio_pad|> positions).
 *   embed_tokens:   get_token_embeddings (:726, :814) -- the model's own embedding rows of n ids, [n, hidden] in the activation dtype
 *                   (bf16; float16 for a float16 model), written to DEVICE memory out_rows; the bits the prompt pass itself gathers.
 *   prefill_embeds: omx_qwen3_prefill with rows [first_row, first_row + n_rows) of the pass overwritten, after the embedding gather and
 *                   in one launch, by `rows` (DEVICE, [n_rows, hidden] of rows_dtype OMX_FLOAT32 / OMX_BFLOAT16 / OMX_FLOAT16, converted
 *                   to the activation dtype round-to-nearest-even as as_dtype does, :759).  Everything else is omx_qwen3_prefill: the
 *                   ids at the overridden positions are still required and range-checked (pass the pad token), the cache may be
 *                   non-empty, the span may include the last row.  n_rows = 0 IS omx_qwen3_prefill (rows may be NULL).
 * Refused by name with n_rows > 0: a span outside the prompt, NULL rows, another dtype; tensor-parallel, expert-parallel and sparse-MoE
 * engines; and "InvalidConfig" where omx_qwen3_prefill would go token-serial, through the decode step, which reads the embedding table
 * itself -- OMX_PREFILL_SERIAL=1, OMX_PREFILL_TAIL_STEP=1, n_prompt < 2, a float16 model with n_prompt <= 16.  n_rows < 0 is refused. */
int omx_qwen3_embed_tokens(omx_qwen3 m, const uint32_t* ids, int n, void* out_rows);
int omx_qwen3_prefill_embeds(omx_qwen3 m, const uint32_t* prompt, int n_prompt, const void* rows, omx_dtype rows_dtype, int first_row,
                             int n_rows, uint32_t* first_token);
/* Generate: n further greedy tokens (model.rs:828-841); tokens_out is a HOST buffer of n entries    */
int omx_qwen3_decode(omx_qwen3 m, int n, uint32_t* tokens_out);
/* copy the logits of the last executed step ([vocab_local] bf16) to a host buffer                  */
int omx_qwen3_last_logits(omx_qwen3 m, void* host_bf16, int n);
/* Per-token log-probabilities of the tokens being generated, inside the step (opt-in; off, nothing the engine launches or allocates
 * changes).  set_logprobs: top_n = -1 off (default), 0 = the drawn token's log-probability only, 1..min(OMX_LOGPROBS_MAX_TOP, V) = with that
 * many alternatives.  While on, every sampled token -- the prefill's first and each decode step, which stays ONE hipGraph per context
 * bucket -- is followed by the two launches of omx_logprob_rows_top over the step's logits row; the target is the token the finalize
 * just wrote, on the device, and the results go into rings beside the token ring at the entry the device derives from its own count.
 * What is reported is the log-softmax of the row omx_qwen3_last_logits returns, the model's RAW logits: before temperature, top-k /
 * top-p and penalties -- what omx_qwen3_score reports for the same position.  Under a sampler the drawn token need not be top_ids[0].
 * The OMX_STEP_AQL / OMX_STEP_ENGINE forms of the step are not taken while it is on (as with a sampler).
 *   decode_logprobs: omx_qwen3_decode + logprobs [n] and, top_n > 0, top_ids / top_logprobs [n, top_n] (both nullable), HOST buffers.
 *   last_logprobs:   the same for the most recently sampled token (after a prefill: its first token); top_ids / top_logprobs nullable.
 * Refused by name: tensor / expert parallel models (a sharded vocabulary), float16 models, top_n outside -1..min(20, V), and
 * decode_logprobs / last_logprobs while off (last_logprobs also before any token was sampled since set_logprobs).               */
int omx_qwen3_set_logprobs(omx_qwen3 m, int top_n);
int omx_qwen3_decode_logprobs(omx_qwen3 m, int n, uint32_t* tokens_out, float* logprobs /*[n]*/, uint32_t* top_ids /*[n, top_n], nullable*/,
                              float* top_logprobs /*[n, top_n], nullable*/);
int omx_qwen3_last_logprobs(omx_qwen3 m, float* logprob, uint32_t* top_ids /*[top_n], nullable*/, float* top_logprobs /*nullable*/);
/* Speculative decoding support (mlx-rs-core/src/speculative.rs).
 *   verify: verify_draft_tokens :132-161 -- the n tokens [last accepted, draft 1 .. draft n-1] in ONE batched pass on top of the cache
 *           (their K/V rows are appended), greedy_out[i] = argmax of the logits after token i; afterwards the pending input token is
 *           greedy_out[n-1].  Single-rank bf16 models.  verify_logits: bf16 logits [V] of one row of the last verify call.
 *   trim:   KeyValueCache::trim(n), the operation :165-169 notes the reference's cache trait lacks: forget the last n cached tokens
 *           and make next_token the pending input token (n = 0: only replace the token).                                             */
/*           With a sampler set (temperature != 0) each row's token is drawn categorical(logits / T) with the next key of the model's
 *           sequence (speculative.rs:104-109, :145-148) instead of the argmax.
 *   sampler_state: the two words of the key sequence (mlx-rs RandomState); set != 0 writes them.  The reference draws the draft's and
 *           the target's tokens from ONE global sequence: two models reproduce it by handing the state over.                        */
int omx_qwen3_verify(omx_qwen3 m, const uint32_t* tokens, int n, uint32_t* greedy_out);
int omx_qwen3_sampler_state(omx_qwen3 m, uint32_t* state2, int set);
int omx_qwen3_verify_logits(omx_qwen3 m, int row, void* host_bf16, int n);
int omx_qwen3_trim(omx_qwen3 m, int n, uint32_t next_token);
/* Score a text (csrc/engine_score.hip): logprobs[i] = log p(targets[i] | cache, tokens[0..i]) for every one of the n tokens, from ONE
 * batched prompt pass -- the log-likelihood the reference would take from the [B, L, V] logits of model.rs:480-490.  The head runs over
 * all n rows in vocabulary panels (OMX_SCORE_PANEL columns, a multiple of 1024, default 16384, read per call): [panel GEMM] [chunk
 * partials, omx_logprob_partial] per panel and one merge; no [n, V] tensor exists.  A packed head (or tied packed embedding) is
 * dequantised a panel at a time in its own format.  targets[i] == OMX_NO_TARGET: logprobs[i] = 0.  greedy[i] (nullable) = argmax of
 * row i.  Bookkeeping is omx_qwen3_verify's: the n tokens run on top of the cache, their K/V rows are appended, the pending input token
 * becomes the last row's argmax (omx_qwen3_trim(m, 0, tok) sets another).  1 <= n <= the prompt buffer, cached + n + 1 <= max_context.
 * The sampler is not consulted.  Refused by name: tensor / expert parallel models (a sharded vocabulary), float16 models, ids and
 * targets out of range.  last_score_ms: device time of the last call's prompt pass and of its head (norm, panels, merge).          */
int omx_qwen3_score(omx_qwen3 m, const uint32_t* tokens, int n, const uint32_t* targets /*[n], OMX_NO_TARGET = none*/,
                    float* logprobs /*[n]*/, uint32_t* greedy /*[n], nullable*/);
int omx_qwen3_last_score_ms(omx_qwen3 m, float* pass_ms, float* head_ms);
/* Batched decode (csrc/engine_batch.hip): up to 8 independent sequences on ONE loaded model.  The reference's Model::forward and KVCache
 * carry a batch dimension ([B, L] ids, [B, Hkv, T, D] cache, mlx-rs-core/src/cache.rs); a batch object is its ragged form: every slot is a
 * sequence with its own K/V slabs, position, pending token and sampler, and one decode step advances any chosen subset of the slots with
 * ONE weight stream per Linear (the rows launches of omx_qwen3_verify).  The model's own sequence (omx_qwen3_prefill / _decode / _verify,
 * its graphs, slabs and state) is untouched and both may be used on the same model -- but a batch shares the model's stream and its
 * prompt-pass scratch: calls on a model and on its batches must be SERIALISED by the caller, and a batch must be destroyed before its model.
 *   create:  n_slots 1..8; max_context 0 = the model's (not above it; rounded up to the 256 step like the model's).  Accepts the models
 *            omx_qwen3_verify accepts: single rank, dense MLP, bf16 weights or packed weights with bf16 scales, and the MODEL's filtered
 *            sampling off (omx_qwen3_set_sampling; create / prefill / fork / decode refuse while it is on -- the slots' filters below are
 *            the batch's own state and never touch the model's).
 *   set_sampler: per slot, the rule of omx_qwen3_set_sampler -- 0 = greedy (default), else categorical(logits / T) with the slot's OWN key
 *            sequence seeded from `seed`.  Turns the slot's filters and penalties off and clears its history.
 *   set_sampling: per slot, the rule of omx_sample_filtered / omx_qwen3_set_sampling (parameter ranges as there): penalties on the ids
 *            in the slot's history, * (1/T), top-k with ties kept, top-p on the survivors, then the draw over the kept set with the NEXT key
 *            of the slot's own sequence (restarted from `seed`); temperature 0 with a penalty = argmax of the penalised logits, without
 *            one the plain argmax.  The history is a byte per vocabulary entry and slot on the device: the tokens the slot SAMPLED since
 *            its last prefill (the prompt excluded), marked by the step itself for slots with a penalty on; cleared by set_sampling,
 *            set_sampler, reset and every prefill (an appending one too).  A step in which no listed slot filters is the plain step,
 *            launch for launch; otherwise every listed row goes through the filtered sampler (a plain slot draws the same token there)
 *            -- one launch for short rows, the launch-per-level selection with one grid row per sequence at vocabulary sizes.  A slot's
 *            tokens do not depend on its neighbours' settings.
 *   prefill: the prompt through the batched prompt pass onto the slot's slabs at the slot's offset (a second prefill appends), then the
 *            first token from the slot's sampler, which becomes the slot's pending token.
 *   decode:  `slots` = 1..n_slots distinct prefilled slots in any order; each advances n_steps (<= 1024) tokens; tokens_out is HOST memory
 *            [n_steps][n_slots], columns in the listed order; slots not listed are untouched.  Every listed slot needs offset + n_steps <=
 *            capacity (checked before anything runs).  The steps are enqueued back to back and the host waits once, at the end: positions,
 *            pending tokens and sampler keys live in device memory.  A sequence's tokens and logits do not depend on which other slots
 *            are listed beside it, nor on their contents.
 *   logits:  bf16 logits [V] of the last prefill or step the slot took part in.   offset: tokens in the slot's cache.
 *   trim:    omx_qwen3_trim per slot: forget the last n cached tokens and make next_token the pending token (n = 0: only the token).
 *            Refused on a slot with a repetition / presence penalty on (a byte history cannot be rewound, as omx_qwen3_trim).
 *   reset:   the slot is empty again (its sampler's key sequence goes on).
 *   fork:    the EMPTY slot dst becomes what it would be had it been fed src's tokens itself: src's position, src's kept logits row, and a
 *            copy of rows [0, position) of src's K/V slabs in dst's own.  resample != 0: dst's pending token is drawn from that row with
 *            dst's own sampler and key sequence (the draw a prefill of the same prompt would have made); 0: it is src's.  *first_token is
 *            that token.  The history: resample = 0 copies src's to dst (the sibling continues src's sequence); resample != 0 starts dst
 *            with an EMPTY one, draws under dst's own settings and marks the token -- right only at the token after the prompt, so it is
 *            refused when dst has a penalty on and src has decoded past its prefill.
 *            Refused: src not prefilled, src == dst, dst not empty (reset it first), a slot out of range.  Siblings share
 *            the whole 256-token chunks below the fork, one level deep (a fork of a fork shares the root's span): the slot table keeps,
 *            per slot, the `owner` whose slabs hold the same bits in rows [0, shared_len), and a decode step MAY read those chunks once per
 *            group of listed rows with the same owner instead of once per row -- to the bit the partials the rows' own slabs give, whatever
 *            the group (OMX_BATCH_SHARE_MIN=2..8: groups from that many rows on; by default none, the grouped block being the slower
 *            one at every size measured).  Every other call works on the slot's own copy; trim / reset / a prefill from position 0 of a slot lower the
 *            shared_len of that slot and of the slots that share with it to the chunk boundary they leave intact.  OMX_BATCH_SHARE=0
 *            (read by create): forks copy, shared_len stays 0, every row reads its own slab.
 *   shared:  owner and shared_len of a slot, from the device's table.
 *   create_kv: create with the K/V storage chosen (MLX's kv_bits).  kv_bits 0 = bf16 slabs, what create makes; 8 = every K row (after
 *            q/k norm and RoPE) and V row stored as MLX affine codes, group 64 along the head dim, scales and biases bf16 -- mlx quantize's
 *            arithmetic on the bf16 row, to the bit -- quantised as the row is appended, and every attention reads (float)code * scale +
 *            bias: the decode step straight from the packed rows, a prompt pass from ONE bf16 staging pair the slot's rows are expanded
 *            into layer by layer (its new rows included, replaced by their dequantised values before the attention).  136 instead of 256
 *            bytes per cached token and KV head at head_dim 128.  Everything else as above; the grouped read of shared chunks is not
 *            built for packed rows (OMX_BATCH_SHARE_MIN is ignored, `shared` reports as before).  Any other kv_bits is refused.
 *   kv_bytes: bytes of K/V storage the batch allocated (the slabs only).
 *   kv_read: HOST copies of rows [first, first + n) (cached rows only) of one slot and layer.  A bf16 batch: k_rows / v_rows bf16
 *            [Hkv, n, D], the four scale / bias pointers null.  A kv_bits 8 batch: k_rows / v_rows MLX-layout uint32 [Hkv, n, D / 4]
 *            (element j of a row = byte j, LSB first), scales and biases bf16 [Hkv, n, D / 64].
 *   debug_attention: test hook, as omx_debug_attn_step -- the decode attention launch alone: row r = the caller's query q[r] ([n, H, D]
 *            bf16, HOST) over ALL rows slot slots[r] holds of `layer`, out [n, H * D] bf16 (HOST).  Prefilled slots only; slot state is
 *            untouched (the model's prompt scratch is used).                                                                           */
typedef struct omx_qwen3_batch_* omx_qwen3_batch;
int omx_qwen3_batch_create(omx_qwen3_batch* out, omx_qwen3 m, int n_slots, int max_context);
int omx_qwen3_batch_create_kv(omx_qwen3_batch* out, omx_qwen3 m, int n_slots, int max_context, int kv_bits);
int omx_qwen3_batch_kv_bytes(omx_qwen3_batch b, size_t* bytes);
int omx_qwen3_batch_kv_read(omx_qwen3_batch b, int slot, int layer, int first, int n, void* k_rows, void* v_rows, void* k_scales,
                            void* k_biases, void* v_scales, void* v_biases);
int omx_qwen3_batch_debug_attention(omx_qwen3_batch b, int layer, const int* slots, int n, const void* q, void* out);
int omx_qwen3_batch_destroy(omx_qwen3_batch b);
int omx_qwen3_batch_set_sampler(omx_qwen3_batch b, int slot, float temperature, uint64_t seed);
int omx_qwen3_batch_set_sampling(omx_qwen3_batch b, int slot, const omx_sampling* p, uint64_t seed);
int omx_qwen3_batch_prefill(omx_qwen3_batch b, int slot, const uint32_t* prompt, int n_prompt, uint32_t* first_token);
/* omx_qwen3_batch_prefill with rows [first_row, first_row + n_rows) of the pass supplied by the caller: omx_qwen3_prefill_embeds' span
 * (DEVICE rows, f32 / bf16 / f16, cast once to nearest even), its refusals and their texts, on the slot's own cache (bf16 or kv_bits = 8).
 * A packed model's prompt of 8 rows or fewer takes the few-row packed launches, which cannot take rows: refused as "InvalidConfig". */
int omx_qwen3_batch_prefill_embeds(omx_qwen3_batch b, int slot, const uint32_t* prompt, int n_prompt, const void* rows, omx_dtype rows_dtype,
                                   int first_row, int n_rows, uint32_t* first_token);
int omx_qwen3_batch_decode(omx_qwen3_batch b, const int* slots, int n_slots, int n_steps, uint32_t* tokens_out);
int omx_qwen3_batch_logits(omx_qwen3_batch b, int slot, void* host_bf16, int n);
int omx_qwen3_batch_offset(omx_qwen3_batch b, int slot, int* offset);
int omx_qwen3_batch_trim(omx_qwen3_batch b, int slot, int n, uint32_t next_token);
int omx_qwen3_batch_reset(omx_qwen3_batch b, int slot);
int omx_qwen3_batch_fork(omx_qwen3_batch b, int src, int dst, int resample, uint32_t* first_token);
int omx_qwen3_batch_shared(omx_qwen3_batch b, int slot, int* owner, int* shared_len);
/* Per-token log-probabilities in the batched step: omx_qwen3_set_logprobs' rule, ONE setting for the batch (top_n -1 = off, the
 * default; 0; 1..min(OMX_LOGPROBS_MAX_TOP, V)).  While on, the step's sampler -- plain or filtered -- is followed by the same two launches
 * over the T rows of the step's logits, the targets being the tokens the sampler just wrote to the token ring; the results are laid out
 * as the token ring is and the host still waits once per call.  The values are those of the raw rows omx_qwen3_batch_logits returns.
 * A row's values do not depend on what runs beside it: a slot's bits are the same alone, among eight and in any order.
 *   decode_logprobs: omx_qwen3_batch_decode + logprobs [n_steps, n_slots] and (nullable) top_ids / top_logprobs [n_steps, n_slots, top_n].
 *   last_logprobs:   of the slot's most recently sampled token: a prefill's or fork's first token, or its last step's.  A
 *                    fork(resample) sibling has its OWN drawn token's value over the source's kept row; fork(resample = 0) copies the
 *                    source's.  Refused while off, and on a slot that has sampled nothing since set_logprobs.                   */
int omx_qwen3_batch_set_logprobs(omx_qwen3_batch b, int top_n);
int omx_qwen3_batch_decode_logprobs(omx_qwen3_batch b, const int* slots, int n_slots, int n_steps, uint32_t* tokens_out,
                                    float* logprobs /*[n_steps, n_slots]*/, uint32_t* top_ids /*[n_steps, n_slots, top_n], nullable*/,
                                    float* top_logprobs /*nullable*/);
int omx_qwen3_batch_last_logprobs(omx_qwen3_batch b, int slot, float* logprob, uint32_t* top_ids /*nullable*/, float* top_logprobs /*nullable*/);
/* device time of the steps of the last omx_qwen3_batch_decode call (HIP events on the model's stream), ms */
int omx_qwen3_batch_last_decode_ms(omx_qwen3_batch b, float* ms);
/* measurement hook (csrc/per_op_route.hip): qwen3-mlx's Model::forward + Generate::next replayed call for call through the mlx-c handle ABI
 * on this engine's weights (borrowed) -- what an UNMODIFIED crate gets.  tokens_out [n_new + 1]: the token sampled from the prompt, then n_new
 * greedy tokens; host wall-clock per decoded token and mlx_* calls per token. */
int omx_bench_qwen3_per_op(omx_qwen3 model, const omx_qwen3_config* cfg, const uint32_t* prompt, int n_prompt, int n_new,
                           uint32_t* tokens_out, double* prefill_ms, double* ms_per_token, double* calls_per_token);
/* timing of the last omx_qwen3_decode call measured with HIP events on the engine stream (ms)       */
int omx_qwen3_last_decode_ms(omx_qwen3 m, float* ms);
int omx_qwen3_last_prefill_ms(omx_qwen3 m, float* ms);   /* same for the last omx_qwen3_prefill call */
/* bytes the engine holds for dequantised weights of a packed model: the prompt pass's dequant cache slab plus its scratch (the
 * verify pass adds none) */
int omx_qwen3_dequant_bytes(omx_qwen3 m, size_t* bytes);
/* test hook: copy an internal bf16 buffer ("h","h2","qkv","attn_out","act","k<l>","v<l>") to the host */
int omx_qwen3_debug_read(omx_qwen3 m, const char* name, void* host, size_t n_elems);
/* test hook: the other way, n_elems 16-bit patterns from the host into the same buffers (the caller keeps n_elems inside the buffer) */
int omx_qwen3_debug_write(omx_qwen3 m, const char* name, const void* host, size_t n_elems);
/* test hook of the dense decode GEMV (csrc/gemv.hip): ONE launch with prologue `pro` (0 none, 1 RMSNorm) and epilogue `epi` (0 store
 * [+ bias], 1 residual, 2 SwiGLU over gate w0 / up w1, 3 logits + argmax partials), bf16 (f16 = 0) or float16 (f16 = 1) operands.
 * w0 | w1 | w2 are row-stacked ([n0 | n1 | rest] rows of K) for the other epilogues.  argmax_slot: omx_debug_gemv_grid(N, K) keys. */
int omx_debug_gemv(void* out, unsigned long long* argmax_slot, const void* x, const void* norm_w, const void* resid, const void* bias,
                   const void* w0, const void* w1, const void* w2, int n0, int n1, int N, int K, int pro, int epi, int f16, float eps,
                   int single_round, omx_stream stream);
int omx_debug_gemv_grid(int N, int K);
/* test hook of the dense decode GEMV, every field of a plain or batched launch (no routing prologue, no peer output).  In: the fields
 * of omx_debug_gemv plus rows_per_wave (0: the tuned choice), row_offset (EPI_ARGMAX), x_partial [x_partial_n][K] f32 with x_out,
 * out_scale (EPI_F32, [n_batch] bf16), the batch fields (n_batch, x_div, x_bstride elements, out_bstride_bytes, w_sel [n_batch]
 * expert ids, w_estride elements, w_sel_lo / w_sel_n) and argmax_slot_n (capacity of argmax_slot; a launch needing more blocks is
 * refused).  Out: the route launch_gemv takes (nv: tuned width class K/512 or 0 for the generic kernel, ksplit waves per row, tail:
 * masked last vectors), the resolved rows_per_wave and the blocks along x (= argmax partials written).  dry_run != 0: only the route,
 * nothing is launched (no device needed).  Synchronises the stream. */
typedef struct omx_gemv_ex_ {
    void* out; unsigned long long* argmax_slot; int argmax_slot_n;
    const void* x; const void* norm_w; const void* resid; const void* bias;
    const void* w0; const void* w1; const void* w2; int n0, n1, N, K, pro, epi, f16; float eps; int single_round;
    int rows_per_wave, row_offset;
    const float* x_partial; int x_partial_n; void* x_out; const void* out_scale;
    int n_batch, x_div; long long x_bstride, out_bstride_bytes; const unsigned* w_sel; long long w_estride; int w_sel_lo, w_sel_n;
    int dry_run;
    int route_nv, route_ksplit, route_tail, route_rows_per_wave, route_blocks;   /* out */
} omx_gemv_ex;
int omx_debug_gemv_ex(omx_gemv_ex* a, omx_stream stream);
/* test hook of the packed decode GEMV (csrc/quant.hip, qgemv_mfma.hip): ONE launch_qgemv with every field the engines set.
 * In: up to three members m[0 .. 2] (n == 0 ends the list; bits / group 0: the launch's) -- a row stack (N = sum of n), or gate m[0] /
 * up m[1] of N rows each for epi 2; N, K, group, bits, pro (0 none, 1 RMSNorm), epi (0 store, 1 residual, 2 SwiGLU, 3 logits + argmax
 * partials, 4 f32 row sums), eps, single_round; scales_f16 (float16 triplets: x, norm_w, resid and out are float16 too); use_sb: build
 * the interleaved scale | bias words first, for any K; use_tiles: build the matrix-core tiles where the shape has them; mfma: the
 * matrix-core mode of this call (0 never), restored afterwards; row_offset, rolled_stage; the batch fields n_batch, x_div, w_sel
 * [n_batch] expert ids, w_estride words / s_estride groups between experts, w_sel_lo / w_sel_n, n_experts (matrices per member's stack,
 * for use_sb; 0 = 1); x, norm_w, resid; out [n_batch, N], out_f32 (epi 4), argmax_slot with its capacity argmax_slot_n (a launch that
 * needs more is refused on the host).  Out, the route the launchers report: route_kernel (1 the VALU kernel on one format, 2 the
 * mixed-format stack kernel, 3 the matrix-core kernel), its BITS / W / RB (stack: 0 / 0 / RB), the resolved rows_per_wave, SB, F16S,
 * blocks along x, dynamic LDS bytes and, on the matrix cores, KS / NU / NBUF.  dry_run != 0: only the route (no device needed, no
 * pointer read).  Synchronises the stream. */
typedef struct omx_qgemv_member_ { const void* w; const void* scales; const void* biases; int n, bits, group; } omx_qgemv_member;
typedef struct omx_qgemv_ex_ {
    omx_qgemv_member m[3];
    int N, K, group, bits, pro, epi; float eps; int single_round;
    int scales_f16, use_sb, use_tiles, mfma, row_offset, rolled_stage;
    int n_batch, x_div; const unsigned* w_sel; long long w_estride, s_estride; int w_sel_lo, w_sel_n, n_experts;
    const void* x; const void* norm_w; const void* resid;
    void* out; float* out_f32; unsigned long long* argmax_slot; int argmax_slot_n;
    int dry_run;
    int route_kernel, route_bits, route_w, route_rb, route_rows_per_wave, route_sb, route_f16s, route_blocks, route_lds_bytes,
        route_ks, route_nu, route_nbuf;   /* out */
} omx_qgemv_ex;
int omx_debug_qgemv_ex(omx_qgemv_ex* a, omx_stream stream);
/* test hook of the step attention (csrc/attn_step.hip): ONE launch_attn_step on caller-owned buffers, without the O projection.
 * qkv [H*D | Hkv*D | Hkv*D] raw, K / V slabs [Hkv, cap, D], q/k norm weights [D] (both null: no q/k norm), rope_cur [D] f32
 * cos | sin of `pos`, granules [granules_n] (kept by the caller: leftovers of earlier calls stay, as in the engine), tag
 * seq * tag_mul + tag_add.  Split plan: chunk / nsplit when both > 0, else attn_step_plan(tk_max) (the engine's rule); refused on the
 * host when it does not cover pos + 1, when pos >= cap or when the granules do not fit.  Out: out [H*D], the plan used, abort_flag.
 * Synchronises the stream. */
typedef struct omx_attn_step_dbg_ {
    const void* qkv; void* k; void* v; int H, Hkv, D, cap; float scale, eps;
    const void* q_norm_w; const void* k_norm_w; const float* rope_cur;
    void* granules; long long granules_n;
    int pos; unsigned seq, tag_mul, tag_add; int f16;
    int chunk, nsplit, tk_max;   /* in: plan (or tk_max); out: the plan used */
    void* out; unsigned abort_flag;   /* out */
} omx_attn_step_dbg;
int omx_debug_attn_step(omx_attn_step_dbg* a, omx_stream stream);
/* test hook of the few-row bf16 Linear (csrc/gemv_rows.hip): ONE launch over M <= 8 activation rows x [M, K] on caller-owned buffers,
 * straight through launch_gemv_rows (segmented == 0) or launch_gemv_rows_segmented -- no N * K routing threshold in between.
 * Plain: out [M, N] = x . w[N, K]^T (+ bias [N]) (relu) then + resid [M, N] (the product rounded first), or resid + product * gate [N].
 * Segmented: n_plain <= 3 Linears {w [cols, K], bias [cols] or null, out [M, cols] with row stride ld}, then a SwiGLU pair w_gate /
 * w_up [half, K] -> out_act [M, half] with row stride ld_act (act_mode 0: one rounding, 1: every primitive rounded); pre_norm_w [K]:
 * RMSNorm of the rows inside the launch (M <= 4, K <= 4096).  Out: route_rpw, the output rows per wave (2 or 4) of the launch.  The
 * launcher's refusals come back as its error text; nothing is launched then.  Synchronises the stream. */
typedef struct omx_gemv_rows_seg_ { const void* w; const void* bias; void* out; int cols, ld; } omx_gemv_rows_seg;
typedef struct omx_gemv_rows_dbg_ {
    const void* x; int M, K, segmented;
    const void* w; const void* bias; const void* resid; const void* gate; int relu, N; void* out;   /* plain */
    omx_gemv_rows_seg seg[3]; int n_plain;                                                           /* segmented */
    const void* w_gate; const void* w_up; void* out_act; int half, ld_act, act_mode;
    const void* pre_norm_w; float pre_norm_eps;
    int route_rpw;   /* out */
} omx_gemv_rows_dbg;
int omx_debug_gemv_rows(omx_gemv_rows_dbg* a, omx_stream stream);
int omx_qwen3_stream(omx_qwen3 m, omx_stream* s);
/* algorithmic HBM bytes of ONE decode step at context length ctx (SURVEY.md 8d formula)             */
int omx_qwen3_step_bytes(omx_qwen3 m, int ctx, double* bytes);
/* how the decode step is executed once built: 0 = not built yet, 1 = step graph (one launch per phase,
 * replayed as a hipGraph; one graph per 1024-token context bucket), 2 = the same launches issued eagerly, 3 = AQL replay on the
 * engine's own queue; bits 8..11: the rungs of the give-up ladder this engine has gone down (gate/up out of the attention launch,
 * down + q/k/v as two launches, persistent step off, O projection out of the attention launch) */
int omx_qwen3_decode_path(omx_qwen3 m, int* path);
/* debug hook (tools/attn_step_trace.py): run ONE decode step eagerly with the attention launches stamping the
 * 100 MHz wall clock; host receives [layers][attention splits][kv heads][16] (word 10 of a block whose launch carries gate/up is
 * a count, the (gate, up) pairs its waves reduced: 48), *blocks = splits * kv heads     */
int omx_qwen3_debug_trace_step(omx_qwen3 m, unsigned long long* host, size_t n_words, int* blocks);
/* measurement hook: `steps` real decode steps run eagerly, every launch of the per-layer kernels carrying its own HIP event pair
 * (the dispatch's begin / end timestamps on the step's stream); us[7] = average microseconds of {QKV GEMV, attention, O GEMV,
 * gate/up + SwiGLU GEMV, down GEMV, lm_head, persistent step launch (all layers; the five per-layer figures are 0 then)}.  bench.py's roofline.achieved is the gate/up figure.  Dense bf16 single-rank models.
 * Where down and the next layer's q/k/v are one launch (csrc/gemv_chain.hip), its duration is split between the down and the QKV figure in
 * proportion to their algorithmic bytes; where gate/up + SwiGLU rides in the attention launch (csrc/attn_step.hip), that launch's duration
 * is split the same way between the attention and the gate/up figure. */
int omx_qwen3_time_step_kernels(omx_qwen3 m, int steps, float* us);
/* debug hook (tools/step_engine_trace.py): ONE eager decode step on the persistent engine (csrc/step_engine.hip, OMX_STEP_ENGINE=1)
 * with per-CU wall-clock stamps; host receives [CUs][64] words, *cus = CUs of the device */
int omx_qwen3_debug_trace_engine(omx_qwen3 m, unsigned long long* host, size_t n_words, int* cus);
/* test hooks of the decode step's forms.  step_forms: what the NEXT step would take -- forms[0] = down + the next layer's q/k/v in one
 * launch (csrc/gemv_chain.hip, OMX_DOWN_QKV=0 turns it off), forms[1] = the O projection inside the attention launch, forms[2] = the
 * persistent-step mode, forms[3] = 1 once a give-up switched the first off for this engine, forms[4] = gate/up + SwiGLU inside the
 * attention launch (OMX_ATTN_GATEUP=0 turns it off), forms[5] = 1 once a give-up switched that off, forms[6] = down + the next layer's q/k/v
 * inside the attention launch as well, one launch per layer (OMX_ATTN_DOWN=0 turns it off; forms holds seven ints).  raise_give_up: sets, from the host, the word
 * a wait inside a launch raises when it gives up; the next omx_qwen3_decode then replays its steps on the next form of the ladder */
int omx_qwen3_debug_step_forms(omx_qwen3 m, int* forms);
int omx_qwen3_debug_raise_give_up(omx_qwen3 m);

/* =====================================================================================
 * MLX affine group quantisation (the reference's flagship checkpoint format).
 * mlx_rs::ops::{quantize, dequantize, quantized_matmul, gather_qmm} (mlx-rs/src/ops/quantization.rs:41-153,
 * 226-279) -> mlx_quantize / mlx_dequantize / mlx_quantized_matmul / mlx_gather_qmm (mlx-c ops.h:356-365,
 * 471-484, 793-810).  w [rows, cols] <-> packed u32 [rows, cols*bits/32] (LSB first) + scales, biases
 * [rows, cols/group_size] (dtype of w); group_size 32/64/128.  quantize / dequantize: bits 2, 4 or 8 on bf16 / f16 / f32 (the
 * reference's own value test loops [2, 4, 8] on f32, quantization.rs:289-305).  The matmuls: bits 4 or 8; dtype = the dtype of x,
 * out, scales and biases alike -- bf16, or f16 for a float16 MLX checkpoint, which then runs in float16 END TO END like in MLX
 * (nn/quantized.rs:361-385): float16 activations, float16 rounding points, f32 accumulation.
 * ===================================================================================== */
int omx_quantize(void* packed, void* scales, void* biases, const void* w, int64_t rows, int cols, int group_size, int bits,
                 omx_dtype dtype, omx_stream stream);
int omx_dequantize(void* out, const void* packed, const void* scales, const void* biases /* may be NULL */, int64_t rows,
                   int cols, int group_size, int bits, omx_dtype dtype, omx_stream stream);
/* out [M, N] = x [M, K] . dequant(W [N, K])^T (transpose = true, nn::QuantizedLinear::forward quantized.rs:366-375):
 * M <= 16 streams the packed weights (GEMV), larger M dequantises into the library workspace and runs the MFMA GEMM */
int omx_quantized_matmul(void* out, const void* x, const void* packed, const void* scales, const void* biases, int M, int N,
                         int K, int group_size, int bits, omx_dtype dtype, omx_stream stream);
/* the compute-bound quantized Linear (qgemm.hip): out [M, N] = x [M, K] . dequant(W)^T with W dequantised INSIDE the matrix-core
 * kernel (no bf16 copy of W); bf16 x / out / scales / biases, bits 4 or 8, group 32 / 64 / 128, K % 64 == 0, any M >= 1.  Each output
 * equals omx_dequantize followed by the 16x16x32 bf16 GEMM (omx_linear with OMX_GEMM_TILE=256 OMX_GEMM_MFMA=16) bit for bit.
 * resid == gate == NULL: plain; both set: out = bf16(resid + acc * gate[col]) (the DiT's gated residual, klein_model.rs:909-925) */
int omx_quantized_linear_mfma(void* out, const void* x, const void* packed, const void* scales, const void* biases, const void* resid,
                              const void* gate, int M, int N, int K, int group_size, int bits, omx_stream stream);
/* omx_linear_swiglu on packed weights: W = [n_plain | half gate | half up] rows; same width rules (n_plain % 4, half % 4, K % 64) */
int omx_quantized_linear_swiglu(void* out_plain, void* out_act, const void* x, const void* packed, const void* scales, const void* biases,
                                int M, int n_plain, int half, int K, int group_size, int bits, omx_stream stream);
/* out [n_rows, N]: row i = x[i / x_div] . dequant(W[rhs_indices[i]])^T over expert-stacked packed weights
 * [n_experts, N, K*bits/32] (QuantizedSwitchLinear::apply, mixtral-mlx/src/model.rs:195-201)                */
int omx_gather_qmm(void* out, const void* x, const void* packed, const void* scales, const void* biases,
                   const uint32_t* rhs_indices, int n_rows, int x_div, int N, int K, int n_experts, int group_size, int bits,
                   omx_dtype dtype, omx_stream stream);

/* dense sibling (mlx_gather_mm, ops.h:463; mlx-rs/src/ops/quantization.rs:169-203): out [n_rows, N], row i = x[i / x_div] . W[rhs_indices[i]]^T
 * over expert-stacked bf16 weights [n_experts, N, K]; expert-selected batched GEMV, K a multiple of 8                      */
int omx_gather_mm(void* out, const void* x, const void* w, const uint32_t* rhs_indices, int n_rows, int x_div, int N, int K,
                  int n_experts, omx_dtype dtype, omx_stream stream);

/* =====================================================================================
 * a6 + a7: sparse-MoE block = router + top-k + SwitchGLU + weighted sum.
 *   mode 0  MixtralSparseMoeBlock::forward (mixtral-mlx/src/model.rs:296-308): top-k of the gate logits,
 *           softmax (precise) over the SELECTED logits;
 *   mode 1  MoeBlock::forward of Qwen3-MoE (qwen3-mlx/src/qwen3_moe.rs:475-503): softmax over all experts,
 *           top-k, scores renormalised when norm_topk_prob.
 *   experts SwitchGLU::forward_experts (model.rs:243-274) = mlx_gather_qmm x3 (ops.h:471-484) + fused_swiglu;
 *           here with dense bf16 stacked weights w_gate/w_up [E, inter, hidden], w_down [E, hidden, inter]
 *           (mlx_gather_mm form, ops.h:463-470).
 * x [n_tokens, hidden] -> out [n_tokens, hidden]; inds_out [n_tokens, top_k] u32 and scores_out
 * [n_tokens, top_k] bf16 are optional device outputs (descending score order).  Scratch comes from the
 * library workspace (omx_moe_workspace_bytes tells how much; omx_set_workspace to provide it).
 * ===================================================================================== */
int omx_moe_workspace_bytes(int n_tokens, int hidden, int inter, int n_experts, int top_k, size_t* bytes);
int omx_moe_forward(void* out, const void* x, const void* gate_w, const void* w_gate, const void* w_up,
                    const void* w_down, int n_tokens, int hidden, int inter, int n_experts, int top_k, int mode,
                    int norm_topk_prob, uint32_t* inds_out, void* scores_out, omx_stream stream);
/* decoder-block form (mixtral model.rs:340-345, qwen3_moe.rs decoder layer): out = resid + moe(rmsnorm(x, norm_w, eps));
 * the norm is folded into the router launch, the residual into the combine launch; xn = [n_tokens, hidden] scratch */
int omx_moe_block_forward(void* out, const void* resid, const void* x, const void* norm_w, float eps, void* xn, const void* gate_w,
                          const void* w_gate, const void* w_up, const void* w_down, int n_tokens, int hidden, int inter,
                          int n_experts, int top_k, int mode, int norm_topk_prob, omx_stream stream);
/* expert-parallel decode form: this rank holds experts [e_lo, e_lo + e_n) (w_* = its stacks);
 * partial [n_tokens, hidden] f32 = its share of sum_j bf16(y_j * score_j), to be all-reduced over the ranks; the residual
 * h + bf16(sum) is the caller's.  n_tokens * top_k <= 32. */
/* tables of the batched expert-parallel block for an exchange-based combine (omx_moe_block_slots_ep -> omx_peer_moe_combine) */
typedef struct omx_moe_ep_slots_ {
    const void* y;                 /* [local slots (sorted by local expert), hidden] bf16 expert outputs */
    const uint32_t* pos_of_slot;   /* [n_tokens * top_k] slot -> row of y (slots of other ranks' experts: unused) */
    const uint32_t* inds;          /* [n_tokens * top_k] global expert id per slot */
    const void* scores;            /* [n_tokens * top_k] bf16 routing weights */
} omx_moe_ep_slots;
int omx_moe_block_partial_ep(float* partial, const void* x, const void* norm_w, float eps, void* xn, const void* gate_w,
                             const void* w_gate, const void* w_up, const void* w_down, int n_tokens, int hidden, int inter,
                             int n_experts, int top_k, int mode, int norm_topk_prob, int e_lo, int e_n, omx_stream stream);
/* the two sharded forms on MLX-packed expert stacks (the reference's own Mixtral format: mixtral-mlx/src/model.rs:466-615): this rank's packed
 * experts / columns -- the triplet of a slice is the slice of the triplet; bf16 scales.  Contracts of omx_moe_block_partial_ep / _tp. */
int omx_moe_block_partial_ep_q(float* partial, const void* x, const void* norm_w, float eps, void* xn, const void* q_router, const void* s_router,
                               const void* b_router, const void* q_gate, const void* s_gate, const void* b_gate, const void* q_up,
                               const void* s_up, const void* b_up, const void* q_down, const void* s_down, const void* b_down, int n_tokens,
                               int hidden, int inter, int n_experts, int top_k, int mode, int norm_topk_prob, int e_lo, int e_n, int group_size,
                               int bits, int f16, omx_stream stream);
int omx_moe_block_partial_tp_q(float* y_partial, uint32_t* route_inds, void* route_scores, const void* x, const void* norm_w, float eps,
                               const void* q_router, const void* s_router, const void* b_router, const void* q_gate, const void* s_gate,
                               const void* b_gate, const void* q_up, const void* s_up, const void* b_up, const void* q_down, const void* s_down,
                               const void* b_down, int n_tokens, int hidden, int inter, int n_experts, int top_k, int mode, int norm_topk_prob,
                               int group_size, int bits, int f16, omx_stream stream);
int omx_moe_block_slots_ep(omx_moe_ep_slots* out, const void* x /* normalised rows */, const void* gate_w, const void* w_gate, const void* w_up,
                           const void* w_down, int n_tokens, int hidden, int inter, int n_experts, int top_k, int mode, int norm_topk_prob,
                           int e_lo, int e_n, omx_stream stream);
/* expert TENSOR parallel decode form (<= 32 routed slots): this rank holds `inter` = I / tp intermediate columns of EVERY expert;
 * y_partial [slots, hidden] f32 = the unrounded partial down projections (to be all-reduced), the replicated router's choice goes to
 * route_inds / route_scores; omx_moe_combine_slots then forms bf16(resid + bf16(sum_j bf16(bf16(y_j) score_j))) (mixtral model.rs:296-308,
 * 343-344 with the single-device roundings).  No reference counterpart: mlx-c distributed.h:30-70 is declared, never bound. */
int omx_moe_block_partial_tp(float* y_partial, uint32_t* route_inds, void* route_scores, const void* x, const void* norm_w, float eps,
                             void* xn, const void* gate_w, const void* w_gate, const void* w_up, const void* w_down, int n_tokens,
                             int hidden, int inter, int n_experts, int top_k, int mode, int norm_topk_prob, omx_stream stream);
int omx_moe_combine_slots(void* out, const float* y_slots, const void* scores, const void* resid, int n_tokens, int hidden, int top_k,
                          omx_stream stream);
/* f16 != 0 (also the last int of the two packed-stack entry points above): a float16 checkpoint -- activations, scores, residual and every
 * rounding point float16 (nn/quantized.rs:361-385: the dequantised weight has the scales' dtype), f32 accumulation; decode form only */
int omx_moe_combine_slots_ex(void* out, const float* y_slots, const void* scores, const void* resid, int n_tokens, int hidden, int top_k,
                             int f16, omx_stream stream);
/* the same on a quantised checkpoint (mixtral-mlx/src/model.rs:560-600): router and expert stacks as MLX triplets */
/* one token, bf16 experts: the block WITHOUT its weighted sum -- partials[j, :] (f32) = bf16(bf16(y_j) * score_j) of the top_k routed
 * experts in slot order; the caller's next streaming GEMV folds x := bf16(resid + bf16(sum_j partials[j])) in its prologue (engine-internal:
 * csrc/gemv.hpp GemvArgs::x_partial_n).  Returns 2 when the shape does not take the batched-GEMV route.                              */
int omx_moe_block_partials(float* partials, const void* x, const void* norm_w, float eps, void* xn, const void* gate_w, const void* w_gate,
                           const void* w_up, const void* w_down, int hidden, int inter, int n_experts, int top_k, int mode,
                           int norm_topk_prob, omx_stream stream);
int omx_moe_block_forward_q(void* out, const void* resid, const void* x, const void* norm_w, float eps, void* xn,
                            const void* q_router, const void* s_router, const void* b_router, const void* q_gate, const void* s_gate,
                            const void* b_gate, const void* q_up, const void* s_up, const void* b_up, const void* q_down,
                            const void* s_down, const void* b_down, int n_tokens, int hidden, int inter, int n_experts, int top_k,
                            int mode, int norm_topk_prob, int group_size, int bits, omx_stream stream);
int omx_moe_block_forward_q_ex(void* out, const void* resid, const void* x, const void* norm_w, float eps, void* xn,
                            const void* q_router, const void* s_router, const void* b_router, const void* q_gate, const void* s_gate,
                            const void* b_gate, const void* q_up, const void* s_up, const void* b_up, const void* q_down,
                            const void* s_down, const void* b_down, int n_tokens, int hidden, int inter, int n_experts, int top_k,
                            int mode, int norm_topk_prob, int group_size, int bits, int f16 /* float16 checkpoint: x, norm weights, triplets and out are float16; <= 32 routed slots */, omx_stream stream);
/* the reference's own Mixtral format (mixtral-mlx/src/model.rs:182-274, QuantizedSwitchLinear -> mlx_gather_qmm x3):
 * expert stacks as MLX affine-quantised triplets, packed u32 [E, out, in*bits/32], scales / biases [E, out, in/group_size];
 * router gate bf16.  <= 32 routed slots: expert-selected GEMVs on the packed weights; more: dequantise + grouped GEMM. */
int omx_moe_forward_q(void* out, const void* x, const void* gate_w, const void* q_gate, const void* s_gate, const void* b_gate,
                      const void* q_up, const void* s_up, const void* b_up, const void* q_down, const void* s_down,
                      const void* b_down, int n_tokens, int hidden, int inter, int n_experts, int top_k, int mode,
                      int norm_topk_prob, int group_size, int bits, uint32_t* inds_out, void* scores_out, omx_stream stream);
/* The same block as three stages, for an expert-parallel host that exchanges token rows between them
 * (all-to-all dispatch + combine; ominix-mlx_amd/ep.py):
 *   route    x [n, hidden] -> inds [n, k] u32, scores [n, k] (dtype of x)            (model.rs:296-302)
 *   experts  rows [m, hidden] that already carry their (local) expert id -> y [m, hidden]
 *            = down_e(fused_swiglu(up_e x, gate_e x))                                 (model.rs:243-274)
 *   combine  y [n, k, hidden], scores [n, k] -> out [n, hidden]                      (model.rs:304-307) */
int omx_moe_route(uint32_t* inds_out, void* scores_out, const void* x, const void* gate_w, int n_tokens, int hidden,
                  int n_experts, int top_k, int mode, int norm_topk_prob, omx_stream stream);
int omx_moe_experts(void* y, const void* x_rows, const uint32_t* expert_ids, int n_rows, const void* w_gate,
                    const void* w_up, const void* w_down, int hidden, int inter, int n_experts, omx_stream stream);
int omx_moe_combine(void* out, const void* y_slots, const void* scores, int n_tokens, int hidden, int top_k,
                    omx_stream stream);

/* DeepSeek-V2 family block (deepseek-ocr2-mlx/src/lib.rs:162-299 MoEGate::route + MoE::forward): routed experts plus shared experts
 * under a third routing arithmetic ("mode 2") -- float32 gate logits (nothing rounded to bf16), softmax over all experts, top-k
 * (descending, ties to the lower index), division by (sum + 1e-20) where norm_topk_prob && top_k > 1, then routed_scaling_factor; the
 * weights stay float32.  out = bf16( bf16(sum_j f32(bf16 y_j) * w_j) + bf16(shared_experts(x)) ).
 *   w_gate / w_up [n_experts + stack_tail, inter, hidden], w_down [n_experts + stack_tail, hidden, inter], bf16: the routed experts and,
 *     where stack_tail == n_shared, the shared MLP behind them as n_shared pseudo-experts of width inter (gate / up: its row blocks,
 *     down: its column blocks).  A token is then top_k + n_shared slots of the expert-selected GEMVs: four launches per block.
 *   sh_gate / sh_up [n_shared * inter, hidden], sh_down [hidden, n_shared * inter] (optional): the shared MLP whole, for more rows than
 *     32 slots hold (n_tokens * (top_k + n_shared) > 32) and for OMX_MOE_SHARED_SLOTS=0.
 * omx_moe_deepseek_form names the launch sequence a call takes: 0 slots, 1 separate GEMVs, 2 grouped GEMMs, -1 none (weights missing).
 * inds_out [n_tokens, top_k] u32 and weights_out [n_tokens, top_k] float32 are optional. */
int omx_moe_deepseek_form(int n_tokens, int hidden, int inter, int top_k, int n_shared, int stack_tail, int have_separate);
int omx_moe_deepseek_workspace_bytes(int n_tokens, int hidden, int inter, int n_experts, int top_k, int n_shared, size_t* bytes);
int omx_moe_deepseek_forward(void* out, const void* x, const void* gate_w, const void* w_gate, const void* w_up, const void* w_down,
                             int stack_tail, const void* sh_gate, const void* sh_up, const void* sh_down, int n_tokens, int hidden,
                             int inter, int n_experts, int top_k, int n_shared, int norm_topk_prob, float routed_scaling_factor,
                             uint32_t* inds_out, float* weights_out, omx_stream stream);
/* decoder-block form: out = resid + block(rmsnorm(x) * norm_w); xn [n_tokens, hidden] receives the normalised rows */
int omx_moe_deepseek_block_forward(void* out, const void* resid, const void* x, const void* norm_w, float eps, void* xn,
                                   const void* gate_w, const void* w_gate, const void* w_up, const void* w_down, int stack_tail,
                                   const void* sh_gate, const void* sh_up, const void* sh_down, int n_tokens, int hidden, int inter,
                                   int n_experts, int top_k, int n_shared, int norm_topk_prob, float routed_scaling_factor,
                                   omx_stream stream);
/* the mode-2 router alone (norm_w optional: the block's RMSNorm folded in, rows left in xn) */
int omx_moe_route_deepseek(uint32_t* inds_out, float* weights_out, const void* x, const void* gate_w, const void* norm_w, float eps,
                           void* xn, int n_tokens, int hidden, int n_experts, int top_k, int norm_topk_prob,
                           float routed_scaling_factor, omx_stream stream);

/* =====================================================================================
 * a14 (+ a9): FLUX.2-klein DiT / MMDiT forward -- FluxKlein::forward_with_rope
 * (flux-klein-mlx/src/klein_model.rs:799-854) with KleinDoubleBlock::forward (:399-522) and
 * KleinSingleBlock::forward (:603-674) as fused launch sequences.  Weights are registered under the
 * reference's internal names (double_blocks.{i}.img_to_q.weight, single_blocks.{i}.to_qkv_mlp.weight,
 * x_embedder.weight, ...; flux-klein-mlx/src/weights.rs:479-596), bf16, [out, in].
 * ===================================================================================== */
typedef struct omx_klein_config_ {   /* FluxKleinParams, klein_model.rs:166-196 */
    int in_channels, hidden_size, txt_embed_dim, num_heads, depth, depth_single, head_dim, mlp_hidden;
    int tp_rank, tp_size;   /* tensor parallel over one node (0/0 or 0/1 = single GPU): heads and MLP width sharded */
} omx_klein_config;
typedef struct omx_klein_* omx_klein;
int omx_klein_create(omx_klein* out, const omx_klein_config* cfg);
int omx_klein_destroy(omx_klein m);
/* `nbytes`: length of the tensor behind `ptr`; every use checks it against the rows x columns it is about to read */
int omx_klein_set_weight(omx_klein m, const char* name, const void* ptr, size_t nbytes);
int omx_klein_synth_weights(omx_klein m, uint32_t base_seed);   /* under TP: this rank's shards of the same logical tensors */
/* quantized DiT (flux-klein-mlx/src/klein_quantized.rs): a Linear's weight as an MLX packed triplet -- packed u32 [rows, cols*bits/32],
 * bf16 scales / biases [rows, cols/group_size] -- under the `.weight` name omx_klein_set_weight takes (the caller keeps the memory).
 * bits 4 / 8, group 32 / 64 / 128, cols % group_size == 0; tp_size 1 only.  A model may mix bf16 and packed Linears. */
int omx_klein_set_quantized_weight(omx_klein m, const char* name, const void* packed, const void* scales, const void* biases, int rows,
                                   int cols, int group_size, int bits);
/* QuantizedFluxKlein::from_unquantized (klein_quantized.rs:498): every bf16 Linear weight registered so far becomes a model-owned
 * packed triplet (omx_quantize); the norms stay bf16.  The forward never reads the bf16 Linear pointers again; synthetic ones are freed. */
int omx_klein_quantize(omx_klein m, int group_size, int bits);
int omx_klein_weight_bytes(omx_klein m, size_t* bytes);   /* device bytes of the tensors the forward reads */
/* comm: ncclComm_t, allreduce_fn: address of ncclAllReduce (RCCL); one bf16 all-reduce after every row-split
 * projection (2 per double-block stream, 1 per single block) */
int omx_klein_set_comm(omx_klein m, void* comm, void* allreduce_fn);
/* latent [s_img, in_channels], txt_embed [s_txt, txt_embed_dim] (device bf16); timestep = t * 1000
 * (generate_klein.rs:434); rope_cos/rope_sin [s_txt + s_img, 128] device f32 with duplicated pair entries,
 * text rows first (compute_rope_freqs, klein_model.rs:53-110); out [s_img, in_channels] device bf16.      */
int omx_klein_forward_with_rope(omx_klein m, void* out, const void* latent, const void* txt_embed, int s_img, int s_txt,
                                float timestep, const float* rope_cos, const float* rope_sin);
/* ---- FLUX VAE decoder: flux-klein-mlx/src/autoencoder.rs Decoder::forward :375-412 with
 *      ResnetBlock :139-157, AttnBlock :195-232, GroupNorm(32, eps 1e-5, pytorch compatible).  NHWC bf16.
 *      Weights (bf16, device) under the names weights.rs:164-217 produces: conv_in.{weight,bias},
 *      mid_block_resnets_{0,1}.{norm1,conv1,norm2,conv2}.*, mid_block_attentions_0.{group_norm,to_q,to_k,to_v,to_out}.*,
 *      up_blocks.{b}.resnets.{j}.{norm1,conv1,norm2,conv2,conv_shortcut}.*, up_blocks.{b}.upsamplers_0_conv.*,
 *      conv_norm_out.*, conv_out.*, post_quant_conv.*; Conv2d weight [out, kH, kW, in], Linear [out, in].
 *      latent [h, w, z_channels] -> image [h*2^(n_mult-1), w*2^(n_mult-1), out_ch] in [-1, 1].                  ---- */
typedef struct omx_vae_config_ {     /* AutoEncoderConfig, autoencoder.rs:22-81 (flux2(): ch 128, mult 1,2,4,4, z 32) */
    int ch, ch_mult[8], n_mult, num_res_blocks, z_channels, out_ch;
    float scale_factor, shift_factor;
} omx_vae_config;
typedef struct omx_vae_decoder_* omx_vae_decoder;
int omx_vae_decoder_create(omx_vae_decoder* out, const omx_vae_config* cfg);
int omx_vae_decoder_destroy(omx_vae_decoder m);
int omx_vae_decoder_set_weight(omx_vae_decoder m, const char* name, const void* ptr);
int omx_vae_decoder_out_shape(omx_vae_decoder m, int h, int w, int* out_h, int* out_w, int* out_c);
int omx_vae_decode(omx_vae_decoder m, void* image, const void* latent, int h, int w);
int omx_vae_decoder_last_ms(omx_vae_decoder m, float* ms);

/* one Euler step of the rectified-flow sampler (flux-klein-mlx/examples/generate_klein.rs:441-443, src/sampler.rs:174-186):
 * latent_f32[i] += dt * v_bf16[i]; latent_bf16 (may be NULL) receives the rounded copy the next forward reads          */
int omx_klein_euler_step(void* latent_f32, const void* v_bf16, float dt, void* latent_bf16, int64_t n, omx_stream stream);
int omx_klein_last_ms(omx_klein m, float* ms);          /* HIP-event time of the last forward */
int omx_klein_debug_read(omx_klein m, const char* name, void* host, size_t n_elems);   /* test hook */

/* In-process stand-in for an RCCL communicator (csrc/loopback_comm.hip): `world` engine instances driven by
 * `world` host threads of one process exchange through it, so the tensor-parallel paths run with real shards
 * on a single-GPU box.  omx_loopback_allreduce has ncclAllReduce's signature.                             */
typedef struct omx_loopback_* omx_loopback;
int omx_loopback_create(omx_loopback* out, int world, size_t max_bytes);
int omx_loopback_destroy(omx_loopback g);
void* omx_loopback_rank_comm(omx_loopback g, int rank);
int omx_loopback_abort(omx_loopback g);

/* One-shot all-reduce over xGMI peer stores for the tensor-parallel decode step (csrc/peer_allreduce.hip): one
 * process per GPU, every rank's inbox (fine-grained device memory) mapped into every peer through HIP IPC handles, a call = ONE
 * kernel that stores tagged 8-byte granules into all inboxes and reduces its own in rank order.  f32 sum / u64 max of up to 8192
 * payload words.  Larger f32 / bf16 sums (16-byte multiples) take the TWO-SHOT path when no RCCL communicator was given at creation
 * (or OMX_PEER_LARGE=1): one kernel, slice s of every rank's input pushed into rank s's stage, summed there in rank order, pushed
 * back to all -- stages of OMX_PEER_STAGE_MB (64) behind every inbox, larger messages in chunks.  Anything else goes to the RCCL
 * communicator given at creation (may be NULL: such calls then fail).
 * omx_peer_allreduce has ncclAllReduce's signature: omx_qwen3_set_comm(model, comm, omx_peer_allreduce_fn()).
 * Host protocol: create -> handle (64 bytes) -> all-gather the handles rank-major -> connect.                                 */
int omx_peer_comm_create(void** out, int rank, int world, void* rccl_comm, void* rccl_allreduce_fn);
int omx_peer_comm_handle(void* comm, void* out64);
int omx_peer_comm_connect(void* comm, const void* handles);
int omx_peer_allreduce(const void* send, void* recv, size_t count, int dtype, int op, void* comm, omx_stream stream);
void* omx_peer_allreduce_fn(void);
int omx_peer_comm_counts(void* comm, unsigned long long* out4);   /* launches by path: one-shot, two-shot chunks, MoE combine, handed to RCCL */
size_t omx_peer_comm_stage_bytes(void* comm);             /* stage size of the two-shot / exchange path; 0 = off */
/* expert-parallel prompt: out [T, hidden] = resid + weighted expert outputs as an all-to-all combine of the routed slots' rows to their
 * tokens' owners + an all-gather of the finished rows (one kernel; BASELINE config 3's "expert-parallel all-to-all over xGMI").
 * Returns 2 when this communicator / size cannot take it (the caller keeps its all-reduce). */
int omx_peer_moe_combine(void* out, const void* resid, const omx_moe_ep_slots* slots, int T, int hidden, int top_k, int e_lo, int e_n, void* comm,
                         omx_stream stream);
const void* omx_peer_comm_device(void* comm);              /* device table for kernels that reduce their own output (engine-internal use) */
int omx_peer_comm_set_scope(void* comm, int system_scope); /* two-shot / exchange hand-offs: 1 system-scope release / acquire (default), 0 agent-scope fences (ranks on ONE GPU) */
int omx_peer_comm_scope(void* comm);
int omx_peer_device_id(char* out, int len);                /* PCI bus id of the current device (ranks compare them: same GPU or not) */
int omx_peer_comm_status(void* comm, unsigned* aborted);   /* 1: a wait gave up (a peer never arrived); results are void */
int omx_peer_comm_destroy(void* comm);

/* =====================================================================================
 * a12: Paraformer mel/STFT frontend (funasr-mlx/src/paraformer.rs:195-412), all on device:
 * x*32768 -> pre-emphasis 0.97 -> frames (n-400)/160+1 -> Hamming -> 400-pt DFT power -> 80 HTK
 * mel filters -> ln(max(.,1e-10)) -> LFR(7,6) -> CMVN.  Replaces MelFrontend::{new,set_cmvn,forward}.
 * ===================================================================================== */
typedef struct omx_mel_config_ {   /* ParaformerConfig frontend fields, paraformer.rs:110-145 */
    int sample_rate, n_mels, n_fft, hop_length, lfr_m, lfr_n;
} omx_mel_config;
typedef struct omx_mel_frontend_* omx_mel_frontend;
int omx_mel_frontend_create(omx_mel_frontend* out, const omx_mel_config* cfg);          /* MelFrontend::new  :195-222 */
int omx_mel_frontend_destroy(omx_mel_frontend f);
/* MelFrontend::set_cmvn :225-228; host vectors of lfr_m*n_mels floats (am.mvn <AddShift>/<Rescale>) */
int omx_mel_frontend_set_cmvn(omx_mel_frontend f, const float* addshift_host, const float* rescale_host, int dim);
/* frame counts for n_samples: STFT frames (1 when shorter than n_fft, :386-388) and LFR frames */
int omx_mel_frontend_frames(omx_mel_frontend f, int64_t n_samples, int* n_frames, int* n_lfr);
/* MelFrontend::forward :278-367.  audio: device f32 [n_samples]; feats: device f32 [n_lfr, lfr_m*n_mels];
 * logmel_out ([n_frames, n_mels]) and power_out ([n_frames, n_fft/2+1]) are optional device outputs.
 * Non-finite samples are an error ("Audio contains NaN or Inf values", :284-286).                     */
int omx_mel_frontend_forward(omx_mel_frontend f, const float* audio, int64_t n_samples, float* feats, float* logmel_out,
                             float* power_out, omx_stream stream);

/* sibling frontend: Fun-ASR-Nano / SenseVoice log-mel, funasr-nano-mlx/src/audio.rs:44-157 (`MelFrontend::{new,
 * compute_mel_spectrogram}`, defaults 16 kHz / 80 mels / n_fft 400 / hop 160 / 30 s): symmetric Hann, frames from sample frame * hop with
 * zero padding, n_frames = max(min(n, max_length * sr) / hop, 1), DFT power, FFT-bin triangles (:287-339), ln(max(., 1e-10)).
 * audio: device f32 [n_samples]; out: device f32 [n_mels, n_frames].  Errors as the reference: empty (:95-99), shorter than a hop (:105-110).
 * omx_apply_lfr = `apply_lfr` (:345-412): mel [n_mels, n_frames] -> out [ceil(n_frames / lfr_n), lfr_m * n_mels], centred, edge-clamped. */
int omx_sensevoice_mel_create(omx_mel_frontend* out, int sample_rate, int n_mels, int n_fft, int hop_length, float max_length_s);
int omx_sensevoice_mel_frames(omx_mel_frontend f, int64_t n_samples, int* n_frames);
int omx_sensevoice_mel_forward(omx_mel_frontend f, const float* audio, int64_t n_samples, float* out, omx_stream stream);
int omx_apply_lfr(float* out, const float* mel, int n_mels, int n_frames, int lfr_m, int lfr_n, omx_stream stream);

/* audio::resample (mlx-rs-core/src/audio.rs:178-277): windowed-sinc resampling with the reference's rubato configuration (sinc_len 256,
 * oversampling 256, cubic phase interpolation, BlackmanHarris2, cutoff 0.95) and its chunking / flush / truncation driver.
 * in: device f32 [n_in]; out: device f32 [out_cap], out_cap >= omx_resample_len(n_in, src, dst) = round(n_in * dst / src), the
 * reference's truncation bound; *n_out = samples written (fewer than the bound for inputs shorter than the filter, as in the
 * reference).  Equal rates / empty input: the input unchanged (:179-181).  Synchronises the stream before returning.             */
int64_t omx_resample_len(int64_t n_in, uint32_t src_rate, uint32_t dst_rate);
int omx_resample_sinc(const float* in, int64_t n_in, uint32_t src_rate, uint32_t dst_rate, float* out, int64_t out_cap, int64_t* n_out,
                      omx_stream stream);

/* sibling frontend: WhisperFeatureExtractor-compatible log-mel, qwen3-asr-mlx/src/audio.rs:24-128
 * (`MelFrontend::{new, compute_mel_spectrogram}`, defaults 16 kHz / 128 mels / n_fft 400 / hop 160): periodic Hann ->
 * 400-pt DFT power -> Slaney filters -> log10(max(., 1e-10)) -> max(., global max - 8) -> (x + 4) / 4.
 * audio: device f32 [n_samples]; out: device f32 [n_mels, n_frames], n_frames = 1 + (n_samples - n_fft) / hop.      */
int omx_whisper_mel_create(omx_mel_frontend* out, int sample_rate, int n_mels, int n_fft, int hop_length);
int omx_whisper_mel_frames(omx_mel_frontend f, int64_t n_samples, int* n_frames);
int omx_whisper_mel_forward(omx_mel_frontend f, const float* audio, int64_t n_samples, float* out, omx_stream stream);

/* The Qwen3-ASR audio tower (qwen3-asr-mlx/src/encoder.rs:254-458, `AudioEncoder::forward_encoder`) in float32 -- the reference feeds a
 * float32 mel into bf16 parameters that are never quantised, and MLX promotes every op to float32; the caller hands the weights
 * widened to float32.  mel (what omx_whisper_mel_forward writes) -> chunks of 2 * n_window frames -> three 3x3 stride-2 convolutions +
 * GELU -> conv_out + sinusoid of the position within the chunk -> pre-norm transformer layers with attention inside windows of
 * 13 * (n_window_infer / (2 * n_window)) rows (the reference's [N, N] additive mask, never materialised) -> ln_post, proj1 + GELU, proj2.
 *   create:  shape preconditions are named "InvalidConfig" errors: d_model % 64, head width d_model / heads = 64, n_window_infer a
 *            multiple of the chunk, a chunk's rows <= max_source_positions, a window that fits the attention kernel (<= 118 rows).
 *   load:    one tensor by its key behind "audio_tower." ("conv2d1.weight" [ds, 3, 3, 1], "layers.3.self_attn.q_proj.bias", ...),
 *            float32 on the HOST; a missing key or a size the config does not imply is an error at forward.
 *   tokens:  rows N a mel of n_frames makes (get_feat_extract_output_lengths, :76-80, with floor division).
 *   forward: mel DEVICE f32 [n_mels, n_frames] -> out_rows DEVICE f32 [N, output_dim] on `stream`.  The handle owns its scratch and
 *            grows it per role; a handle reused for another n_frames gives a fresh handle's bits.  A NaN / infinite mel is refused.
 *   omx_window_attention_f32: the tower's attention alone -- q | k | v DEVICE f32 rows `ld` floats apart (the thirds of one stacked
 *            projection), head h at column 64 h, scale 1; out token-major, rows `ldo` apart; windows of `window` rows from row 0. */
typedef struct omx_qwen3_asr_encoder_* omx_qwen3_asr_encoder;
typedef struct omx_qwen3_asr_encoder_config_ {
    int n_mels, n_layers, n_heads, ffn_dim, d_model, max_source_positions, n_window, output_dim, n_window_infer, downsample_hidden_size;
} omx_qwen3_asr_encoder_config;
int omx_qwen3_asr_encoder_create(omx_qwen3_asr_encoder* out, const omx_qwen3_asr_encoder_config* cfg);
int omx_qwen3_asr_encoder_load(omx_qwen3_asr_encoder e, const char* name, const float* host, const int64_t* shape, int ndim);
int omx_qwen3_asr_encoder_tokens(omx_qwen3_asr_encoder e, int n_frames, int* n);
int omx_qwen3_asr_encoder_forward(omx_qwen3_asr_encoder e, const float* mel, int n_frames, float* out_rows, omx_stream stream);
int omx_qwen3_asr_encoder_destroy(omx_qwen3_asr_encoder e);
/* test hook: n_elems floats of a stage of the LAST forward to the host -- "x1" / "x2" / "x3" the stem's layers [chunks, f, t, ds] (NHWC),
 * "h" the hidden rows [N, d_model] (the assembled rows when the tower has no layers) */
int omx_qwen3_asr_encoder_debug_read(omx_qwen3_asr_encoder e, const char* name, float* host, size_t n_elems);
int omx_window_attention_f32(float* out, int64_t ldo, const float* q, const float* k, const float* v, int64_t ld, int n, int heads, int window,
                             omx_stream stream);

/* The audio tower of Fun-ASR-Nano (funasr-nano-mlx/src/sensevoice_encoder.rs:453-478 `SenseVoiceEncoder::forward`, then adaptor.rs:247-261
 * `AudioAdaptor::forward`) in float32, over UP TO 8 UTTERANCES AT ONCE: their LFR rows stacked into one [sum T, lfr_dim] tensor, every GEMM
 * and LayerNorm over all rows, attention and the FSMN memory block stopping at utterance boundaries, positions restarting at 1.
 *   x + PE(t + 1) (no scale) -> encoders0 (lfr_dim -> output_size, no attention residual) -> num_blocks - 1 encoders -> after_norm ->
 *   tp_blocks tp_encoders -> tp_norm -> linear1 + ReLU -> linear2 -> n_layer pre-norm blocks (8 heads, FFN bottleneck 256) -> [sum T, llm_dim]
 *   create:  "InvalidConfig" by name: head width other than 128 (output_size / attention_heads, or llm_dim / 8), an even or > 31
 *            kernel_size, widths that are no multiple of 4.
 *   load:    one tensor by its key after the reference's key map (model.rs:350-374): "encoder.encoders0.0.self_attn.linear_q_k_v.weight",
 *            "encoder.tp_encoders.3.self_attn.fsmn.weight" [dim, 1, k], "encoder.after_norm.bias", "adaptor.linear1.weight",
 *            "adaptor.blocks.0.self_attn.linear_q.weight", ...; float32 on the HOST.  Keys with another prefix are refused; the shape is
 *            checked against the config at once ("ShapeMismatch"); a missing key is "WeightNotFound" at forward.  The adaptor's
 *            linear_q / k / v are stacked into one [3 llm_dim, llm_dim] product at the first forward.
 *   forward: lfr_rows DEVICE f32 [sum T, lfr_dim]; seg HOST int[n_utt + 1], the row offsets (seg[0] = 0, increasing); out_rows DEVICE f32
 *            [sum T, llm_dim].  1 <= n_utt <= 8, every utterance 1..512 rows (30 s of audio make 501; 512 is the one-launch attention's
 *            key limit): anything else is refused by name before the first launch.  A GEMM's split of K depends on its row count, so the
 *            last bits of an utterance's rows may depend on what shares the pass.
 *   omx_segment_attention_f32: the tower's attention alone -- out = softmax(q k^T / sqrt(128)) v per head of width 128 and per utterance,
 *            one launch; q | k | v DEVICE f32 rows ld* floats apart, head h at column 128 h.
 *   omx_sanm_segment_layer_f32: one SenseVoiceEncoderLayer (:368-384) over stacked utterances, x [sum T, in_dim] -> out [sum T, dim];
 *            in_dim != dim is the first layer's form (no attention residual).  Declared with omx_sanm_layer_weights below. */
typedef struct omx_funasr_nano_encoder_* omx_funasr_nano_encoder;
typedef struct omx_funasr_nano_encoder_config_ {
    int lfr_dim, output_size, attention_heads, linear_units, num_blocks, tp_blocks, kernel_size;   /* SenseVoiceEncoderConfig */
    int encoder_dim, ffn_dim, llm_dim, n_layer;                                                     /* AdaptorConfig */
} omx_funasr_nano_encoder_config;
int omx_funasr_nano_encoder_create(omx_funasr_nano_encoder* out, const omx_funasr_nano_encoder_config* cfg);
int omx_funasr_nano_encoder_load(omx_funasr_nano_encoder e, const char* name, const float* host, const int64_t* shape, int ndim);
int omx_funasr_nano_encoder_forward(omx_funasr_nano_encoder e, const float* lfr_rows, const int* seg, int n_utt, float* out_rows, omx_stream stream);
int omx_funasr_nano_encoder_destroy(omx_funasr_nano_encoder e);
/* test hook: n_elems floats of a stage of the LAST forward to the host -- "pos" [sum T, lfr_dim] (rows + positions), "after_norm" and
 * "tp_norm" [sum T, output_size], "linear2" [sum T, llm_dim] (the adaptor before its blocks; the blocks' output is out_rows) */
int omx_funasr_nano_encoder_debug_read(omx_funasr_nano_encoder e, const char* name, float* host, size_t n_elems);
int omx_segment_attention_f32(float* out, const float* q, const float* k, const float* v, int64_t ldq, int64_t ldkv, int64_t ldo, const int* seg,
                              int n_utt, int heads, omx_stream stream);

/* The vision towers of Moxin-VLM (moxin-vlm-mlx/src/vision.rs `ViTEncoder::forward`, :259-310) and its projector (projector.rs:34-40) in
 * float32 -- the reference feeds a float32 image into bf16 parameters and casts nothing, MLX promotes every op to float32; the caller
 * hands the weights widened to float32.  image [S, S, 3] in [0, 1] -> (x - mean) / std -> P x P stride-P convolution (im2col + the
 * float32 matrix-core GEMM) -> CLS | registers | patches + pos_embed -> blocks 0 .. depth - 2 (pre-norm, eps 1e-6, exact GELU,
 * optional LayerScale) -> the patch rows; the final norm is never applied, as in the reference.
 *   config:  every field of ViTConfig, the three-channel mean / std of the tower's image preparation (lib.rs:427-440), and the
 *            checkpoint prefix the error texts name ("vision_backbone.featurizer").
 *   create:  "InvalidConfig" by name: head width other than 64 / 72, embed_dim != heads * width, image size no multiple of the patch,
 *            more than 1024 rows.
 *   load:    one tensor by its key behind the prefix ("patch_embed.proj.weight" [O, 3, P, P] as the checkpoint holds it, "pos_embed",
 *            "cls_token", "reg_token" or "register_tokens", "blocks.3.attn.qkv.weight", "blocks.3.ls1.gamma" or ".scale_factor", ...),
 *            float32 on the HOST.  A missing key ("WeightNotFound: <key>"), a size the config does not imply, or a pos_embed of
 *            neither num_patches nor num_patches + 1 rows is an error at forward, before any launch.  Biases are optional.
 *   tokens:  rows of the sequence (CLS + registers + patches) and rows that come out (patches).
 *   forward: image DEVICE f32 [S, S, 3] -> out_rows DEVICE f32 [patches, embed_dim], rows `ldo` floats apart (two towers fill the two
 *            column ranges of one buffer).  The handle owns its scratch and reuses it; a reused handle gives a fresh handle's bits.  A
 *            NaN / infinite image is refused.
 *   debug_read (test hook): a stage of the LAST forward -- "col" [patches, 3 P P], "patches" [patches, dim], "h" [tokens, dim] (the
 *            assembled rows when no block runs, else the last block's rows after its attention residual), and of the last block "ln1",
 *            "qkv" [tokens, 3 dim], "attn", "ln2", "mlp" [tokens, intermediate].
 *   omx_vit_attention_f32: the towers' attention alone -- unmasked softmax(q k^T width^-0.5) v in float32 on the f32 matrix cores;
 *            q | k | v DEVICE rows `ld` floats apart, head h at column h * width, out token-major.  width 64 or 72, 1 <= n <= 1024,
 *            anything else is refused by name.  Fixed summation order: the same input gives the same bits.
 *   omx_gemm_f32_epilogue: out [M, N] = resid + col_scale * gelu?(a [M, K] . w [N, K]^T + bias) through the float32 GEMM's fused
 *            epilogues (test hook and building block); bias, resid, col_scale optional, all contiguous.
 *   omx_vlm_projector_*: fc1 -> gelu -> fc2 -> gelu -> fc3 with keys "fc1.weight", "fc1.bias", ...; widths are read from the weights. */
typedef struct omx_vit_encoder_* omx_vit_encoder;
typedef struct omx_vlm_projector_* omx_vlm_projector;
typedef struct omx_vit_config_ {
    int embed_dim, depth, num_heads, head_dim, intermediate_dim, has_cls_token, num_registers, has_layer_scale, patch_size, image_size;
    float mean[3], std[3];
    char key_prefix[128];
} omx_vit_config;
int omx_vit_encoder_create(omx_vit_encoder* out, const omx_vit_config* cfg);
int omx_vit_encoder_load(omx_vit_encoder e, const char* name, const float* host, const int64_t* shape, int ndim);
int omx_vit_encoder_tokens(omx_vit_encoder e, int* n_tokens, int* n_rows);
int omx_vit_encoder_forward(omx_vit_encoder e, const float* image, float* out_rows, int64_t ldo, omx_stream stream);
int omx_vit_encoder_launches(omx_vit_encoder e, int* n);   /* launches the last forward enqueued, split-K reduce launches not counted */
int omx_vit_encoder_debug_read(omx_vit_encoder e, const char* name, float* host, size_t n_elems);
int omx_vit_encoder_destroy(omx_vit_encoder e);
int omx_vit_attention_f32(float* out, int64_t ldo, const float* q, const float* k, const float* v, int64_t ld, int n, int heads, int width,
                          omx_stream stream);
int omx_gemm_f32_epilogue(float* out, const float* a, const float* w, const float* bias, const float* resid, const float* col_scale, int M, int N, int K,
                          int gelu, omx_stream stream);
int omx_vlm_projector_create(omx_vlm_projector* out);
int omx_vlm_projector_load(omx_vlm_projector p, const char* name, const float* host, const int64_t* shape, int ndim);
int omx_vlm_projector_dims(omx_vlm_projector p, int* in_dim, int* out_dim);
int omx_vlm_projector_forward(omx_vlm_projector p, const float* x, int rows, float* out, omx_stream stream);
int omx_vlm_projector_destroy(omx_vlm_projector p);

/* The vision side of DeepSeek-OCR-2 (deepseek-ocr2-mlx/src/vision.rs `ImageEncoderViT::forward` :385-431, qwen2_encoder.rs
 * `Qwen2Encoder::forward_vision` :198-244) in float32, for the reason given above: a float32 image meets bf16 parameters, nothing is cast.
 * The caller hands the weights widened to float32, by their checkpoint keys behind the prefix.
 *   omx_sam_attention_f32: SAM's attention alone over `images` stacked images of a gh x gw grid.  qkv DEVICE rows `ld` floats apart hold
 *            q | k | v side by side, head h at column 64 h; out [images * gh * gw, heads * 64] token-major in image order.
 *            s = (q . k) / 8 + q . Rh[qh, kh] + q . Rw[qw, kw] (q unscaled in the bias), R[a, b] = T[a - b + g - 1] with T = rel_pos_*
 *            [len, 64] resampled nearest-neighbour when len != 2 g - 1 (vision.rs:186-196).  window 0: every key of the image, any
 *            count -- an online softmax on the float32 matrix cores, nothing of N x N is written to memory, the bias comes from
 *            [64, gh + gw] tables a block builds in LDS.  window > 0: the grid zero-padded to multiples of the window and cut into
 *            windows (:271-326) with g = window; the rows are read in place, a padded position reads pad_qkv [3 * heads * 64] (the qkv
 *            Linear's bias) as its q | k | v, takes part as a key and is dropped as a query; pad_qkv is required when a grid side is no
 *            multiple of the window.  width other than 64 is refused by name.  Fixed summation order: the same bits twice.
 *   omx_prefix_causal_attention_f32: `images` stacked sequences of n_rows; qkv rows hold `heads` query heads, then kv_heads key heads,
 *            then kv_heads value heads of 64; query head h reads key/value head h / (heads / kv_heads); row i sees keys
 *            j < max(n_prefix, i + 1) of its own sequence (qwen2_encoder.rs:249-288); scale 1 / 8; any n_rows.
 *   omx_sam_encoder_*: images DEVICE f32 [n, S, S, 3] in [-1, 1], S a multiple of the patch -> out_rows DEVICE f32 [n * (S / P / 4)^2,
 *            net_3's rows].  16 x 16 patch convolution + bias, + pos_embed (gathered nearest-neighbour where its grid differs, :435-454),
 *            the blocks (LayerNorm 1e-6, attention as above -- global on global_attn_indexes, windowed elsewhere --, tanh GELU), neck
 *            and the two stride-2 convolutions; neck and output widths are read from the weights.  keep_stages: keep a copy of the rows
 *            after the positions and after every block for debug_read (tests).  tokens: the grid side, the rows per image that come out
 *            and their width.  scratch_bytes: the device scratch the handle holds after its last forward (the split-K workspace the
 *            GEMMs share per stream is not the handle's).  debug_read stages: "patches", "h0", "block<N>" [n * G * G, embed_dim],
 *            "neck" [n * G * G, neck width], "out".
 *   omx_vcf_encoder_*: x DEVICE f32 [n * n_img, hidden] (the SAM rows) -> out_rows DEVICE f32 [n * n_query, hidden]: per image its rows
 *            followed by query_768 (n_img == 144) or query_1024 (otherwise), `layers` Qwen2 layers (RMSNorm, q | k | v with bias in one
 *            stacked GEMM, RoPE over the full 64 dims at positions 0 .. L - 1, the prefix-causal attention with n_prefix = n_img,
 *            SwiGLU MLP), the final RMSNorm, the query rows.  debug_read stages: "layer<N>" [n * L, hidden] (keep_stages), "out". */
typedef struct omx_sam_encoder_* omx_sam_encoder;
typedef struct omx_vcf_encoder_* omx_vcf_encoder;
typedef struct omx_sam_config_ {
    int embed_dim, depth, num_heads, mlp_dim, window, patch_size, n_global, keep_stages;
    int global_attn_indexes[16];
    char key_prefix[128];
} omx_sam_config;
typedef struct omx_vcf_config_ {
    int hidden, layers, heads, kv_heads, intermediate, keep_stages;
    float rope_theta, eps;
    char key_prefix[128];
} omx_vcf_config;
int omx_sam_attention_f32(float* out, int64_t ldo, const float* qkv, int64_t ld, int images, int gh, int gw, int heads, int width, int window,
                          const float* rel_pos_h, int len_h, const float* rel_pos_w, int len_w, const float* pad_qkv, omx_stream stream);
int omx_prefix_causal_attention_f32(float* out, int64_t ldo, const float* qkv, int64_t ld, int images, int n_rows, int heads, int kv_heads, int width,
                                    int n_prefix, omx_stream stream);
int omx_sam_encoder_create(omx_sam_encoder* out, const omx_sam_config* cfg);
int omx_sam_encoder_load(omx_sam_encoder e, const char* name, const float* host, const int64_t* shape, int ndim);
int omx_sam_encoder_tokens(omx_sam_encoder e, int image_size, int* grid, int* n_rows, int* out_dim);
int omx_sam_encoder_forward(omx_sam_encoder e, const float* images, int n_images, int image_size, float* out_rows, omx_stream stream);
int omx_sam_encoder_launches(omx_sam_encoder e, int* n);   /* launches the last forward enqueued, split-K reduce launches not counted */
int omx_sam_encoder_scratch_bytes(omx_sam_encoder e, size_t* bytes);
int omx_sam_encoder_debug_read(omx_sam_encoder e, const char* name, float* host, size_t n_elems);
int omx_sam_encoder_destroy(omx_sam_encoder e);
int omx_vcf_encoder_create(omx_vcf_encoder* out, const omx_vcf_config* cfg);
int omx_vcf_encoder_load(omx_vcf_encoder e, const char* name, const float* host, const int64_t* shape, int ndim);
int omx_vcf_encoder_tokens(omx_vcf_encoder e, int n_img, int* n_query, int* seq_len);
int omx_vcf_encoder_forward(omx_vcf_encoder e, const float* x, int n_images, int n_img, float* out_rows, omx_stream stream);
int omx_vcf_encoder_launches(omx_vcf_encoder e, int* n);
int omx_vcf_encoder_scratch_bytes(omx_vcf_encoder e, size_t* bytes);
int omx_vcf_encoder_debug_read(omx_vcf_encoder e, const char* name, float* host, size_t n_elems);
int omx_vcf_encoder_destroy(omx_vcf_encoder e);

/* =====================================================================================
 * a13: Paraformer body pieces (funasr-mlx/src/paraformer.rs).
 *   omx_sanm_encoder_layer  SanmEncoderLayer::forward :618-634 = LayerNorm(1e-5) -> SanmAttention (:496-532:
 *       fused qkv Linear, softmax(q k^T d^-1/2) v with heads x 128, FSMN depthwise Conv1d(k=11, pad 5) over v
 *       plus v, out_proj) -> residual (skipped when in_dim != dim, :625-629) -> LayerNorm -> Linear/ReLU/Linear
 *       (:560-570) -> residual.  x [T, in_dim] -> out [T, dim]; weights: Linear [out, in] + bias [out];
 *       fsmn_w [dim, kernel_size] (MLX Conv1d weight [C, k, 1], :1293-1298).
 *   Every entry point takes the arithmetic mode as `dtype` -- activations AND weights are of that type:
 *       OMX_FLOAT32   the reference's own (f32 checkpoint, f32 activations; exact-f32 matrix cores, explicit softmax);
 *       OMX_BFLOAT16  bf16 with fp32 accumulation (faster; narrower than the reference).
 *   omx_cif_fire            CIFPredictor::cif_fire :779-879 (threshold 1.0, tail 0.45): hidden [B, T, H] f32,
 *       alphas [B, T] f32 -> frames [B, max_frames, H] f32 (zero padded) and counts [B]; all device pointers.
 * ===================================================================================== */
typedef struct omx_sanm_layer_weights_ {
    const void *norm1_w, *norm1_b, *qkv_w, *qkv_b, *out_w, *out_b, *fsmn_w, *norm2_w, *norm2_b, *ffn_up_w, *ffn_up_b,
        *ffn_down_w, *ffn_down_b;
} omx_sanm_layer_weights;
int omx_sanm_encoder_layer(void* out, const void* x, const omx_sanm_layer_weights* w, int T, int in_dim, int dim,
                           int heads, int ffn_dim, int kernel_size, omx_dtype dtype, omx_stream stream);
/* SanmEncoder::forward's layer loop + after_norm (paraformer.rs:691-708) in ONE call (round 6): layers[0] maps in_dim -> dim, the others
 * keep dim; out [T, dim] = after_norm(layers(x)).  Scratch (device, caller-owned): act0 / act1 [T, dim], nrm0 / nrm1 [T, max(in_dim, dim)].
 * In float32 every layer's last launch also computes the next layer's norm1 (the last one: after_norm). */
int omx_sanm_encoder_stack(void* out, const void* x, const omx_sanm_layer_weights* layers, int n_layers, int T, int in_dim, int dim, int heads,
                           int ffn_dim, int kernel_size, const void* after_norm_w, const void* after_norm_b, void* act0, void* act1, void* nrm0,
                           void* nrm1, omx_dtype dtype, omx_stream stream);
/* one SenseVoiceEncoderLayer over stacked utterances (float32; see omx_funasr_nano_encoder above): seg HOST int[n_utt + 1] */
int omx_sanm_segment_layer_f32(float* out, const float* x, const omx_sanm_layer_weights* w, const int* seg, int n_utt, int in_dim, int dim,
                               int heads, int ffn_dim, int kernel_size, omx_stream stream);
int omx_cif_fire(float* frames, int* counts, const float* hidden, const float* alphas, int batch, int T, int H,
                 float threshold, float tail_threshold, int max_frames, omx_stream stream);
/* SanmEncoder::forward prologue (paraformer.rs:691-703): out [T, dim] = mel f32 [T, dim] * sqrt(512) + sinusoidal
 * position encoding (positions 1.., [sin | cos] halves, :418-439) */
int omx_paraformer_embed(void* out, const float* mel, int T, int dim, omx_dtype dtype, omx_stream stream);
/* CIFPredictor::compute_alphas (:761-768): alphas f32 [T] = sigmoid(Linear_{dim->1}(relu(Conv1d_{k}(enc)))) with the dense
 * convolution weight in MLX layout [dim_out, k, dim_in]; also writes enc as f32 (the hidden CIF integrates)           */
int omx_cif_alphas(float* alphas, float* hidden_f32, const void* enc, const void* conv_w, const void* conv_b,
                   const void* proj_w, const void* proj_b, int T, int dim, int kernel_size, omx_dtype dtype, omx_stream stream);
/* ParaformerDecoderLayer::forward (:1030-1053) incl. cross_attention (:981-1017): x [N, dim] acoustic embeddings,
 * enc [Ts, enc_dim] encoder output; FFN down has no bias (loader :1421)                                              */
typedef struct omx_paraformer_decoder_weights_ {
    const void *norm1_w, *norm1_b, *ffn_up_w, *ffn_up_b, *ffn_norm_w, *ffn_norm_b, *ffn_down_w, *norm2_w, *norm2_b, *fsmn_w,
        *norm3_w, *norm3_b, *q_w, *q_b, *kv_w, *kv_b, *out_w, *out_b;
} omx_paraformer_decoder_weights;
int omx_paraformer_decoder_layer(void* out, const void* x, const void* enc, const omx_paraformer_decoder_weights* w, int N,
                                 int Ts, int dim, int enc_dim, int heads, int ffn_dim, int kernel_size, omx_dtype dtype,
                                 omx_stream stream);
/* The float32 model's attention as one op (funasr-mlx/src/paraformer.rs:509-516 encoder self-attention, :1090-1102 decoder cross-attention):
 * out = softmax(q k^T / sqrt(128)) v per head of width 128, f32 throughout, no mask; rows ldq / ldkv / ldo floats apart, head h at column
 * 128 h (so q | k | v may be the three thirds of one fused projection). */
int omx_paraformer_attention_f32(float* out, const float* q, const float* k, const float* v, int64_t ldq, int64_t ldkv, int64_t ldo, int Tq,
                                 int Tk, int heads, omx_stream stream);
/* ParaformerDecoder::forward's layer loop (:1144-1156) in one call: out [N, dim] = layers(x).  Scratch: act0/act1 [N, dim], nrm0/nrm1 [N, dim],
 * kv_all [Ts, n_layers * 2 * dim] or null.  With kv_all given and the layers' linear_k_v weights / biases back to back in memory, the encoder
 * output's k | v projection for ALL layers is one GEMM up front; in float32 each layer's last launch also computes the next layer's norm1. */
int omx_paraformer_decoder_stack(void* out, const void* x, const void* enc, const omx_paraformer_decoder_weights* layers, int n_layers, int N,
                                 int Ts, int dim, int enc_dim, int heads, int ffn_dim, int kernel_size, void* act0, void* act1, void* nrm0,
                                 void* nrm1, void* kv_all, omx_dtype dtype, omx_stream stream);
/* ParaformerDecoder::forward tail (:1157-1165): LN -> Linear+ReLU -> LN(ffn) -> Linear(no bias) -> LN -> output_proj;
 * logits [N, vocab]                                                                                                    */
typedef struct omx_paraformer_tail_weights_ {
    const void *norm1_w, *norm1_b, *up_w, *up_b, *ffn_norm_w, *ffn_norm_b, *down_w, *after_norm_w, *after_norm_b, *out_w, *out_b;
} omx_paraformer_tail_weights;
int omx_paraformer_decoder_tail(void* logits, const void* x, const omx_paraformer_tail_weights* w, int N, int dim, int ffn_dim,
                                int vocab, omx_dtype dtype, omx_stream stream);
/* elementwise dtype conversion between bf16 / f16 / f32 device buffers (Array::as_dtype) */
int omx_cast(void* dst, omx_dtype dst_dtype, const void* src, omx_dtype src_dtype, int64_t n, omx_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* OMX_H */
