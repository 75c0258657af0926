// Paraformer body pieces: SAN-M encoder layer and the CIF integrate-and-fire.
//   reference: funasr-mlx/src/paraformer.rs -- SanmAttention::forward :496-532, FeedForward :560-570,
//   SanmEncoderLayer::forward :618-634, CIFPredictor::cif_fire :779-879.
// The reference runs this model in float32 with explicit QK^T / softmax / PV matmuls and a CPU loop for CIF
// (with a device->host->device round trip).  Two arithmetic modes here, chosen by the `dtype` argument of every entry point:
//   OMX_FLOAT32   the reference's own: f32 weights and activations, every GEMM on the exact-f32 matrix cores (gemm_f32.hip),
//                 explicit scores / row softmax / PV in f32 -- the mode the parity bar is stated for (1e-4 of the oracle);
//   OMX_BFLOAT16  bf16 weights / activations with fp32 accumulation on the bf16 matrix cores and the flash-attention kernel
//                 (the fused projection consumed in place through strides) -- faster, lower precision than the reference.
// Both: the FSMN depthwise convolution + both residual adds in one pass, CIF without a host round trip.
#include <math.h>

#include "gemm.hpp"
#include "sanm_f32.hpp"
#include "workspace.hpp"

namespace omx {
namespace {

// CIF integrate-and-fire (paraformer.rs:779-879).  The fire decisions form a scalar recurrence over time that does not depend
// on the hidden column, and a fired frame only sums the few time steps between two fires.  So: every block of the (batch, NB)
// grid replays the scalar recurrence from LDS (one thread, ~10 ns per step; T = 501 -> 5 us) and records, per fired frame, the
// time step and the weight of that step; then the blocks share the frames, thread d owning hidden column d, each frame summed
// in time order with the operations of the serial definition (frame = remainder * h; frame += alpha * h ...; frame +=
// completion * h) -- the same bits as a one-thread-per-column walk over all T steps, which took 280 us for 30 s of audio.
__global__ __launch_bounds__(256) void cif_fire_kernel(const float* __restrict__ hidden, const float* __restrict__ alphas,
                                                       int T, int H, float threshold, float tail_threshold,
                                                       float* __restrict__ frames, int max_frames, int* __restrict__ counts) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cif_smem[];
    float* al = reinterpret_cast<float*>(cif_smem);                 // [T]
    int* fire_t = reinterpret_cast<int*>(al + T);                   // [max_frames] time step of the n-th fire
    float* fire_w = reinterpret_cast<float*>(fire_t + max_frames);  // [max_frames] weight of that step in the fired frame
    __shared__ int s_fired, s_tail;
    const int b = blockIdx.x;
    const float* hb = hidden + (size_t)b * T * H;
    const float* ab = alphas + (size_t)b * T;
    float* fb = frames + (size_t)b * max_frames * H;
    for (int t = threadIdx.x; t < T; t += blockDim.x) al[t] = ab[t];
    __syncthreads();
    if (threadIdx.x == 0) {
        float integrate = 0.f;
        int n = 0;
#pragma unroll 4
        for (int t = 0; t < T; ++t) {
            const float alpha = al[t];
            const float completion = 1.0f - integrate;
            integrate += alpha;
            if (integrate >= threshold) {
                integrate -= 1.0f;
                if (n < max_frames) { fire_t[n] = t; fire_w[n] = completion; }
                ++n;
            }
        }
        s_fired = n;
        s_tail = integrate > tail_threshold ? 1 : 0;
        if (blockIdx.y == 0) counts[b] = n + s_tail;
    }
    __syncthreads();
    const int fired = s_fired;
    const int n_out = min(fired + s_tail, max_frames);
    for (int n = blockIdx.y; n < n_out; n += gridDim.y) {
        const int t_prev = n > 0 ? fire_t[n - 1] : -1;              // the fire that opened this frame
        const bool closes = n < fired;                              // ends with a fire (else: the tail frame)
        const int t_end = closes ? fire_t[n] : T;                   // plain-alpha steps are (t_prev, t_end)
        for (int d = threadIdx.x; d < H; d += blockDim.x) {
            float frame = 0.f;
            if (t_prev >= 0) frame = (al[t_prev] - fire_w[n - 1]) * hb[(size_t)t_prev * H + d];
            for (int t = t_prev + 1; t < t_end; ++t) frame += al[t] * hb[(size_t)t * H + d];
            if (closes) frame += fire_w[n] * hb[(size_t)t_end * H + d];
            fb[(size_t)n * H + d] = frame;
        }
    }
}

// out = mel * sqrt(512) + PE, PE[pos, i] = sin((pos+1) * ts_i), PE[pos, half+i] = cos(...), ts_i = exp(-i ln(1e4)/(half-1))
template <int DT>
__global__ __launch_bounds__(256) void paraformer_embed_kernel(typename Elem<DT>::T* __restrict__ out, const float* __restrict__ mel, int T, int dim) {
    const int half = dim / 2;
    const float inc = logf(10000.0f) / ((float)half - 1.0f);
    const float scale = sqrtf(512.0f);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < (int64_t)T * dim; i += (int64_t)gridDim.x * 256) {
        const int pos = (int)(i / dim), c = (int)(i % dim);
        const int k = c < half ? c : c - half;
        const float st = (float)(pos + 1) * expf(-(float)k * inc);
        const float pe = c < half ? sinf(st) : cosf(st);
        Elem<DT>::st(out + i, mel[i] * scale + pe);
    }
}

// im2col for a dense Conv1d over time: col[t, j*C + c] = x[t + j - pad, c] (zero padded); also x as f32
template <int DT>
__global__ __launch_bounds__(256) void im2col_time_kernel(typename Elem<DT>::T* __restrict__ col, float* __restrict__ xf, const typename Elem<DT>::T* __restrict__ x,
                                                          int T, int C, int ksize) {
    const int pad = ksize / 2;
    const int64_t n = (int64_t)T * ksize * C;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % C), j = (int)((i / C) % ksize), t = (int)(i / ((int64_t)C * ksize));
        const int tt = t + j - pad;
        const typename Elem<DT>::T v = (tt >= 0 && tt < T) ? x[(size_t)tt * C + c] : (typename Elem<DT>::T)0;
        col[i] = v;
        if (xf && j == pad) xf[(size_t)t * C + c] = Elem<DT>::ld(&v);
    }
}

// alphas[t] = sigmoid(h[t] . w + b) (each op output in the activation dtype), one wave per row
template <int DT>
__global__ __launch_bounds__(256) void alpha_head_kernel(float* __restrict__ alphas, const typename Elem<DT>::T* __restrict__ h,
                                                         const typename Elem<DT>::T* __restrict__ w, const typename Elem<DT>::T* __restrict__ b, int T, int C) {
    typedef Elem<DT> E;
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= T) return;
    float acc = 0.f;
    for (int c = lane; c < C; c += 64) acc = fmaf(E::ld(h + (size_t)t * C + c), E::ld(w + c), acc);
    acc = wave_sum(acc);
    if (lane == 0) {
        const float z = E::rnd(acc + (b ? E::ld(b) : 0.f));
        alphas[t] = E::rnd(1.0f / (1.0f + expf(-z)));
    }
}

template <int DD, int DS>
__global__ __launch_bounds__(256) void cast_dt_kernel(typename Elem<DD>::T* __restrict__ dst, const typename Elem<DS>::T* __restrict__ src, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        Elem<DD>::st(dst + i, Elem<DS>::ld(src + i));
}

}  // namespace
}  // namespace omx

extern "C" {

int omx_cast(void* dst, omx_dtype dd, const void* src, omx_dtype ds, int64_t n, omx_stream stream) {
    using namespace omx;
    OMX_REQUIRE(dst && src && n >= 0, "omx_cast: bad arguments");
    if (n == 0) return 0;
    const unsigned blocks = (unsigned)((n + 255) / 256 < 8192 ? (n + 255) / 256 : 8192);
    hipStream_t s = (hipStream_t)stream;
#define OMX_CAST_CASE(A, B)                                                                                                 \
    if (dd == A && ds == B) {                                                                                               \
        cast_dt_kernel<A, B><<<blocks, 256, 0, s>>>((Elem<A>::T*)dst, (const Elem<B>::T*)src, n);                           \
        OMX_LAUNCH_CHECK();                                                                                                 \
        return 0;                                                                                                           \
    }
    OMX_CAST_CASE(OMX_BFLOAT16, OMX_FLOAT32) OMX_CAST_CASE(OMX_FLOAT32, OMX_BFLOAT16) OMX_CAST_CASE(OMX_FLOAT16, OMX_FLOAT32)
    OMX_CAST_CASE(OMX_FLOAT32, OMX_FLOAT16) OMX_CAST_CASE(OMX_BFLOAT16, OMX_FLOAT16) OMX_CAST_CASE(OMX_FLOAT16, OMX_BFLOAT16)
    OMX_CAST_CASE(OMX_FLOAT32, OMX_FLOAT32) OMX_CAST_CASE(OMX_BFLOAT16, OMX_BFLOAT16) OMX_CAST_CASE(OMX_FLOAT16, OMX_FLOAT16)
#undef OMX_CAST_CASE
    return set_error("omx_cast: unsupported conversion %d -> %d", (int)ds, (int)dd);
}

}  // extern "C"

namespace omx {
namespace {

// row softmax in place over [rows, n] f32, one wave per row (the explicit attention of the f32 mode, paraformer.rs:513-514)
__global__ __launch_bounds__(256) void softmax_rows_f32_kernel(float* __restrict__ s, int64_t rows, int n) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    float* p = s + row * n;
    float mx = -INFINITY;
    for (int i = lane; i < n; i += 64) mx = fmaxf(mx, p[i]);
    mx = wave_max(mx);
    float sum = 0.f;
    for (int i = lane; i < n; i += 64) { const float e = expf(p[i] - mx); p[i] = e; sum += e; }
    sum = wave_sum(sum);
    for (int i = lane; i < n; i += 64) p[i] = p[i] / sum;
}

// the GEMM / attention building blocks in the two arithmetic modes
template <int DT> struct Ops;
template <> struct Ops<OMX_BFLOAT16> {
    typedef bf16_t T;
    static int gemm(T* out, const T* x, const T* w, const T* b, int M, int N, int K, hipStream_t s) { return launch_gemm_bf16(out, x, w, b, M, N, K, s); }
    static int gemm_relu(T* out, const T* x, const T* w, const T* b, int M, int N, int K, hipStream_t s) { return launch_gemm_bf16_bias_relu(out, x, w, b, M, N, K, s); }
    static int gemm_resid(T* out, const T* x, const T* w, const T* b, const T* r, int M, int N, int K, hipStream_t s) { return launch_gemm_bf16_ex(out, x, w, b, r, M, N, K, s); }
    static size_t score_elems(int, int, int) { return 0; }
    // softmax(q k^T * scale) v per head; q / k / v / out rows `ld*` apart, head h at column h * 128
    static int attention(T* out, const T* q, const T* k, const T* v, int64_t ldq, int64_t ldkv, int64_t ldo, int Tq, int Tk, int heads, float*,
                         hipStream_t s) {
        AttnLayout L = {0, 128, ldq, ldkv, 0, 128, ldo};
        return launch_attn_prefill(out, q, k, v, 1, heads, heads, Tq, Tk, 128, 0, 128, 1.0f / sqrtf(128.0f), OMX_MASK_NONE, nullptr, s, false, &L);
    }
};
template <> struct Ops<OMX_FLOAT32> {
    typedef float T;
    static int g(T* out, const T* x, const T* w, const T* b, const T* r, int M, int N, int K, int relu, hipStream_t s) {
        GemmF32 p = {x, w, b, r, out, M, N, K, K, K, N, N, 0, 0, 0, 1, relu, 0, 1.0f};
        return launch_gemm_f32(p, s);
    }
    static int gemm(T* out, const T* x, const T* w, const T* b, int M, int N, int K, hipStream_t s) { return g(out, x, w, b, nullptr, M, N, K, 0, s); }
    static int gemm_relu(T* out, const T* x, const T* w, const T* b, int M, int N, int K, hipStream_t s) { return g(out, x, w, b, nullptr, M, N, K, 1, s); }
    static int gemm_resid(T* out, const T* x, const T* w, const T* b, const T* r, int M, int N, int K, hipStream_t s) { return g(out, x, w, b, r, M, N, K, 0, s); }
    static size_t score_elems(int heads, int Tq, int Tk) { return (size_t)heads * Tq * Tk; }
    // the reference's explicit form (paraformer.rs:509-516): scores = q k^T * scale -> softmax over keys -> scores . v, all f32
    static int attention(T* out, const T* q, const T* k, const T* v, int64_t ldq, int64_t ldkv, int64_t ldo, int Tq, int Tk, int heads, float* scores,
                         hipStream_t s) {
        const int one = launch_attn_f32(out, q, k, v, ldq, ldkv, ldo, Tq, Tk, heads, 1.0f / sqrtf(128.0f), s);
        if (one >= 0) return one;
        GemmF32 qk = {q, k, nullptr, nullptr, scores, Tq, Tk, 128, ldq, ldkv, Tk, 0, 128, 128, (int64_t)Tq * Tk, heads, 0, 0, 1.0f / sqrtf(128.0f)};
        if (launch_gemm_f32(qk, s)) return 1;
        const int64_t rows = (int64_t)heads * Tq;
        softmax_rows_f32_kernel<<<(unsigned)((rows + 3) / 4), 256, 0, s>>>(scores, rows, Tk);
        OMX_LAUNCH_CHECK();
        GemmF32 pv = {scores, v, nullptr, nullptr, out, Tq, 128, Tk, Tk, ldkv, ldo, 0, (int64_t)Tq * Tk, 128, 128, heads, 0, 1, 1.0f};
        return launch_gemm_f32(pv, s);
    }
};

template <int DT>
int cif_alphas_impl(float* alphas, float* hidden_f32, const void* enc, const void* conv_w, const void* conv_b, const void* proj_w,
                    const void* proj_b, int T, int dim, int kernel_size, hipStream_t s) {
    typedef typename Ops<DT>::T E;
    void* ws = nullptr;
    if (get_workspace(&ws, ((size_t)T * kernel_size * dim + (size_t)T * dim) * sizeof(E) + 1024)) return 1;
    E* col = (E*)ws;
    E* h = col + (size_t)T * kernel_size * dim;
    im2col_time_kernel<DT><<<1024, 256, 0, s>>>(col, hidden_f32, (const E*)enc, T, dim, kernel_size);
    OMX_LAUNCH_CHECK();
    if (Ops<DT>::gemm_relu(h, col, (const E*)conv_w, (const E*)conv_b, T, dim, kernel_size * dim, s)) return 1;
    alpha_head_kernel<DT><<<(T + 3) / 4, 256, 0, s>>>(alphas, h, (const E*)proj_w, (const E*)proj_b, T, dim);
    OMX_LAUNCH_CHECK();
    return 0;
}

// what omx_paraformer_decoder_stack hands a layer (all optional): norm1(x) already computed by the previous layer's last launch; this layer's
// k | v rows of the encoder output, projected for all layers at once; and the norm the NEXT consumer applies to `out`, to be left in next_h1
struct DecoderHandover {
    const void* h1_pre = nullptr;
    const void* kv_pre = nullptr; int64_t ld_kv = 0;
    const void* next_ln_w = nullptr; const void* next_ln_b = nullptr; void* next_h1 = nullptr;
};

template <int DT>
int decoder_layer_impl(void* out, const void* x, const void* enc, const omx_paraformer_decoder_weights* w, int N, int Ts, int dim, int enc_dim,
                       int heads, int ffn_dim, int kernel_size, omx_stream stream, const DecoderHandover& ho = DecoderHandover()) {
    typedef typename Ops<DT>::T E;
    hipStream_t s = (hipStream_t)stream;
    const size_t scores = Ops<DT>::score_elems(heads, N, Ts);
    const size_t need = ((size_t)N * (5 * (size_t)dim + 2 * (size_t)ffn_dim) + (size_t)Ts * 2 * dim + 1024) * sizeof(E) + scores * 4 + 64;
    void* ws = nullptr;
    if (get_workspace(&ws, need)) return 1;
    E* h = (E*)ws;                           // [N, dim]   scratch LN outputs
    E* ff = h + (size_t)N * dim;             // [N, ffn]
    E* ffn = ff + (size_t)N * ffn_dim;       // [N, ffn]   LN(ffn)
    E* tgt = ffn + (size_t)N * ffn_dim;      // [N, dim]
    E* x1 = tgt + (size_t)N * dim;           // [N, dim]   after the FSMN residual
    E* q = x1 + (size_t)N * dim;             // [N, dim]
    E* att = q + (size_t)N * dim;            // [N, dim]
    E* kv = att + (size_t)N * dim;           // [Ts, 2*dim]
    float* sc = reinterpret_cast<float*>(kv + (size_t)Ts * 2 * dim + 8);   // [heads, N, Ts] (f32 mode only)
    const E* xin = (const E*)x;
    const omx_dtype dt = (omx_dtype)DT;
    // tgt = down(LN_ffn(relu(up(norm1(x)))))                                                     (:1036-1042)
    const E* h1 = (const E*)ho.h1_pre;
    if (!h1) {
        if (omx_layer_norm(h, xin, w->norm1_w, w->norm1_b, N, dim, 1e-5f, dt, stream)) return 1;
        h1 = h;
    }
    bool fused = false;
    if constexpr (DT == OMX_FLOAT32) {
        if (fuse_f32_tails() && f32_tail_width_ok(ffn_dim) && f32_tail_width_ok(dim)) {
            // round 6: [up + bias + relu + LN_ffn] and [down + norm2] each finished by one launch after the product (f32_epilogue_ln_kernel)
            F32Tail t1; t1.bias = (const float*)w->ffn_up_b; t1.relu = 1; t1.ln_w = (const float*)w->ffn_norm_w; t1.ln_b = (const float*)w->ffn_norm_b; t1.ln_out = ffn;
            if (gemm_f32_with_tail(nullptr, h1, (const float*)w->ffn_up_w, N, ffn_dim, dim, t1, ff, s)) return 1;
            F32Tail t2; t2.ln_w = (const float*)w->norm2_w; t2.ln_b = (const float*)w->norm2_b; t2.ln_out = h;
            if (gemm_f32_with_tail(nullptr, ffn, (const float*)w->ffn_down_w, N, dim, ffn_dim, t2, tgt, s)) return 1;
            // x1 = x + (fsmn(norm2(tgt)) + norm2(tgt)) and norm3(x1) in one launch: the same tail over the rows of x (:1044-1049).  `q` holds
            // norm3(x1) until the projection below has read it
            F32Tail t3; t3.v = h; t3.ldv = dim; t3.fw = (const float*)w->fsmn_w; t3.ksize = kernel_size; t3.ln_w = (const float*)w->norm3_w;
            t3.ln_b = (const float*)w->norm3_b; t3.ln_out = att;
            if (launch_f32_tail(x1, xin, 1, N, dim, t3, s)) return 1;
            fused = true;
        }
    }
    const E* h3 = att;                       // norm3(x1): the fused path leaves it in `att` (free until the attention writes it)
    if (!fused) {
    if (Ops<DT>::gemm_relu(ff, h1, (const E*)w->ffn_up_w, (const E*)w->ffn_up_b, N, ffn_dim, dim, s)) return 1;
    if (omx_layer_norm(ffn, ff, w->ffn_norm_w, w->ffn_norm_b, N, ffn_dim, 1e-5f, dt, stream)) return 1;
    if (Ops<DT>::gemm(tgt, ffn, (const E*)w->ffn_down_w, nullptr, N, dim, ffn_dim, s)) return 1;
    // x1 = x + (fsmn(norm2(tgt)) + norm2(tgt))                                                   (:1044-1047)
    if (omx_layer_norm(h, tgt, w->norm2_w, w->norm2_b, N, dim, 1e-5f, dt, stream)) return 1;
    fsmn_add_kernel<DT, false><<<1024, 256, 0, s>>>(x1, xin, h, dim, (const E*)w->fsmn_w, N, dim, kernel_size, nullptr, SegTable{});
    OMX_LAUNCH_CHECK();
    if (omx_layer_norm(h, x1, w->norm3_w, w->norm3_b, N, dim, 1e-5f, dt, stream)) return 1;
    h3 = h;
    }
    // out = x1 + src_attn_out(softmax(q k^T * d^-1/2) v), q from norm3(x1), k/v from the encoder output      (:1049-1052, 981-1017)
    if (Ops<DT>::gemm(q, h3, (const E*)w->q_w, (const E*)w->q_b, N, dim, dim, s)) return 1;
    const E* kvp = (const E*)ho.kv_pre;
    int64_t ldkv = ho.ld_kv;
    if (!kvp) {
        if (Ops<DT>::gemm(kv, (const E*)enc, (const E*)w->kv_w, (const E*)w->kv_b, Ts, 2 * dim, enc_dim, s)) return 1;
        kvp = kv; ldkv = 2 * (int64_t)dim;
    }
    if (Ops<DT>::attention(att, q, kvp, kvp + dim, dim, ldkv, dim, N, Ts, heads, sc, s)) return 1;
    if constexpr (DT == OMX_FLOAT32) {
        if (fused) {
            // out = x1 + (out_proj(att) + bias) and the next consumer's norm of `out`, one launch behind the product
            F32Tail t4; t4.bias = (const float*)w->out_b; t4.resid = x1; t4.ldr = dim; t4.ln_w = (const float*)ho.next_ln_w; t4.ln_b = (const float*)ho.next_ln_b;
            t4.ln_out = (float*)ho.next_h1;
            return gemm_f32_with_tail((float*)out, att, (const float*)w->out_w, N, dim, dim, t4, nullptr, s);
        }
    }
    if (Ops<DT>::gemm_resid((E*)out, att, (const E*)w->out_w, (const E*)w->out_b, x1, N, dim, dim, s)) return 1;
    if (ho.next_h1) return omx_layer_norm(ho.next_h1, out, ho.next_ln_w, ho.next_ln_b, N, dim, 1e-5f, dt, stream);
    return 0;
}

template <int DT>
int decoder_tail_impl(void* logits, const void* x, const omx_paraformer_tail_weights* w, int N, int dim, int ffn_dim, int vocab, omx_stream stream) {
    typedef typename Ops<DT>::T E;
    hipStream_t s = (hipStream_t)stream;
    void* ws = nullptr;
    if (get_workspace(&ws, ((size_t)N * (2 * (size_t)dim + 2 * (size_t)ffn_dim) + 1024) * sizeof(E))) return 1;
    E* h = (E*)ws;
    E* ff = h + (size_t)N * dim;
    E* ffn = ff + (size_t)N * ffn_dim;
    E* t = ffn + (size_t)N * ffn_dim;
    const omx_dtype dt = (omx_dtype)DT;
    if (omx_layer_norm(h, x, w->norm1_w, w->norm1_b, N, dim, 1e-5f, dt, stream)) return 1;
    bool fused = false;
    if constexpr (DT == OMX_FLOAT32) {
        if (fuse_f32_tails() && f32_tail_width_ok(ffn_dim) && f32_tail_width_ok(dim)) {
            F32Tail t1; t1.bias = (const float*)w->up_b; t1.relu = 1; t1.ln_w = (const float*)w->ffn_norm_w; t1.ln_b = (const float*)w->ffn_norm_b; t1.ln_out = ffn;
            if (gemm_f32_with_tail(nullptr, h, (const float*)w->up_w, N, ffn_dim, dim, t1, ff, s)) return 1;
            F32Tail t2; t2.ln_w = (const float*)w->after_norm_w; t2.ln_b = (const float*)w->after_norm_b; t2.ln_out = h;
            if (gemm_f32_with_tail(nullptr, ffn, (const float*)w->down_w, N, dim, ffn_dim, t2, t, s)) return 1;
            fused = true;
        }
    }
    if (!fused) {
    if (Ops<DT>::gemm_relu(ff, h, (const E*)w->up_w, (const E*)w->up_b, N, ffn_dim, dim, s)) return 1;
    if (omx_layer_norm(ffn, ff, w->ffn_norm_w, w->ffn_norm_b, N, ffn_dim, 1e-5f, dt, stream)) return 1;
    if (Ops<DT>::gemm(t, ffn, (const E*)w->down_w, nullptr, N, dim, ffn_dim, s)) return 1;
    if (omx_layer_norm(h, t, w->after_norm_w, w->after_norm_b, N, dim, 1e-5f, dt, stream)) return 1;
    }
    return Ops<DT>::gemm((E*)logits, h, (const E*)w->out_w, (const E*)w->out_b, N, vocab, dim, s);
}

// h1_pre != null: norm1(x) was already computed (by the previous layer's last launch); next_ln_* / next_h1 != null: THIS layer's last launch
// also leaves LayerNorm(out) with those weights in next_h1 -- the next layer's norm1, or the encoder's after_norm (omx_sanm_encoder_stack)
template <int DT>
int encoder_layer_impl(void* out, const void* x, const omx_sanm_layer_weights* w, int T, int in_dim, int dim, int heads, int ffn_dim,
                       int kernel_size, omx_stream stream, const void* h1_pre = nullptr, const void* next_ln_w = nullptr,
                       const void* next_ln_b = nullptr, void* next_h1 = nullptr) {
    typedef typename Ops<DT>::T E;
    hipStream_t s = (hipStream_t)stream;
    const size_t scores = Ops<DT>::score_elems(heads, T, T);
    const size_t need = ((size_t)T * (in_dim + 3 * dim + 3 * dim + ffn_dim + dim) + 1024) * sizeof(E) + scores * 4 + 64;
    void* ws = nullptr;
    if (get_workspace(&ws, need)) return 1;
    E* h1 = (E*)ws;                          // [T, in_dim]  LN1(x)
    E* qkv = h1 + (size_t)T * in_dim;        // [T, 3*dim]
    E* att = qkv + (size_t)T * 3 * dim;      // [T, dim]
    E* prj = att + (size_t)T * dim;          // [T, dim]
    E* xr = prj + (size_t)T * dim;           // [T, dim]  x after the attention residual
    E* h2 = xr + (size_t)T * dim;            // [T, dim]  LN2
    E* ff = h2 + (size_t)T * dim;            // [T, ffn_dim]
    float* sc = reinterpret_cast<float*>(ff + (size_t)T * ffn_dim + 8);   // [heads, T, T] (f32 mode only)
    const E* xin = (const E*)x;
    const omx_dtype dt = (omx_dtype)DT;
    // h = norm1(x) ; qkv = linear_q_k_v(h)                                           (paraformer.rs:619, 500)
    if (h1_pre) h1 = (E*)h1_pre;
    else if (omx_layer_norm(h1, xin, w->norm1_w, w->norm1_b, T, in_dim, 1e-5f, dt, stream)) return 1;
    if (Ops<DT>::gemm(qkv, h1, (const E*)w->qkv_w, (const E*)w->qkv_b, T, 3 * dim, in_dim, s)) return 1;
    // softmax(q k^T * d^-1/2) v, 4 heads x 128, operands read in place from the fused projection    (:503-522)
    if (Ops<DT>::attention(att, qkv, qkv + dim, qkv + 2 * dim, 3 * (int64_t)dim, 3 * (int64_t)dim, dim, T, T, heads, sc, s)) return 1;
    bool fused = false;
    if constexpr (DT == OMX_FLOAT32) {
        if (fuse_f32_tails() && f32_tail_width_ok(dim)) {
            // round 6: out_proj's split-K sum + bias, the FSMN block, the layer residual and norm2 in ONE launch behind the product
            F32Tail t; t.bias = (const float*)w->out_b; t.v = qkv + 2 * dim; t.ldv = 3 * (int64_t)dim; t.fw = (const float*)w->fsmn_w; t.ksize = kernel_size;
            t.resid2 = in_dim == dim ? xin : nullptr; t.ln_w = (const float*)w->norm2_w; t.ln_b = (const float*)w->norm2_b; t.ln_out = h2;
            if (gemm_f32_with_tail(xr, att, (const float*)w->out_w, T, dim, dim, t, prj, s)) return 1;
            fused = true;
        }
    }
    if (!fused) {
    if (Ops<DT>::gemm(prj, att, (const E*)w->out_w, (const E*)w->out_b, T, dim, dim, s)) return 1;
    // out_proj(attn) + (fsmn_block(v) + v)                                             (:524-529)
    // + the layer residual in the same launch; only when the layer keeps its width (the first maps 560 -> 512 without it, :625-629)
    fsmn_add_kernel<DT, false><<<1024, 256, 0, s>>>(xr, prj, qkv + 2 * dim, 3 * (int64_t)dim, (const E*)w->fsmn_w, T, dim, kernel_size,
                                                    in_dim == dim ? xin : nullptr, SegTable{});
    OMX_LAUNCH_CHECK();
    if (omx_layer_norm(h2, xr, w->norm2_w, w->norm2_b, T, dim, 1e-5f, dt, stream)) return 1;
    }
    if (Ops<DT>::gemm_relu(ff, h2, (const E*)w->ffn_up_w, (const E*)w->ffn_up_b, T, ffn_dim, dim, s)) return 1;
    if constexpr (DT == OMX_FLOAT32) {
        if (next_h1 && fuse_f32_tails() && f32_tail_width_ok(dim)) {
            // out = xr + (ffn_down(ff) + bias) and the NEXT norm of `out`, one launch behind the product
            F32Tail t; t.bias = (const float*)w->ffn_down_b; t.resid = xr; t.ldr = dim; t.ln_w = (const float*)next_ln_w; t.ln_b = (const float*)next_ln_b;
            t.ln_out = (float*)next_h1;
            return gemm_f32_with_tail((float*)out, ff, (const float*)w->ffn_down_w, T, dim, ffn_dim, t, nullptr, s);
        }
    }
    // out = xr + (ffn_down(ff) + bias): the FFN residual in the GEMM epilogue
    if (Ops<DT>::gemm_resid((E*)out, ff, (const E*)w->ffn_down_w, (const E*)w->ffn_down_b, xr, T, dim, ffn_dim, s)) return 1;
    if (next_h1) return omx_layer_norm(next_h1, out, next_ln_w, next_ln_b, T, dim, 1e-5f, dt, stream);
    return 0;
}

}  // namespace
}  // namespace omx

extern "C" {

#define OMX_PARAFORMER_DT(dtype, CALL_BF16, CALL_F32)                                                                   \
    if ((dtype) == OMX_BFLOAT16) return CALL_BF16;                                                                        \
    if ((dtype) == OMX_FLOAT32) return CALL_F32;                                                                          \
    return omx::set_error("paraformer: dtype %d unsupported (float32 = the reference's arithmetic, bfloat16)", (int)(dtype));

int omx_paraformer_embed(void* out, const float* mel, int T, int dim, omx_dtype dtype, omx_stream stream) {
    OMX_REQUIRE(out && mel && T > 0 && dim >= 4 && dim % 2 == 0, "omx_paraformer_embed: bad arguments");
    if (dtype == OMX_BFLOAT16) omx::paraformer_embed_kernel<OMX_BFLOAT16><<<1024, 256, 0, (hipStream_t)stream>>>((omx::bf16_t*)out, mel, T, dim);
    else if (dtype == OMX_FLOAT32) omx::paraformer_embed_kernel<OMX_FLOAT32><<<1024, 256, 0, (hipStream_t)stream>>>((float*)out, mel, T, dim);
    else return omx::set_error("omx_paraformer_embed: dtype %d unsupported", (int)dtype);
    OMX_LAUNCH_CHECK();
    return 0;
}

int omx_cif_alphas(float* alphas, float* hidden_f32, const void* enc, const void* conv_w, const void* conv_b, const void* proj_w,
                   const void* proj_b, int T, int dim, int kernel_size, omx_dtype dtype, omx_stream stream) {
    OMX_REQUIRE(alphas && enc && conv_w && proj_w, "omx_cif_alphas: null argument");
    OMX_REQUIRE(T > 0 && dim % 64 == 0 && kernel_size % 2 == 1 && kernel_size <= 15, "omx_cif_alphas: bad shape");
    hipStream_t s = (hipStream_t)stream;
    OMX_PARAFORMER_DT(dtype, omx::cif_alphas_impl<OMX_BFLOAT16>(alphas, hidden_f32, enc, conv_w, conv_b, proj_w, proj_b, T, dim, kernel_size, s),
                      omx::cif_alphas_impl<OMX_FLOAT32>(alphas, hidden_f32, enc, conv_w, conv_b, proj_w, proj_b, T, dim, kernel_size, s))
}

/* The f32 model's attention on its own (paraformer.rs:509-516 / 1090-1102): out = softmax(q k^T / sqrt(128)) v per head of width 128, rows ld*
 * floats apart, head h at column 128 h.  One launch for Tk <= 512, GEMM + softmax + GEMM beyond. */
int omx_paraformer_attention_f32(float* out, const float* q, const float* k, const float* v, int64_t ldq, int64_t ldkv, int64_t ldo, int Tq,
                                 int Tk, int heads, omx_stream stream) {
    OMX_REQUIRE(out && q && k && v && Tq > 0 && Tk > 0 && heads > 0, "omx_paraformer_attention_f32: bad arguments");
    OMX_REQUIRE(ldq >= 128 * (int64_t)heads && ldkv >= 128 * (int64_t)heads && ldo >= 128 * (int64_t)heads, "omx_paraformer_attention_f32: rows shorter than heads x 128");
    void* ws = nullptr;
    if (omx::get_workspace(&ws, omx::Ops<OMX_FLOAT32>::score_elems(heads, Tq, Tk) * 4 + 64)) return 1;
    return omx::Ops<OMX_FLOAT32>::attention(out, q, k, v, ldq, ldkv, ldo, Tq, Tk, heads, (float*)ws, (hipStream_t)stream);
}

int omx_paraformer_decoder_layer(void* out, const void* x, const void* enc, const omx_paraformer_decoder_weights* w, int N, int Ts,
                                 int dim, int enc_dim, int heads, int ffn_dim, int kernel_size, omx_dtype dtype, omx_stream stream) {
    OMX_REQUIRE(out && x && enc && w, "omx_paraformer_decoder_layer: null argument");
    OMX_REQUIRE(N > 0 && Ts > 0 && dim % heads == 0 && dim / heads == 128, "omx_paraformer_decoder_layer: head_dim must be 128 (dim %d, heads %d)", dim, heads);
    OMX_REQUIRE(kernel_size % 2 == 1 && kernel_size <= 31, "omx_paraformer_decoder_layer: odd kernel_size <= 31 expected");
    OMX_PARAFORMER_DT(dtype, omx::decoder_layer_impl<OMX_BFLOAT16>(out, x, enc, w, N, Ts, dim, enc_dim, heads, ffn_dim, kernel_size, stream),
                      omx::decoder_layer_impl<OMX_FLOAT32>(out, x, enc, w, N, Ts, dim, enc_dim, heads, ffn_dim, kernel_size, stream))
}

/* ParaformerDecoder::forward's layer loop (paraformer.rs:1144-1156) in one call.  out [N, dim] = layers(x); scratch: two [N, dim] activations,
 * two [N, dim] normalised inputs the layers hand each other, and (optional) kv_all [Ts, n_layers * 2 * dim].  With kv_all and the layers'
 * linear_k_v weights / biases laid out back to back in memory (layer l's right behind layer l - 1's), the encoder output is projected for ALL
 * layers by one GEMM up front (it does not depend on the decoder state); otherwise each layer projects its own.  In float32 every layer's
 * last launch also computes the next layer's norm1. */
int omx_paraformer_decoder_stack(void* out, const void* x, const void* enc, const omx_paraformer_decoder_weights* layers, int n_layers, int N,
                                 int Ts, int dim, int enc_dim, int heads, int ffn_dim, int kernel_size, void* act0, void* act1, void* nrm0,
                                 void* nrm1, void* kv_all, omx_dtype dtype, omx_stream stream) {
    OMX_REQUIRE(out && x && enc && layers && n_layers > 0 && act0 && act1 && nrm0 && nrm1, "omx_paraformer_decoder_stack: null argument");
    OMX_REQUIRE(N > 0 && Ts > 0 && dim % heads == 0 && dim / heads == 128, "omx_paraformer_decoder_stack: head_dim must be 128 (dim %d, heads %d)", dim, heads);
    OMX_REQUIRE(kernel_size % 2 == 1 && kernel_size <= 31, "omx_paraformer_decoder_stack: odd kernel_size <= 31 expected");
    OMX_REQUIRE(dtype == OMX_BFLOAT16 || dtype == OMX_FLOAT32, "paraformer: dtype %d unsupported (float32 = the reference's arithmetic, bfloat16)", (int)dtype);
    const size_t esz = dtype == OMX_FLOAT32 ? 4 : 2;
    bool hoist = kv_all != nullptr;
    for (int l = 1; l < n_layers && hoist; ++l)
        hoist = (const char*)layers[l].kv_w == (const char*)layers[l - 1].kv_w + (size_t)2 * dim * enc_dim * esz &&
                (const char*)layers[l].kv_b == (const char*)layers[l - 1].kv_b + (size_t)2 * dim * esz;
    const int64_t ld_all = (int64_t)n_layers * 2 * dim;
    if (hoist) {
        const int rc = dtype == OMX_BFLOAT16
                           ? omx::Ops<OMX_BFLOAT16>::gemm((omx::bf16_t*)kv_all, (const omx::bf16_t*)enc, (const omx::bf16_t*)layers[0].kv_w,
                                                          (const omx::bf16_t*)layers[0].kv_b, Ts, (int)ld_all, enc_dim, (hipStream_t)stream)
                           : omx::Ops<OMX_FLOAT32>::gemm((float*)kv_all, (const float*)enc, (const float*)layers[0].kv_w, (const float*)layers[0].kv_b, Ts,
                                                         (int)ld_all, enc_dim, (hipStream_t)stream);
        if (rc) return 1;
    }
    void* act[2] = {act0, act1};
    void* nrm[2] = {nrm0, nrm1};
    const void* h = x;
    const void* pre = nullptr;
    for (int l = 0; l < n_layers; ++l) {
        const bool last = l + 1 == n_layers;
        void* o = last ? out : act[l & 1];
        omx::DecoderHandover ho;
        ho.h1_pre = pre;
        if (hoist) { ho.kv_pre = (const char*)kv_all + (size_t)l * 2 * dim * esz; ho.ld_kv = ld_all; }
        if (!last && dtype == OMX_FLOAT32 && omx::fuse_f32_tails()) {
            ho.next_ln_w = layers[l + 1].norm1_w; ho.next_ln_b = layers[l + 1].norm1_b; ho.next_h1 = nrm[l & 1];
        }
        const int rc = dtype == OMX_BFLOAT16
                           ? omx::decoder_layer_impl<OMX_BFLOAT16>(o, h, enc, &layers[l], N, Ts, dim, enc_dim, heads, ffn_dim, kernel_size, stream, ho)
                           : omx::decoder_layer_impl<OMX_FLOAT32>(o, h, enc, &layers[l], N, Ts, dim, enc_dim, heads, ffn_dim, kernel_size, stream, ho);
        if (rc) return 1;
        h = o; pre = ho.next_h1;
    }
    return 0;
}

int omx_paraformer_decoder_tail(void* logits, const void* x, const omx_paraformer_tail_weights* w, int N, int dim, int ffn_dim,
                                int vocab, omx_dtype dtype, omx_stream stream) {
    OMX_REQUIRE(logits && x && w && N > 0, "omx_paraformer_decoder_tail: bad arguments");
    OMX_PARAFORMER_DT(dtype, omx::decoder_tail_impl<OMX_BFLOAT16>(logits, x, w, N, dim, ffn_dim, vocab, stream),
                      omx::decoder_tail_impl<OMX_FLOAT32>(logits, x, w, N, dim, ffn_dim, vocab, stream))
}

/* SanmEncoder::forward's layer loop + after_norm (paraformer.rs:691-708) in one call: layer 0 maps in_dim -> dim, the others keep dim.
 * out [T, dim] = after_norm(layers(x)); scratch: two [T, dim] activations and two [T, max(in_dim, dim)] normalised inputs the layers hand each
 * other (the float32 mode computes every layer's norm1 -- and the final after_norm -- in the previous layer's last launch). */
int omx_sanm_encoder_stack(void* out, const void* x, const omx_sanm_layer_weights* layers, int n_layers, int T, int in_dim, int dim, int heads,
                           int ffn_dim, int kernel_size, const void* after_norm_w, const void* after_norm_b, void* act0, void* act1, void* nrm0,
                           void* nrm1, omx_dtype dtype, omx_stream stream) {
    OMX_REQUIRE(out && x && layers && n_layers > 0 && act0 && act1 && nrm0 && nrm1 && after_norm_w && after_norm_b, "omx_sanm_encoder_stack: null argument");
    OMX_REQUIRE(T > 0 && dim % heads == 0 && dim / heads == 128, "omx_sanm_encoder_stack: head_dim must be 128 (dim %d, heads %d)", dim, heads);
    OMX_REQUIRE(kernel_size % 2 == 1 && kernel_size <= 31, "omx_sanm_encoder_stack: odd kernel_size <= 31 expected");
    OMX_REQUIRE(dtype == OMX_BFLOAT16 || dtype == OMX_FLOAT32, "paraformer: dtype %d unsupported (float32 = the reference's arithmetic, bfloat16)", (int)dtype);
    void* act[2] = {act0, act1};
    void* nrm[2] = {nrm0, nrm1};
    const void* h = x;
    const void* pre = nullptr;
    int d_in = in_dim;
    for (int l = 0; l < n_layers; ++l) {
        const bool last = l + 1 == n_layers;
        void* o = act[l & 1];
        const void* nw = last ? after_norm_w : layers[l + 1].norm1_w;
        const void* nb = last ? after_norm_b : layers[l + 1].norm1_b;
        void* nh = last ? out : nrm[l & 1];
        const int rc = dtype == OMX_BFLOAT16
                           ? omx::encoder_layer_impl<OMX_BFLOAT16>(o, h, &layers[l], T, d_in, dim, heads, ffn_dim, kernel_size, stream, pre, nw, nb, nh)
                           : omx::encoder_layer_impl<OMX_FLOAT32>(o, h, &layers[l], T, d_in, dim, heads, ffn_dim, kernel_size, stream, pre, nw, nb, nh);
        if (rc) return 1;
        h = o; pre = nh; d_in = dim;
    }
    return 0;
}

int omx_sanm_encoder_layer(void* out, const void* x, const omx_sanm_layer_weights* w, int T, int in_dim, int dim,
                           int heads, int ffn_dim, int kernel_size, omx_dtype dtype, omx_stream stream) {
    OMX_REQUIRE(out && x && w, "omx_sanm_encoder_layer: null argument");
    OMX_REQUIRE(T > 0 && dim % heads == 0 && dim / heads == 128, "omx_sanm_encoder_layer: head_dim must be 128 (dim %d, heads %d)", dim, heads);
    OMX_REQUIRE(kernel_size % 2 == 1 && kernel_size <= 31, "omx_sanm_encoder_layer: odd kernel_size <= 31 expected");
    OMX_PARAFORMER_DT(dtype, omx::encoder_layer_impl<OMX_BFLOAT16>(out, x, w, T, in_dim, dim, heads, ffn_dim, kernel_size, stream),
                      omx::encoder_layer_impl<OMX_FLOAT32>(out, x, w, T, in_dim, dim, heads, ffn_dim, kernel_size, stream))
}

int omx_cif_fire(float* frames, int* counts, const float* hidden, const float* alphas, int batch, int T, int H,
                 float threshold, float tail_threshold, int max_frames, omx_stream stream) {
    OMX_REQUIRE(frames && counts && hidden && alphas, "omx_cif_fire: null argument");
    OMX_REQUIRE(batch > 0 && T > 0 && H > 0 && max_frames > 0, "omx_cif_fire: bad shape");
    OMX_HIP_CHECK(hipMemsetAsync(frames, 0, (size_t)batch * max_frames * H * 4, (hipStream_t)stream));
    const size_t lds = (size_t)T * 4 + (size_t)max_frames * 8;
    OMX_REQUIRE(lds <= 160 * 1024 - 64, "omx_cif_fire: %d steps / %d frames exceed the LDS tables (%zu bytes)", T, max_frames, lds);
    static bool attr_set = false;
    if (!attr_set) {
        OMX_HIP_CHECK(hipFuncSetAttribute((const void*)omx::cif_fire_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 64));
        attr_set = true;
    }
    omx::cif_fire_kernel<<<dim3(batch, 32), 256, lds, (hipStream_t)stream>>>(hidden, alphas, T, H, threshold, tail_threshold, frames,
                                                                            max_frames, counts);
    OMX_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
