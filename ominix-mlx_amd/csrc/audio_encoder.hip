// The Qwen3-ASR audio tower (qwen3-asr-mlx/src/encoder.rs:254-458) in float32: the reference feeds a float32 mel into bf16 parameters
// that are never quantised (model.rs:305), and MLX promotes every op of the tower to float32 -- so the weights are widened once at
// load (the caller hands float32) and every launch below is float32, as the Paraformer path's are.
//   mel [n_mels, F] -> chunks of 2 * n_window frames, zero-padded to the longest -> three 3x3 stride-2 convolutions + GELU (NHWC;
//   layer 1 direct, layers 2 / 3 im2col per group of chunks + the float32 matrix-core GEMM) -> [chunks, t, ds * f] rows -> conv_out
//   -> + sinusoid of the position WITHIN the chunk, valid rows compacted to [N, d_model] -> pre-norm transformer layers whose
//   attention runs inside windows of `window` rows (the reference's [N, N] additive -1e9 mask, never materialised) -> ln_post,
//   proj1 + GELU, proj2 -> [N, output_dim].
#include <math.h>

#include <map>
#include <string>
#include <vector>

#include "gemm.hpp"

namespace {

using namespace omx;

// nn::gelu (mlx-rs/src/nn/activation.rs:164): the exact form x * (1 + erf(x / sqrt 2)) / 2
__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }

__global__ void scale_kernel(float* __restrict__ x, int64_t n, float a) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) x[i] *= a;
}

__global__ void gelu_kernel(float* __restrict__ x, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) x[i] = gelu_erf(x[i]);
}

// flag[0] |= 1 where the mel holds a NaN or an infinity
__global__ void nonfinite_kernel(const float* __restrict__ x, int64_t n, int* __restrict__ flag) {
    bool bad = false;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) bad |= !(fabsf(x[i]) <= 3.4028234e38f);
    if (bad) atomicOr(flag, 1);
}

// conv2d1 + GELU straight from the mel: out [C, H1, W1, ds] (NHWC, H = mel bin, W = frame within the chunk).  Chunk c covers frames
// [c * chunk, c * chunk + Wp) of which the ones at or past F are the zero padding; the padded frames are convolved like real ones.
__global__ void conv1_gelu_kernel(float* __restrict__ out, const float* __restrict__ mel, const float* __restrict__ w, const float* __restrict__ b,
                                  int n_mels, int F, int chunk, int Wp, int C, int H1, int W1, int ds) {
    const int64_t n = (int64_t)C * H1 * W1 * ds;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int oc = (int)(i % ds), ow = (int)((i / ds) % W1), oh = (int)((i / ((int64_t)ds * W1)) % H1), c = (int)(i / ((int64_t)ds * W1 * H1));
        float acc = b[oc];
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
            const int ih = 2 * oh - 1 + kh;
            if (ih < 0 || ih >= n_mels) continue;
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int iw = 2 * ow - 1 + kw;
                if (iw < 0 || iw >= Wp) continue;
                const int64_t fr = (int64_t)c * chunk + iw;
                const float x = fr < F ? mel[(int64_t)ih * F + fr] : 0.f;
                acc += w[(oc * 3 + kh) * 3 + kw] * x;
            }
        }
        out[i] = gelu_erf(acc);
    }
}

// im2col of a 3x3 stride-2 pad-1 convolution over NHWC x [C, H, W, ch]: A [C * OH * OW, 9 * ch], k = (kh * 3 + kw) * ch + ic -- the
// order of a weight [out, 3, 3, in] read as [out, 9 * in].  ch % 4 == 0: one float4 per thread and step.
__global__ void im2col_kernel(float* __restrict__ A, const float* __restrict__ x, int C, int H, int W, int ch, int OH, int OW) {
    const int q = ch / 4;
    const int64_t n = (int64_t)C * OH * OW * 9 * q;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int iq = (int)(i % q), tap = (int)((i / q) % 9);
        const int64_t row = i / ((int64_t)q * 9);
        const int ow = (int)(row % OW), oh = (int)((row / OW) % OH), c = (int)(row / ((int64_t)OW * OH));
        const int ih = 2 * oh - 1 + tap / 3, iw = 2 * ow - 1 + tap % 3;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (ih >= 0 && ih < H && iw >= 0 && iw < W) v = *reinterpret_cast<const f32x4*>(x + (((int64_t)c * H + ih) * W + iw) * ch + iq * 4);
        *reinterpret_cast<f32x4*>(A + row * 9 * ch + (int64_t)tap * ch + iq * 4) = v;
    }
}

// encoder.rs:376-377: x [C, f, t, ch] -> rows [C * t, ch * f], column = channel * f_n + frequency
__global__ void rows_kernel(float* __restrict__ out, const float* __restrict__ x, int C, int Fq, int T, int ch) {
    const int64_t n = (int64_t)C * Fq * T * ch;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int f = (int)(i % Fq), k = (int)((i / Fq) % ch), t = (int)((i / ((int64_t)Fq * ch)) % T), c = (int)(i / ((int64_t)Fq * ch * T));
        out[i] = x[(((int64_t)c * Fq + f) * T + t) * ch + k];
    }
}

// + the sinusoid row of the position within the chunk, and the valid rows of every chunk compacted: chunk c's rows [0, valid_c) go to
// rows [c * full, ...) of out -- every chunk but the last is full (`full` valid rows), so the offsets need no table
__global__ void pos_compact_kernel(float* __restrict__ out, const float* __restrict__ y, const float* __restrict__ pos, int N, int full, int T, int d) {
    const int64_t n = (int64_t)N * d;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int col = (int)(i % d), r = (int)(i / d), c = r / full, t = r % full;
        out[i] = y[((int64_t)c * T + t) * d + col] + pos[(int64_t)t * d + col];
    }
}

// Attention inside windows, head width 64, float32: block (query tile of 16 rows, head, window).  The window's K (rows 65 floats apart:
// lane j reads key j's row without a bank conflict) and V lie in LDS; a wave takes one query row at a time -- lane j scores keys j and
// j + 64, the row's maximum and sum go through the wave, lane d then sums p_j * V[j][d].  q is pre-scaled (q rows of the stacked
// projection carry head_dim^-0.5), the scale here is 1, as in the reference.  Keys outside the window would add exp(-1e9 - max) = 0
// in float32: they are not read.  q | k | v are read in place (row stride ld, head h at column 64 h), out is token-major.
constexpr int AW_D = 64, AW_KLD = 65, AW_QROWS = 16, AW_MAXW = 128;
__global__ __launch_bounds__(256) void window_attn_kernel(float* __restrict__ out, int64_t ldo, const float* __restrict__ q, const float* __restrict__ k,
                                                          const float* __restrict__ v, int64_t ld, int N, int window) {
    extern __shared__ float lds[];
    const int w0 = blockIdx.z * window, wlen = min(window, N - w0), h = blockIdx.y, q0 = blockIdx.x * AW_QROWS;
    if (q0 >= wlen) return;
    float* Ks = lds;                               // [window][65]
    float* Vs = Ks + (size_t)window * AW_KLD;      // [window][64]
    float* Ps = Vs + (size_t)window * AW_D;        // [4 waves][AW_MAXW]
    float* Qs = Ps + 4 * AW_MAXW;                  // [4 waves][64]
    for (int i = threadIdx.x; i < wlen * AW_D; i += 256) {
        const int j = i / AW_D, d = i % AW_D;
        Ks[j * AW_KLD + d] = k[(int64_t)(w0 + j) * ld + h * AW_D + d];
        Vs[j * AW_D + d] = v[(int64_t)(w0 + j) * ld + h * AW_D + d];
    }
    __syncthreads();
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    float* P = Ps + wave * AW_MAXW;
    float* Q = Qs + wave * AW_D;
    for (int r = q0 + wave; r < min(q0 + AW_QROWS, wlen); r += 4) {
        Q[lane] = q[(int64_t)(w0 + r) * ld + h * AW_D + lane];
        __builtin_amdgcn_wave_barrier();
        float s0 = -INFINITY, s1 = -INFINITY;
        if (lane < wlen) {
            float a = 0.f;
            for (int d = 0; d < AW_D; ++d) a += Q[d] * Ks[lane * AW_KLD + d];
            s0 = a;
        }
        if (lane + 64 < wlen) {
            float a = 0.f;
            for (int d = 0; d < AW_D; ++d) a += Q[d] * Ks[(lane + 64) * AW_KLD + d];
            s1 = a;
        }
        float m = fmaxf(s0, s1);
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        const float p0 = lane < wlen ? expf(s0 - m) : 0.f, p1 = lane + 64 < wlen ? expf(s1 - m) : 0.f;
        float sum = p0 + p1;
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
        P[lane] = p0;
        P[lane + 64] = p1;
        __builtin_amdgcn_wave_barrier();
        float acc = 0.f;
        for (int j = 0; j < wlen; ++j) acc += P[j] * Vs[j * AW_D + lane];
        out[(int64_t)(w0 + r) * ldo + h * AW_D + lane] = acc / sum;
        __builtin_amdgcn_wave_barrier();
    }
}

inline size_t window_attn_lds(int window) { return ((size_t)window * (AW_KLD + AW_D) + 4 * AW_MAXW + 4 * AW_D) * sizeof(float); }

inline unsigned grid_for(int64_t n) { return (unsigned)std::min<int64_t>((n + 255) / 256, 8192); }

// get_feat_extract_output_lengths (encoder.rs:76-80) with the FLOOR division of the model's own definition: a remainder of 0 frames makes
// 0 rows, so 100 frames make the 13 rows the convolutions make.  (The reference's i32 division truncates, (0 - 1) / 2 = 0, which gives a
// full chunk 14 "valid" rows of the 13 that exist and with that windows of 112 rows instead of 104: DESIGN 4.12.)
inline int floor_half(int x) { return x >= 0 ? x / 2 : -((1 - x) / 2); }
inline int feat_len(int n, int chunk, int per_chunk) {
    const int leave = n % chunk, f = floor_half(leave - 1) + 1;
    return floor_half(floor_half(f - 1) + 1 - 1) + 1 + (n / chunk) * per_chunk;
}

inline int conv_out_len(int n) { return (n + 2 - 3) / 2 + 1; }

int launch_window_attn_f32(float* out, int64_t ldo, const float* q, const float* k, const float* v, int64_t ld, int N, int heads, int window,
                           hipStream_t s) {
    OMX_REQUIRE(out && q && k && v && N >= 1 && heads >= 1, "window attention: bad arguments (N=%d heads=%d)", N, heads);
    OMX_REQUIRE(window >= 1 && window <= AW_MAXW && window_attn_lds(window) <= 64 * 1024,
                "InvalidConfig: window attention: a window of %d rows does not fit the kernel (K and V of a window in 64 KB of LDS: at most 118 rows)", window);
    OMX_REQUIRE(ld >= heads * AW_D && ldo >= heads * AW_D, "window attention: leading dimensions %lld / %lld below heads * 64", (long long)ld, (long long)ldo);
    static const bool lds_ok = hipFuncSetAttribute((const void*)window_attn_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024) == hipSuccess;
    OMX_REQUIRE(lds_ok, "window attention: the device refused 64 KB of LDS per block");
    const int nwin = (N + window - 1) / window, qtiles = (std::min(window, N) + AW_QROWS - 1) / AW_QROWS;
    window_attn_kernel<<<dim3(qtiles, heads, nwin), 256, window_attn_lds(window), s>>>(out, ldo, q, k, v, ld, N, window);
    OMX_LAUNCH_CHECK();
    return 0;
}

}  // namespace

struct omx_qwen3_asr_encoder_ {
    omx_qwen3_asr_encoder_config cfg;
    int chunk, head_dim, f3;                      // frames per chunk, head width, mel bins after the stem
    std::map<std::string, float*> w;              // device float32 tensors by name (the keys behind "audio_tower.")
    std::map<std::string, size_t> wn;             // ... and their element counts
    std::vector<float*> qkv_w, qkv_b;             // per layer: q | k | v stacked [3 d, d] / [3 d], the q part scaled by head_dim^-0.5
    float* pos = nullptr;                         // [max_source_positions, d_model]
    int* flag = nullptr;
    // scratch, grown per role
    float* buf[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    size_t cap[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

namespace {

enum { B_X1 = 0, B_X2, B_X3, B_COL, B_ROWS, B_H, B_T0, B_T1 };

int reserve(omx_qwen3_asr_encoder e, int role, size_t elems, hipStream_t s) {
    if (elems <= e->cap[role]) return 0;
    OMX_HIP_CHECK(hipStreamSynchronize(s));
    if (e->buf[role]) OMX_HIP_CHECK(hipFree(e->buf[role]));
    e->buf[role] = nullptr; e->cap[role] = 0;
    OMX_HIP_CHECK(hipMalloc((void**)&e->buf[role], elems * sizeof(float)));
    e->cap[role] = elems;
    return 0;
}

const float* weight(omx_qwen3_asr_encoder e, const std::string& name, size_t want, int* err) {
    if (*err) return nullptr;                     // the first missing or misshapen tensor is the one reported
    auto it = e->w.find(name);
    if (it == e->w.end()) { *err = omx::set_error("WeightNotFound: audio_tower.%s", name.c_str()); return nullptr; }
    if (e->wn[name] != want) { *err = omx::set_error("ShapeMismatch: audio_tower.%s has %zu elements, the config expects %zu", name.c_str(), e->wn[name], want); return nullptr; }
    return it->second;
}

int gemm(float* out, const float* a, const float* w, const float* bias, const float* resid, int M, int N, int K, hipStream_t s) {
    GemmF32 g = {};
    g.a = a; g.b = w; g.bias = bias; g.resid = resid; g.out = out;
    g.M = M; g.N = N; g.K = K; g.lda = K; g.ldb = K; g.ldc = N; g.ldr = N;
    g.batch = 1; g.alpha = 1.0f;
    return launch_gemm_f32(g, s);
}

int gelu(float* x, int64_t n, hipStream_t s) {
    gelu_kernel<<<grid_for(n), 256, 0, s>>>(x, n);
    OMX_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" {

int omx_qwen3_asr_encoder_create(omx_qwen3_asr_encoder* out, const omx_qwen3_asr_encoder_config* cfg) {
    OMX_REQUIRE(out && cfg, "omx_qwen3_asr_encoder_create: null argument");
    const omx_qwen3_asr_encoder_config& c = *cfg;
    OMX_REQUIRE(c.n_mels >= 1 && c.n_layers >= 0 && c.n_heads >= 1 && c.ffn_dim >= 4 && c.d_model >= 4 && c.output_dim >= 1 && c.n_window >= 1 &&
                c.max_source_positions >= 1 && c.downsample_hidden_size >= 4,
                "InvalidConfig: qwen3-asr encoder n_mels=%d layers=%d heads=%d ffn=%d d_model=%d", c.n_mels, c.n_layers, c.n_heads, c.ffn_dim, c.d_model);
    OMX_REQUIRE(c.d_model % 64 == 0, "InvalidConfig: qwen3-asr encoder d_model %d must be a multiple of 64", c.d_model);
    OMX_REQUIRE(c.d_model == c.n_heads * 64, "InvalidConfig: qwen3-asr encoder head width %d (d_model %d / %d heads): the attention kernel is built for 64",
                c.d_model / c.n_heads, c.d_model, c.n_heads);
    OMX_REQUIRE(c.n_window_infer >= 2 * c.n_window && c.n_window_infer % (2 * c.n_window) == 0,
                "InvalidConfig: qwen3-asr encoder n_window_infer %d must be a multiple of the chunk, 2 * n_window = %d", c.n_window_infer, 2 * c.n_window);
    OMX_REQUIRE(c.downsample_hidden_size % 4 == 0 && c.ffn_dim % 4 == 0 && c.output_dim % 4 == 0,
                "InvalidConfig: qwen3-asr encoder widths must be multiples of 4 (ds %d, ffn %d, output %d)", c.downsample_hidden_size, c.ffn_dim, c.output_dim);
    const int chunk = 2 * c.n_window;
    const int per_chunk = conv_out_len(conv_out_len(conv_out_len(chunk)));
    OMX_REQUIRE(per_chunk <= c.max_source_positions, "InvalidConfig: qwen3-asr encoder: a chunk makes %d rows, max_source_positions is %d", per_chunk, c.max_source_positions);
    const int window = per_chunk * (c.n_window_infer / chunk);
    OMX_REQUIRE(window <= AW_MAXW && window_attn_lds(window) <= 64 * 1024,
                "InvalidConfig: qwen3-asr encoder: attention windows of %d rows (%d per chunk x %d chunks) exceed the kernel's 118", window, per_chunk, c.n_window_infer / chunk);
    omx_qwen3_asr_encoder e = new omx_qwen3_asr_encoder_();
    e->cfg = c;
    e->chunk = chunk;
    e->head_dim = 64;
    e->f3 = conv_out_len(conv_out_len(conv_out_len(c.n_mels)));
    // SinusoidalPositionEmbedding::new (encoder.rs:89-105), float32 as the reference computes it
    const int d = c.d_model, half = d / 2;
    std::vector<float> pos((size_t)c.max_source_positions * d, 0.f);
    const float log_timescale = logf(10000.0f) / (float)(half - 1);
    for (int p = 0; p < c.max_source_positions; ++p)
        for (int i = 0; i < half; ++i) {
            const float scaled = (float)p * expf(-log_timescale * (float)i);
            pos[(size_t)p * d + i] = sinf(scaled);
            pos[(size_t)p * d + half + i] = cosf(scaled);
        }
    if (hipMalloc((void**)&e->pos, pos.size() * sizeof(float)) != hipSuccess || hipMalloc((void**)&e->flag, sizeof(int)) != hipSuccess ||
        hipMemcpy(e->pos, pos.data(), pos.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        omx_qwen3_asr_encoder_destroy(e);
        return omx::set_error("omx_qwen3_asr_encoder_create: device allocation failed");
    }
    e->qkv_w.assign(c.n_layers, nullptr);
    e->qkv_b.assign(c.n_layers, nullptr);
    *out = e;
    return 0;
}

int omx_qwen3_asr_encoder_destroy(omx_qwen3_asr_encoder e) {
    if (!e) return 0;
    (void)hipDeviceSynchronize();
    for (auto& kv : e->w) (void)hipFree(kv.second);
    for (float* p : e->qkv_w) if (p) (void)hipFree(p);
    for (float* p : e->qkv_b) if (p) (void)hipFree(p);
    for (float* p : e->buf) if (p) (void)hipFree(p);
    if (e->pos) (void)hipFree(e->pos);
    if (e->flag) (void)hipFree(e->flag);
    delete e;
    return 0;
}

/* one tensor of the checkpoint, float32 on the HOST (the bf16 parameters widened by the caller), by its key behind "audio_tower."; the
 * shape is checked against the config when the tensor is first used */
int omx_qwen3_asr_encoder_load(omx_qwen3_asr_encoder e, const char* name, const float* host, const int64_t* shape, int ndim) {
    OMX_REQUIRE(e && name && host && shape && ndim >= 1 && ndim <= 4, "omx_qwen3_asr_encoder_load: bad argument");
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) { OMX_REQUIRE(shape[i] >= 1, "omx_qwen3_asr_encoder_load: %s: empty dimension", name); n *= (size_t)shape[i]; }
    const std::string key(name);
    auto it = e->w.find(key);
    if (it != e->w.end()) { (void)hipFree(it->second); e->w.erase(it); }
    float* dev = nullptr;
    OMX_HIP_CHECK(hipMalloc((void**)&dev, n * sizeof(float)));
    OMX_HIP_CHECK(hipMemcpy(dev, host, n * sizeof(float), hipMemcpyHostToDevice));
    e->w[key] = dev;
    e->wn[key] = n;
    // a q / k / v projection changed: the layer's stacked copy is rebuilt at the next forward
    for (int l = 0; l < e->cfg.n_layers; ++l)
        if (key.rfind("layers." + std::to_string(l) + ".self_attn.", 0) == 0 && e->qkv_w[l]) {
            (void)hipFree(e->qkv_w[l]); (void)hipFree(e->qkv_b[l]);
            e->qkv_w[l] = e->qkv_b[l] = nullptr;
        }
    return 0;
}

/* rows the tower makes of a mel of n_frames frames: get_feat_extract_output_lengths (encoder.rs:76-80) */
int omx_qwen3_asr_encoder_tokens(omx_qwen3_asr_encoder e, int n_frames, int* n) {
    OMX_REQUIRE(e && n, "omx_qwen3_asr_encoder_tokens: null argument");
    OMX_REQUIRE(n_frames >= 1, "omx_qwen3_asr_encoder_tokens: %d frames", n_frames);
    *n = feat_len(n_frames, e->chunk, conv_out_len(conv_out_len(conv_out_len(e->chunk))));
    return 0;
}

/* AudioEncoder::forward_encoder (encoder.rs:303-436): mel (DEVICE f32 [n_mels, n_frames]) -> out_rows (DEVICE f32 [N, output_dim]),
 * N = omx_qwen3_asr_encoder_tokens(n_frames).  Runs on `stream`; returns after the work is enqueued, except for one read-back of the
 * NaN flag of the mel at the start. */
int omx_qwen3_asr_encoder_forward(omx_qwen3_asr_encoder e, const float* mel, int n_frames, float* out_rows, omx_stream stream) {
    OMX_REQUIRE(e && mel && out_rows, "omx_qwen3_asr_encoder_forward: null argument");
    OMX_REQUIRE(n_frames >= 1, "omx_qwen3_asr_encoder_forward: %d frames", n_frames);
    hipStream_t s = (hipStream_t)stream;
    const omx_qwen3_asr_encoder_config& c = e->cfg;
    const int F = n_frames, chunk = e->chunk, ds = c.downsample_hidden_size, d = c.d_model, ffn = c.ffn_dim;
    const int C = (F + chunk - 1) / chunk, Wp = C > 1 ? chunk : F;                     // chunks, and the length every chunk is padded to
    const int H1 = conv_out_len(c.n_mels), H2 = conv_out_len(H1), H3 = conv_out_len(H2);
    const int W1 = conv_out_len(Wp), W2 = conv_out_len(W1), W3 = conv_out_len(W2);
    const int per_chunk = conv_out_len(conv_out_len(conv_out_len(chunk)));
    const int N = feat_len(F, chunk, per_chunk);
    // rows per chunk: `per_chunk` for every full chunk; the compaction's c = r / full needs a row count that is the same for all chunks
    // but the last
    const int full = C > 1 ? per_chunk : N;
    const int max_len = C > 1 ? per_chunk : N;                                         // max_len_after_cnn
    const int window = max_len * (c.n_window_infer / chunk);
    OMX_REQUIRE(max_len <= W3, "omx_qwen3_asr_encoder_forward: %d valid rows per chunk but the stem makes %d", max_len, W3);
    OMX_REQUIRE(max_len <= c.max_source_positions, "InvalidConfig: qwen3-asr encoder: %d rows per chunk exceed max_source_positions %d", max_len, c.max_source_positions);
    OMX_REQUIRE(N >= 1, "omx_qwen3_asr_encoder_forward: %d frames make no row", F);

    OMX_HIP_CHECK(hipMemsetAsync(e->flag, 0, sizeof(int), s));
    nonfinite_kernel<<<grid_for((int64_t)c.n_mels * F), 256, 0, s>>>(mel, (int64_t)c.n_mels * F, e->flag);
    OMX_LAUNCH_CHECK();
    int bad = 0;
    OMX_HIP_CHECK(hipMemcpyAsync(&bad, e->flag, sizeof(int), hipMemcpyDeviceToHost, s));
    OMX_HIP_CHECK(hipStreamSynchronize(s));
    OMX_REQUIRE(!bad, "omx_qwen3_asr_encoder_forward: the mel holds a NaN or an infinity");

    int err = 0;
    auto W = [&](const std::string& name, size_t want) { return weight(e, name, want, &err); };
    const float* c1w = W("conv2d1.weight", (size_t)ds * 9);   const float* c1b = W("conv2d1.bias", ds);
    const float* c2w = W("conv2d2.weight", (size_t)ds * 9 * ds); const float* c2b = W("conv2d2.bias", ds);
    const float* c3w = W("conv2d3.weight", (size_t)ds * 9 * ds); const float* c3b = W("conv2d3.bias", ds);
    const float* cow = W("conv_out.weight", (size_t)d * ds * H3);
    const float* lnw = W("ln_post.weight", d); const float* lnb = W("ln_post.bias", d);
    const float* p1w = W("proj1.weight", (size_t)d * d); const float* p1b = W("proj1.bias", d);
    const float* p2w = W("proj2.weight", (size_t)c.output_dim * d); const float* p2b = W("proj2.bias", c.output_dim);
    if (err) return 1;
    OMX_REQUIRE(H3 == e->f3, "omx_qwen3_asr_encoder_forward: internal: %d mel bins after the stem, %d expected", H3, e->f3);

    // ---- stem ----
    // im2col scratch bounded per group of chunks: <= ~64 MB whatever the clip length (30 s at the real widths would need 415 MB at once)
    const size_t col_budget = (size_t)16 << 20;                                        // floats
    const int g2 = std::max<int>(1, (int)std::min<size_t>(C, col_budget / ((size_t)H2 * W2 * 9 * ds)));
    const int g3 = std::max<int>(1, (int)std::min<size_t>(C, col_budget / ((size_t)H3 * W3 * 9 * ds)));
    if (reserve(e, B_X1, (size_t)C * H1 * W1 * ds, s) || reserve(e, B_X2, (size_t)C * H2 * W2 * ds, s) || reserve(e, B_X3, (size_t)C * H3 * W3 * ds, s) ||
        reserve(e, B_COL, std::max((size_t)g2 * H2 * W2, (size_t)g3 * H3 * W3) * 9 * ds, s) || reserve(e, B_ROWS, (size_t)C * W3 * ds * H3, s) ||
        reserve(e, B_H, (size_t)N * d, s) || reserve(e, B_T0, std::max((size_t)N * std::max(3 * d, ffn), (size_t)C * W3 * d), s) ||
        reserve(e, B_T1, (size_t)N * d, s))
        return 1;
    float *x1 = e->buf[B_X1], *x2 = e->buf[B_X2], *x3 = e->buf[B_X3], *col = e->buf[B_COL], *rows = e->buf[B_ROWS], *h = e->buf[B_H],
          *t0 = e->buf[B_T0], *t1 = e->buf[B_T1];
    conv1_gelu_kernel<<<grid_for((int64_t)C * H1 * W1 * ds), 256, 0, s>>>(x1, mel, c1w, c1b, c.n_mels, F, chunk, Wp, C, H1, W1, ds);
    OMX_LAUNCH_CHECK();
    for (int c0 = 0; c0 < C; c0 += g2) {
        const int g = std::min(g2, C - c0), M = g * H2 * W2;
        im2col_kernel<<<grid_for((int64_t)M * 9 * ds / 4), 256, 0, s>>>(col, x1 + (size_t)c0 * H1 * W1 * ds, g, H1, W1, ds, H2, W2);
        OMX_LAUNCH_CHECK();
        float* y = x2 + (size_t)c0 * H2 * W2 * ds;
        if (gemm(y, col, c2w, c2b, nullptr, M, ds, 9 * ds, s) || gelu(y, (int64_t)M * ds, s)) return 1;
    }
    for (int c0 = 0; c0 < C; c0 += g3) {
        const int g = std::min(g3, C - c0), M = g * H3 * W3;
        im2col_kernel<<<grid_for((int64_t)M * 9 * ds / 4), 256, 0, s>>>(col, x2 + (size_t)c0 * H2 * W2 * ds, g, H2, W2, ds, H3, W3);
        OMX_LAUNCH_CHECK();
        float* y = x3 + (size_t)c0 * H3 * W3 * ds;
        if (gemm(y, col, c3w, c3b, nullptr, M, ds, 9 * ds, s) || gelu(y, (int64_t)M * ds, s)) return 1;
    }
    // ---- rows: [C, t, ds * f] -> conv_out -> + position within the chunk, valid rows compacted ----
    rows_kernel<<<grid_for((int64_t)C * H3 * W3 * ds), 256, 0, s>>>(rows, x3, C, H3, W3, ds);
    OMX_LAUNCH_CHECK();
    if (gemm(t0, rows, cow, nullptr, nullptr, C * W3, d, ds * H3, s)) return 1;
    pos_compact_kernel<<<grid_for((int64_t)N * d), 256, 0, s>>>(h, t0, e->pos, N, full, W3, d);
    OMX_LAUNCH_CHECK();

    // ---- transformer layers ----
    for (int l = 0; l < c.n_layers; ++l) {
        const std::string p = "layers." + std::to_string(l) + ".";
        const float* n1w = W(p + "self_attn_layer_norm.weight", d); const float* n1b = W(p + "self_attn_layer_norm.bias", d);
        const float* ow = W(p + "self_attn.out_proj.weight", (size_t)d * d); const float* ob = W(p + "self_attn.out_proj.bias", d);
        const float* n2w = W(p + "final_layer_norm.weight", d); const float* n2b = W(p + "final_layer_norm.bias", d);
        const float* f1w = W(p + "fc1.weight", (size_t)ffn * d); const float* f1b = W(p + "fc1.bias", ffn);
        const float* f2w = W(p + "fc2.weight", (size_t)d * ffn); const float* f2b = W(p + "fc2.bias", d);
        if (err) return 1;
        if (!e->qkv_w[l]) {
            // q | k | v as one stacked projection; the q rows (weight and bias) carry head_dim^-0.5 = 2^-3, an exact scaling in float32:
            // (x Wq + bq) * 2^-3 == x (2^-3 Wq) + 2^-3 bq bit for bit
            OMX_HIP_CHECK(hipMalloc((void**)&e->qkv_w[l], (size_t)3 * d * d * sizeof(float)));
            OMX_HIP_CHECK(hipMalloc((void**)&e->qkv_b[l], (size_t)3 * d * sizeof(float)));
            const char* nm[3] = {"q_proj", "k_proj", "v_proj"};
            for (int i = 0; i < 3; ++i) {
                const float* pw = W(p + "self_attn." + nm[i] + ".weight", (size_t)d * d);
                const float* pb = W(p + "self_attn." + nm[i] + ".bias", d);
                if (err) return 1;
                OMX_HIP_CHECK(hipMemcpyAsync(e->qkv_w[l] + (size_t)i * d * d, pw, (size_t)d * d * sizeof(float), hipMemcpyDeviceToDevice, s));
                OMX_HIP_CHECK(hipMemcpyAsync(e->qkv_b[l] + (size_t)i * d, pb, (size_t)d * sizeof(float), hipMemcpyDeviceToDevice, s));
            }
            scale_kernel<<<grid_for((int64_t)d * d), 256, 0, s>>>(e->qkv_w[l], (int64_t)d * d, 0.125f);
            scale_kernel<<<grid_for(d), 256, 0, s>>>(e->qkv_b[l], d, 0.125f);
            OMX_LAUNCH_CHECK();
        }
        if (omx_layer_norm(t1, h, n1w, n1b, N, d, 1e-5f, OMX_FLOAT32, s)) return 1;
        if (gemm(t0, t1, e->qkv_w[l], e->qkv_b[l], nullptr, N, 3 * d, d, s)) return 1;
        if (launch_window_attn_f32(t1, d, t0, t0 + d, t0 + 2 * d, 3 * d, N, c.n_heads, window, s)) return 1;
        if (gemm(h, t1, ow, ob, h, N, d, d, s)) return 1;                              // + residual, in place: each element read then written by its own thread
        if (omx_layer_norm(t1, h, n2w, n2b, N, d, 1e-5f, OMX_FLOAT32, s)) return 1;
        if (gemm(t0, t1, f1w, f1b, nullptr, N, ffn, d, s) || gelu(t0, (int64_t)N * ffn, s)) return 1;
        if (gemm(h, t0, f2w, f2b, h, N, d, ffn, s)) return 1;
    }
    // ---- tail ----
    if (omx_layer_norm(t1, h, lnw, lnb, N, d, 1e-5f, OMX_FLOAT32, s)) return 1;
    if (gemm(t0, t1, p1w, p1b, nullptr, N, d, d, s) || gelu(t0, (int64_t)N * d, s)) return 1;
    return gemm(out_rows, t0, p2w, p2b, nullptr, N, c.output_dim, d, s);
}

int omx_qwen3_asr_encoder_debug_read(omx_qwen3_asr_encoder e, const char* name, float* host, size_t n_elems) {
    OMX_REQUIRE(e && name && host, "omx_qwen3_asr_encoder_debug_read: null argument");
    const std::string s(name);
    const int role = s == "x1" ? B_X1 : s == "x2" ? B_X2 : s == "x3" ? B_X3 : s == "h" ? B_H : -1;
    OMX_REQUIRE(role >= 0, "omx_qwen3_asr_encoder_debug_read: unknown stage %s", name);
    OMX_REQUIRE(e->buf[role] && n_elems <= e->cap[role], "omx_qwen3_asr_encoder_debug_read: %zu elements of %s, the buffer holds %zu", n_elems, name, e->cap[role]);
    OMX_HIP_CHECK(hipDeviceSynchronize());
    OMX_HIP_CHECK(hipMemcpy(host, e->buf[role], n_elems * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

/* the windowed attention alone (test hook and building block): q | k | v DEVICE f32 rows `ld` floats apart, head h at column 64 h;
 * out token-major, rows `ldo` apart; windows of `window` rows from row 0, a shorter last one */
int omx_window_attention_f32(float* out, int64_t ldo, const float* q, const float* k, const float* v, int64_t ld, int n, int heads, int window,
                             omx_stream stream) {
    return launch_window_attn_f32(out, ldo, q, k, v, ld, n, heads, window, (hipStream_t)stream);
}

}  // extern "C"
