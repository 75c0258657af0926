// The two vision towers of Moxin-VLM (moxin-vlm-mlx/src/vision.rs: DINOv2 ViT-L/14 with CLS, registers and LayerScale; SigLIP SO400M/14
// plain) and its projector (projector.rs) in float32: the reference feeds a float32 image into bf16 parameters and casts nothing, so MLX
// promotes every op of the towers and the projector to float32 -- the situation audio_encoder.hip describes for the audio tower.  Weights
// are widened once at load (the caller hands float32), every launch below is float32.
//   image [S, S, 3] in [0, 1] -> im2col of the P x P x 3 patches with (x - mean) / std folded into the gather -> the float32 matrix-core
//   GEMM (K = 3 P P) -> one launch assembles CLS | registers | patches + pos_embed (either form of pos_embed, vision.rs:268-295) ->
//   blocks 0 .. depth - 2 (the feature layer of vision.rs:297-301; the tower's final norm is loaded and never applied, as there) ->
//   the patch rows, written with a caller's row stride so that two towers fill the two column ranges of one buffer.
// Per block, seven launches (nine where a product splits K: its reduce launch):
//   LayerNorm | qkv GEMM (+ bias) | attention | proj GEMM (+ bias, * ls1, + residual) | LayerNorm | fc1 GEMM (+ bias, GELU) |
//   fc2 GEMM (+ bias, * ls2, + residual)
#include <math.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "gemm.hpp"

namespace {

using namespace omx;

// flag[0] |= 1 where the image holds a NaN or an infinity
__global__ void vit_nonfinite_kernel(const float* __restrict__ x, int64_t n, int* __restrict__ flag) {
    bool bad = false;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) bad |= !(fabsf(x[i]) <= 3.4028234e38f);
    if (bad) atomicOr(flag, 1);
}

// the checkpoint's convolution weight [O, I, P, P] as the [O, P, P, I] the reference transposes it to (vision.rs:386-387): rows of the GEMM's B
__global__ void conv_weight_kernel(float* __restrict__ out, const float* __restrict__ w, int O, int I, int P) {
    const int64_t n = (int64_t)O * I * P * P;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % I), kw = (int)((i / I) % P), kh = (int)((i / ((int64_t)I * P)) % P), o = (int)(i / ((int64_t)I * P * P));
        out[i] = w[(((int64_t)o * I + c) * P + kh) * P + kw];
    }
}

// im2col of the stride-P, unpadded P x P convolution over the NHWC image [S, S, 3], normalised on the way: A [G * G, P * P * 3],
// k = (kh * P + kw) * 3 + c.  (x - mean) / std in float32, the two ops of normalize_dino / normalize_siglip (lib.rs:427-440).
struct Norm3 { float mean[3], std[3]; };
__global__ void patch_im2col_kernel(float* __restrict__ A, const float* __restrict__ img, int S, int P, int G, Norm3 nm) {
    const int K = P * P * 3;
    const int64_t n = (int64_t)G * G * K;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int k = (int)(i % K), p = (int)(i / K);
        const int c = k % 3, kw = (k / 3) % P, kh = k / (3 * P), px = p % G, py = p / G;
        const float x = img[((int64_t)(py * P + kh) * S + px * P + kw) * 3 + c];
        A[i] = (x - nm.mean[c]) / nm.std[c];
    }
}

// vision.rs:268-295 in one launch: h [T, dim] = CLS (+ pos[0] when pos_embed has a CLS row) | registers (no position) | patches + pos.
// pos_rows == np: pos row i goes with patch i; pos_rows == np + 1: row 0 with CLS, row 1 + i with patch i.
__global__ void assemble_kernel(float* __restrict__ h, const float* __restrict__ patches, const float* __restrict__ pos, const float* __restrict__ cls,
                                const float* __restrict__ reg, int np, int dim, int n_cls, int n_reg, int pos_rows) {
    const int T = n_cls + n_reg + np;
    const int64_t n = (int64_t)T * dim;
    const int shift = pos_rows == np ? 0 : 1;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int col = (int)(i % dim), r = (int)(i / dim);
        float v;
        if (r < n_cls) v = shift ? cls[col] + pos[col] : cls[col];
        else if (r < n_cls + n_reg) v = reg[(int64_t)(r - n_cls) * dim + col];
        else {
            const int p = r - n_cls - n_reg;
            v = patches[(int64_t)p * dim + col] + pos[(int64_t)(p + shift) * dim + col];
        }
        h[i] = v;
    }
}

// rows [skip, skip + np) of h to the caller's rows (row stride ldo): only a tower that runs no block ends here, the others' last GEMM
// writes the caller's rows itself
__global__ void rows_out_kernel(float* __restrict__ out, int64_t ldo, const float* __restrict__ h, int np, int dim) {
    const int64_t n = (int64_t)np * dim;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[(i / dim) * ldo + i % dim] = h[i];
}

// ---- full (unmasked) float32 attention at head widths 64 and 72 on v_mfma_f32_16x16x4_f32, the explicit form: every score of a row, then
//      max / exp / sum, then the product with V, the division last.  Block = (16 query rows, head), four waves.
//        scores   wave w takes the key tiles w, w + 4, ...: S[16 x 16] = Q . K^T in W / 8 pairs of MFMAs.  The terms of a dot product are
//                 taken in a permuted order -- lane (n, g) of pair j multiplies k = 8 j + 2 g and 8 j + 2 g + 1 -- so that Q and K fragments
//                 are 8-byte loads straight from the stacked projection (72 = 9 x 8: width 72 needs no tail form).  Even and odd terms run
//                 in two accumulator chains (the 16 x 16 x 4 form's dependent latency is above its issue interval) added at the end.
//                 Scores * scale go to LDS rows of SLD floats, SLD = 4 mod 64: the P fragment reads below are conflict-free.
//        softmax  wave w owns rows 4 w .. 4 w + 3: maximum, expf, sum through the wave's shuffle tree; the unnormalised p overwrite the
//                 scores, columns at and past N become 0, the row's sum waits in LDS.
//        P . V    wave w takes a quarter of the key quads, contiguous, against ALL ceil(W / 16) column tiles (width 72: 4.5 tiles, the
//                 fifth half masked) -- V fragments are 64-byte runs of a row read from global memory.  The four partial tiles meet in
//                 LDS (over the dead scores) and are added in wave order 0, 1, 2, 3, then divided by the row's sum: one fixed order, the
//                 same input gives the same bits.
//      Rows past N of the last query tile compute on the last row's q and are not stored; keys past N re-read the last key and their
//      scores are never used; V past N is read as 0.
constexpr int VA_ROWS = 16, VA_MAXN = 1024, VA_CT = 5;
using f32x2 = __attribute__((ext_vector_type(2))) float;
inline int va_sld(int N) { return ((N + 63) / 64) * 64 + 4; }
inline size_t va_lds_bytes(int N) {
    const size_t s = (size_t)VA_ROWS * va_sld(N), o = (size_t)4 * VA_ROWS * VA_CT * 16;
    return (std::max(s, o) + VA_ROWS) * sizeof(float);
}

template <int W>
__global__ __launch_bounds__(256) void vit_attn_kernel(float* __restrict__ out, int64_t ldo, const float* __restrict__ q, const float* __restrict__ k,
                                                       const float* __restrict__ v, int64_t ld, int N, int SLD, float scale) {
    extern __shared__ __attribute__((aligned(16))) float va_lds[];
    constexpr int CT = (W + 15) / 16;
    const int body = VA_ROWS * SLD > 4 * VA_ROWS * VA_CT * 16 ? VA_ROWS * SLD : 4 * VA_ROWS * VA_CT * 16;
    float* S = va_lds;                                 // [16][SLD] scores, then p; later [4 waves][16][CT * 16] partial outputs
    float* rowsum = va_lds + body;                     // [16]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, g = lane >> 4;
    const int q0 = blockIdx.x * VA_ROWS, hc = blockIdx.y * W;
    const int ntiles = (N + 15) / 16;

    // ---- scores ----
    {
        f32x2 a[W / 8];
        const float* qr = q + (int64_t)min(q0 + n, N - 1) * ld + hc + 2 * g;
#pragma unroll
        for (int j = 0; j < W / 8; ++j) a[j] = *reinterpret_cast<const f32x2*>(qr + 8 * j);
        for (int t = wave; t < ntiles; t += 4) {
            const float* kr = k + (int64_t)min(t * 16 + n, N - 1) * ld + hc + 2 * g;
            f32x2 b[W / 8];
#pragma unroll
            for (int j = 0; j < W / 8; ++j) b[j] = *reinterpret_cast<const f32x2*>(kr + 8 * j);
            f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < W / 8; ++j) {
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j][0], b[j][0], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j][1], b[j][1], acc1, 0, 0, 0);
            }
            // D of the 16 x 16 form: column (key) = lane & 15, row (query) = 4 (lane >> 4) + reg
#pragma unroll
            for (int r = 0; r < 4; ++r) S[(4 * g + r) * SLD + t * 16 + n] = (acc0[r] + acc1[r]) * scale;
        }
    }
    __syncthreads();
    // ---- softmax numerators ----
    const int npad4 = ntiles * 16;
    for (int r = 4 * wave; r < 4 * wave + 4; ++r) {
        float* row = S + r * SLD;
        float m = -INFINITY;
        for (int c = lane; c < N; c += 64) m = fmaxf(m, row[c]);
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        float sum = 0.f;
        for (int c = lane; c < npad4; c += 64) {
            const float p = c < N ? expf(row[c] - m) : 0.f;
            row[c] = p;
            sum += p;
        }
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
        if (lane == 0) rowsum[r] = sum;
    }
    __syncthreads();
    // ---- P . V: this wave's key quads ----
    f32x4 o[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) o[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
    {
        const int quads = npad4 / 4, per = (quads + 3) / 4, s0 = wave * per, s1 = min(quads, s0 + per);
        for (int s = s0; s < s1; ++s) {
            const int key = 4 * s + g;
            const float p = S[n * SLD + key];          // A fragment: row lane & 15, k = lane >> 4
            const float* vr = v + (int64_t)min(key, N - 1) * ld + hc;
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                const int col = c * 16 + n;
                const float x = (key < N && col < W) ? vr[min(col, W - 1)] : 0.f;
                o[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(p, x, o[c], 0, 0, 0);
            }
        }
    }
    __syncthreads();                                   // every wave is done with p: the partial tiles go over it
    float* part = S + wave * VA_ROWS * VA_CT * 16;
#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) part[(4 * g + r) * (VA_CT * 16) + c * 16 + n] = o[c][r];
    __syncthreads();
    for (int i = threadIdx.x; i < VA_ROWS * W; i += 256) {
        const int r = i / W, col = i % W;
        if (q0 + r >= N) continue;
        float acc = S[r * (VA_CT * 16) + col];
#pragma unroll
        for (int w = 1; w < 4; ++w) acc += S[(w * VA_ROWS + r) * (VA_CT * 16) + col];
        out[(int64_t)(q0 + r) * ldo + hc + col] = acc / rowsum[r];
    }
}

int launch_vit_attn_f32(float* out, int64_t ldo, const float* q, const float* k, const float* v, int64_t ld, int N, int heads, int width, hipStream_t s) {
    OMX_REQUIRE(out && q && k && v && heads >= 1, "vit attention: bad arguments (heads=%d)", heads);
    OMX_REQUIRE(width == 64 || width == 72, "InvalidConfig: vit attention: head width %d: the kernel is built for 64 and 72", width);
    OMX_REQUIRE(N >= 1 && N <= VA_MAXN, "InvalidConfig: vit attention: %d rows: the kernel takes 1 .. %d (a row's scores lie in LDS)", N, VA_MAXN);
    OMX_REQUIRE(ld >= (int64_t)heads * width && ldo >= (int64_t)heads * width, "vit attention: leading dimensions %lld / %lld below heads * width = %d",
                (long long)ld, (long long)ldo, heads * width);
    // the 8-byte fragment loads
    OMX_REQUIRE(ld % 2 == 0 && ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k)) & 7u) == 0,
                "vit attention: q / k rows must be 8-byte aligned (ld %lld)", (long long)ld);
    static const bool lds_ok = hipFuncSetAttribute((const void*)vit_attn_kernel<64>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)va_lds_bytes(VA_MAXN)) == hipSuccess &&
                               hipFuncSetAttribute((const void*)vit_attn_kernel<72>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)va_lds_bytes(VA_MAXN)) == hipSuccess;
    OMX_REQUIRE(lds_ok, "vit attention: the device refused %zu bytes of LDS per block", va_lds_bytes(VA_MAXN));
    const dim3 grid((N + VA_ROWS - 1) / VA_ROWS, heads);
    const float scale = 1.0f / sqrtf((float)width);
    if (width == 64) vit_attn_kernel<64><<<grid, 256, va_lds_bytes(N), s>>>(out, ldo, q, k, v, ld, N, va_sld(N), scale);
    else vit_attn_kernel<72><<<grid, 256, va_lds_bytes(N), s>>>(out, ldo, q, k, v, ld, N, va_sld(N), scale);
    OMX_LAUNCH_CHECK();
    return 0;
}

inline unsigned grid_for(int64_t n) { return (unsigned)std::min<int64_t>((n + 255) / 256, 8192); }

struct Linear {
    const float* a; const float* w; const float* bias; const float* resid; const float* col_scale; float* out;
    int M, N, K; int64_t ldc, ldr; int gelu;
};
int gemm(const Linear& l, hipStream_t s) {
    GemmF32 g = {};
    g.a = l.a; g.b = l.w; g.bias = l.bias; g.resid = l.resid; g.out = l.out;
    g.M = l.M; g.N = l.N; g.K = l.K; g.lda = l.K; g.ldb = l.K; g.ldc = l.ldc ? l.ldc : l.N; g.ldr = l.ldr ? l.ldr : l.N;
    g.batch = 1; g.alpha = 1.0f;
    g.gelu = l.gelu; g.col_scale = l.col_scale;
    return launch_gemm_f32(g, s);
}

struct Store {
    std::map<std::string, float*> w;              // device float32 tensors by key
    std::map<std::string, std::vector<int64_t>> shape;
    ~Store() { for (auto& kv : w) (void)hipFree(kv.second); }
    int load(const char* who, const char* name, const float* host, const int64_t* shp, int ndim) {
        OMX_REQUIRE(name && host && shp && ndim >= 1 && ndim <= 4, "%s: bad argument", who);
        size_t n = 1;
        for (int i = 0; i < ndim; ++i) { OMX_REQUIRE(shp[i] >= 1, "%s: %s: empty dimension", who, name); n *= (size_t)shp[i]; }
        const std::string key(name);
        auto it = w.find(key);
        if (it != w.end()) { (void)hipDeviceSynchronize(); (void)hipFree(it->second); w.erase(it); }
        float* dev = nullptr;
        OMX_HIP_CHECK(hipMalloc((void**)&dev, n * sizeof(float)));
        if (hipMemcpy(dev, host, n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(dev); return omx::set_error("%s: %s: copy to the device failed", who, name); }
        w[key] = dev;
        shape[key] = std::vector<int64_t>(shp, shp + ndim);
        return 0;
    }
    size_t count(const std::string& key) const {
        auto it = shape.find(key);
        if (it == shape.end()) return 0;
        size_t n = 1;
        for (int64_t d : it->second) n *= (size_t)d;
        return n;
    }
};

}  // namespace

struct omx_vit_encoder_ {
    omx_vit_config cfg;
    std::string prefix;                           // the checkpoint prefix, for the error texts only
    int grid, np, tokens, skip, blocks_run;
    Store st;
    float* conv_w = nullptr;                      // [dim, P, P, 3]
    int* flag = nullptr;
    float* buf[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // scratch, grown per role
    size_t cap[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int launches = 0;                             // of the last forward
};

struct omx_vlm_projector_ {
    Store st;
    float* buf[2] = {nullptr, nullptr};
    size_t cap[2] = {0, 0};
};

namespace {

enum { V_COL = 0, V_PATCH, V_H, V_LN1, V_QKV, V_ATT, V_LN2, V_MLP };

int reserve(float** buf, size_t* cap, size_t elems, hipStream_t s) {
    if (elems <= *cap) return 0;
    OMX_HIP_CHECK(hipStreamSynchronize(s));
    if (*buf) OMX_HIP_CHECK(hipFree(*buf));
    *buf = nullptr; *cap = 0;
    OMX_HIP_CHECK(hipMalloc((void**)buf, elems * sizeof(float)));
    *cap = elems;
    return 0;
}

struct BlockW {
    const float *n1w, *n1b, *qkvw, *qkvb, *pw, *pb, *ls1, *n2w, *n2b, *f1w, *f1b, *f2w, *f2b, *ls2;
};

// a tensor by key: required (WeightNotFound) or optional (null), its element count checked against the config where it is present
const float* find(omx_vit_encoder e, const std::string& key, const std::string& alt, size_t want, bool required, int* err) {
    if (*err) return nullptr;                     // the first missing or misshapen tensor is the one reported
    const std::string* name = &key;
    auto it = e->st.w.find(key);
    if (it == e->st.w.end() && !alt.empty()) { it = e->st.w.find(alt); name = &alt; }
    if (it == e->st.w.end()) {
        if (required) *err = omx::set_error("WeightNotFound: %s%s%s%s", e->prefix.c_str(), key.c_str(), alt.empty() ? "" : " or ", alt.empty() ? "" : (e->prefix + alt).c_str());
        return nullptr;
    }
    if (e->st.count(*name) != want) {
        *err = omx::set_error("ShapeMismatch: %s%s has %zu elements, the config expects %zu", e->prefix.c_str(), name->c_str(), e->st.count(*name), want);
        return nullptr;
    }
    return it->second;
}

}  // namespace

extern "C" {

int omx_vit_encoder_create(omx_vit_encoder* out, const omx_vit_config* cfg) {
    OMX_REQUIRE(out && cfg, "omx_vit_encoder_create: null argument");
    const omx_vit_config& c = *cfg;
    OMX_REQUIRE(c.embed_dim >= 4 && c.depth >= 1 && c.num_heads >= 1 && c.head_dim >= 1 && c.intermediate_dim >= 4 && c.patch_size >= 1 && c.image_size >= 1 &&
                c.num_registers >= 0, "InvalidConfig: vit encoder embed_dim=%d depth=%d heads=%d head_dim=%d mlp=%d patch=%d image=%d registers=%d",
                c.embed_dim, c.depth, c.num_heads, c.head_dim, c.intermediate_dim, c.patch_size, c.image_size, c.num_registers);
    OMX_REQUIRE(c.head_dim == 64 || c.head_dim == 72, "InvalidConfig: vit encoder head width %d: the attention kernel is built for 64 and 72", c.head_dim);
    OMX_REQUIRE(c.embed_dim == c.num_heads * c.head_dim, "InvalidConfig: vit encoder embed_dim %d is not heads * head width = %d * %d", c.embed_dim, c.num_heads, c.head_dim);
    OMX_REQUIRE(c.image_size % c.patch_size == 0, "InvalidConfig: vit encoder image size %d is not a multiple of the patch %d", c.image_size, c.patch_size);
    OMX_REQUIRE(c.num_registers == 0 || c.has_cls_token, "InvalidConfig: vit encoder: %d register rows without a CLS row (the reference inserts them behind it)", c.num_registers);
    for (int i = 0; i < 3; ++i)
        OMX_REQUIRE(c.std[i] > 0.f && c.std[i] <= 3.4028234e38f && fabsf(c.mean[i]) <= 3.4028234e38f, "InvalidConfig: vit encoder channel %d mean %g / std %g", i, c.mean[i], c.std[i]);
    const int G = c.image_size / c.patch_size, np = G * G, T = (c.has_cls_token ? 1 : 0) + c.num_registers + np;
    OMX_REQUIRE(T <= VA_MAXN, "InvalidConfig: vit encoder: %d rows (image %d, patch %d) exceed the attention kernel's %d", T, c.image_size, c.patch_size, VA_MAXN);
    omx_vit_encoder e = new omx_vit_encoder_();
    e->cfg = c;
    e->cfg.key_prefix[sizeof(e->cfg.key_prefix) - 1] = 0;
    e->prefix = e->cfg.key_prefix;
    if (!e->prefix.empty() && e->prefix.back() != '.') e->prefix += '.';
    e->grid = G; e->np = np; e->tokens = T;
    e->skip = T - np;
    e->blocks_run = c.depth - 1;                  // blocks 0 .. depth - 2 (vision.rs:297-301)
    if (hipMalloc((void**)&e->flag, sizeof(int)) != hipSuccess) {
        delete e;
        return omx::set_error("omx_vit_encoder_create: device allocation failed");
    }
    *out = e;
    return 0;
}

int omx_vit_encoder_destroy(omx_vit_encoder e) {
    if (!e) return 0;
    (void)hipDeviceSynchronize();
    for (float* p : e->buf) if (p) (void)hipFree(p);
    if (e->conv_w) (void)hipFree(e->conv_w);
    if (e->flag) (void)hipFree(e->flag);
    delete e;
    return 0;
}

int omx_vit_encoder_load(omx_vit_encoder e, const char* name, const float* host, const int64_t* shape, int ndim) {
    OMX_REQUIRE(e, "omx_vit_encoder_load: null handle");
    if (e->st.load("omx_vit_encoder_load", name, host, shape, ndim)) return 1;
    if (std::string(name) == "patch_embed.proj.weight" && e->conv_w) { (void)hipFree(e->conv_w); e->conv_w = nullptr; }   // re-laid at the next forward
    return 0;
}

int omx_vit_encoder_tokens(omx_vit_encoder e, int* n_tokens, int* n_rows) {
    OMX_REQUIRE(e && n_tokens && n_rows, "omx_vit_encoder_tokens: null argument");
    *n_tokens = e->tokens;
    *n_rows = e->np;
    return 0;
}

int omx_vit_encoder_launches(omx_vit_encoder e, int* n) {
    OMX_REQUIRE(e && n, "omx_vit_encoder_launches: null argument");
    *n = e->launches;
    return 0;
}

int omx_vit_encoder_forward(omx_vit_encoder e, const float* image, float* out_rows, int64_t ldo, omx_stream stream) {
    OMX_REQUIRE(e && image && out_rows, "omx_vit_encoder_forward: null argument");
    hipStream_t s = (hipStream_t)stream;
    const omx_vit_config& c = e->cfg;
    const int d = c.embed_dim, ffn = c.intermediate_dim, P = c.patch_size, S = c.image_size, np = e->np, T = e->tokens, K0 = 3 * P * P;
    OMX_REQUIRE(ldo >= d, "omx_vit_encoder_forward: row stride %lld below the tower's width %d", (long long)ldo, d);

    // ---- every tensor the pass reads, before any launch ----
    int err = 0;
    auto W = [&](const std::string& key, size_t want) { return find(e, key, "", want, true, &err); };
    auto O = [&](const std::string& key, size_t want) { return find(e, key, "", want, false, &err); };
    const float* cw = W("patch_embed.proj.weight", (size_t)d * K0);
    const float* cb = O("patch_embed.proj.bias", d);
    if (err) return 1;
    const size_t pos_n = e->st.count("pos_embed");
    OMX_REQUIRE(pos_n, "WeightNotFound: %spos_embed", e->prefix.c_str());
    const int pos_rows = (int)(pos_n / d);
    OMX_REQUIRE(pos_n % d == 0 && (pos_rows == np || (pos_rows == np + 1 && c.has_cls_token)),
                "ShapeMismatch: %spos_embed has %zu elements: neither %d rows (added before the CLS row) nor %d rows with a CLS row (added after) of %d",
                e->prefix.c_str(), pos_n, np, np + 1, d);
    const float* pos = W("pos_embed", pos_n);
    const float* cls = c.has_cls_token ? W("cls_token", d) : nullptr;
    const float* reg = c.num_registers ? find(e, "reg_token", "register_tokens", (size_t)c.num_registers * d, true, &err) : nullptr;
    (void)O("norm.weight", d); (void)O("norm.bias", d);          // loaded by the reference, applied by nobody (vision.rs:297-309)
    std::vector<BlockW> bw(e->blocks_run);
    for (int l = 0; l < e->blocks_run; ++l) {
        const std::string p = "blocks." + std::to_string(l) + ".";
        BlockW& b = bw[l];
        b.n1w = W(p + "norm1.weight", d); b.n1b = O(p + "norm1.bias", d);
        b.qkvw = W(p + "attn.qkv.weight", (size_t)3 * d * d); b.qkvb = O(p + "attn.qkv.bias", (size_t)3 * d);
        b.pw = W(p + "attn.proj.weight", (size_t)d * d); b.pb = O(p + "attn.proj.bias", d);
        b.n2w = W(p + "norm2.weight", d); b.n2b = O(p + "norm2.bias", d);
        b.f1w = W(p + "mlp.fc1.weight", (size_t)ffn * d); b.f1b = O(p + "mlp.fc1.bias", ffn);
        b.f2w = W(p + "mlp.fc2.weight", (size_t)d * ffn); b.f2b = O(p + "mlp.fc2.bias", d);
        b.ls1 = c.has_layer_scale ? find(e, p + "ls1.gamma", p + "ls1.scale_factor", d, true, &err) : nullptr;
        b.ls2 = c.has_layer_scale ? find(e, p + "ls2.gamma", p + "ls2.scale_factor", d, true, &err) : nullptr;
    }
    if (err) return 1;

    OMX_HIP_CHECK(hipMemsetAsync(e->flag, 0, sizeof(int), s));
    vit_nonfinite_kernel<<<grid_for((int64_t)S * S * 3), 256, 0, s>>>(image, (int64_t)S * S * 3, e->flag);
    OMX_LAUNCH_CHECK();
    int bad = 0;
    OMX_HIP_CHECK(hipMemcpyAsync(&bad, e->flag, sizeof(int), hipMemcpyDeviceToHost, s));
    OMX_HIP_CHECK(hipStreamSynchronize(s));
    OMX_REQUIRE(!bad, "omx_vit_encoder_forward: the image holds a NaN or an infinity");

    const bool blocks = e->blocks_run > 0;
    if (reserve(&e->buf[V_COL], &e->cap[V_COL], (size_t)np * K0, s) || reserve(&e->buf[V_PATCH], &e->cap[V_PATCH], (size_t)np * d, s) ||
        reserve(&e->buf[V_H], &e->cap[V_H], (size_t)T * d, s))
        return 1;
    if (blocks && (reserve(&e->buf[V_LN1], &e->cap[V_LN1], (size_t)T * d, s) || reserve(&e->buf[V_QKV], &e->cap[V_QKV], (size_t)T * 3 * d, s) ||
                   reserve(&e->buf[V_ATT], &e->cap[V_ATT], (size_t)T * d, s) || reserve(&e->buf[V_LN2], &e->cap[V_LN2], (size_t)T * d, s) ||
                   reserve(&e->buf[V_MLP], &e->cap[V_MLP], (size_t)T * ffn, s)))
        return 1;
    float *col = e->buf[V_COL], *patches = e->buf[V_PATCH], *h = e->buf[V_H], *ln1 = e->buf[V_LN1], *qkv = e->buf[V_QKV], *att = e->buf[V_ATT],
          *ln2 = e->buf[V_LN2], *mlp = e->buf[V_MLP];
    if (!e->conv_w) {
        OMX_HIP_CHECK(hipMalloc((void**)&e->conv_w, (size_t)d * K0 * sizeof(float)));
        conv_weight_kernel<<<grid_for((int64_t)d * K0), 256, 0, s>>>(e->conv_w, cw, d, 3, P);
        OMX_LAUNCH_CHECK();
    }
    int launches = 1;                             // the non-finite check
    // ---- patch embedding and assembly ----
    Norm3 nm;
    for (int i = 0; i < 3; ++i) { nm.mean[i] = c.mean[i]; nm.std[i] = c.std[i]; }
    patch_im2col_kernel<<<grid_for((int64_t)np * K0), 256, 0, s>>>(col, image, S, P, e->grid, nm);
    OMX_LAUNCH_CHECK();
    if (gemm({col, e->conv_w, cb, nullptr, nullptr, patches, np, d, K0, 0, 0, 0}, s)) return 1;
    assemble_kernel<<<grid_for((int64_t)T * d), 256, 0, s>>>(h, patches, pos, cls, reg, np, d, c.has_cls_token ? 1 : 0, c.num_registers, pos_rows);
    OMX_LAUNCH_CHECK();
    launches += 3;
    // ---- blocks 0 .. depth - 2 (vision.rs:216-230) ----
    for (int l = 0; l < e->blocks_run; ++l) {
        const BlockW& b = bw[l];
        const bool last = l + 1 == e->blocks_run;
        if (omx_layer_norm(ln1, h, b.n1w, b.n1b, T, d, 1e-6f, OMX_FLOAT32, s)) return 1;
        if (gemm({ln1, b.qkvw, b.qkvb, nullptr, nullptr, qkv, T, 3 * d, d, 0, 0, 0}, s)) return 1;
        if (launch_vit_attn_f32(att, d, qkv, qkv + d, qkv + 2 * d, 3 * d, T, c.num_heads, c.head_dim, s)) return 1;
        // h += ls1 * (att . Wp^T + bp), in place: each element is read, then written, by its own thread
        if (gemm({att, b.pw, b.pb, h, b.ls1, h, T, d, d, 0, 0, 0}, s)) return 1;
        if (omx_layer_norm(ln2, h, b.n2w, b.n2b, T, d, 1e-6f, OMX_FLOAT32, s)) return 1;
        if (gemm({ln2, b.f1w, b.f1b, nullptr, nullptr, mlp, T, ffn, d, 0, 0, 1}, s)) return 1;
        // the last block's fc2 computes the patch rows only and writes them where the caller wants them: CLS and register rows are dropped
        // by never being made, and two towers fill one [rows, d0 + d1] buffer without a concatenation
        if (!last) { if (gemm({mlp, b.f2w, b.f2b, h, b.ls2, h, T, d, ffn, 0, 0, 0}, s)) return 1; }
        else if (gemm({mlp + (size_t)e->skip * ffn, b.f2w, b.f2b, h + (size_t)e->skip * d, b.ls2, out_rows, np, d, ffn, ldo, d, 0}, s)) return 1;
        launches += 7;
    }
    if (!blocks) {
        rows_out_kernel<<<grid_for((int64_t)np * d), 256, 0, s>>>(out_rows, ldo, h + (size_t)e->skip * d, np, d);
        OMX_LAUNCH_CHECK();
        launches += 1;
    }
    e->launches = launches;
    return 0;
}

int omx_vit_encoder_debug_read(omx_vit_encoder e, const char* name, float* host, size_t n_elems) {
    OMX_REQUIRE(e && name && host, "omx_vit_encoder_debug_read: null argument");
    const std::string s(name);
    const int role = s == "col" ? V_COL : s == "patches" ? V_PATCH : s == "h" ? V_H : s == "ln1" ? V_LN1 : s == "qkv" ? V_QKV : s == "attn" ? V_ATT :
                     s == "ln2" ? V_LN2 : s == "mlp" ? V_MLP : -1;
    OMX_REQUIRE(role >= 0, "omx_vit_encoder_debug_read: unknown stage %s", name);
    OMX_REQUIRE(e->buf[role] && n_elems <= e->cap[role], "omx_vit_encoder_debug_read: %zu elements of %s, the buffer holds %zu", n_elems, name, e->cap[role]);
    OMX_HIP_CHECK(hipDeviceSynchronize());
    OMX_HIP_CHECK(hipMemcpy(host, e->buf[role], n_elems * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

int omx_vit_attention_f32(float* out, int64_t ldo, const float* q, const float* k, const float* v, int64_t ld, int n, int heads, int width,
                          omx_stream stream) {
    return launch_vit_attn_f32(out, ldo, q, k, v, ld, n, heads, width, (hipStream_t)stream);
}

int omx_gemm_f32_epilogue(float* out, const float* a, const float* w, const float* bias, const float* resid, const float* col_scale, int M, int N, int K,
                          int gelu, omx_stream stream) {
    OMX_REQUIRE(out && a && w, "omx_gemm_f32_epilogue: null tensor");
    return gemm({a, w, bias, resid, col_scale, out, M, N, K, 0, 0, gelu ? 1 : 0}, (hipStream_t)stream);
}

int omx_vlm_projector_create(omx_vlm_projector* out) {
    OMX_REQUIRE(out, "omx_vlm_projector_create: null argument");
    *out = new omx_vlm_projector_();
    return 0;
}

int omx_vlm_projector_destroy(omx_vlm_projector p) {
    if (!p) return 0;
    (void)hipDeviceSynchronize();
    for (float* b : p->buf) if (b) (void)hipFree(b);
    delete p;
    return 0;
}

int omx_vlm_projector_load(omx_vlm_projector p, const char* name, const float* host, const int64_t* shape, int ndim) {
    OMX_REQUIRE(p, "omx_vlm_projector_load: null handle");
    return p->st.load("omx_vlm_projector_load", name, host, shape, ndim);
}

/* the widths, read from the weights (projector.rs has no config): in = fc1's columns, out = fc3's rows */
int omx_vlm_projector_dims(omx_vlm_projector p, int* in_dim, int* out_dim) {
    OMX_REQUIRE(p && in_dim && out_dim, "omx_vlm_projector_dims: null argument");
    const char* need[3] = {"fc1.weight", "fc2.weight", "fc3.weight"};
    for (const char* k : need) {
        auto it = p->st.shape.find(k);
        OMX_REQUIRE(it != p->st.shape.end(), "WeightNotFound: projector.%s", k);
        OMX_REQUIRE(it->second.size() == 2, "ShapeMismatch: projector.%s is not a matrix", k);
    }
    const auto &s1 = p->st.shape["fc1.weight"], &s2 = p->st.shape["fc2.weight"], &s3 = p->st.shape["fc3.weight"];
    OMX_REQUIRE(s2[1] == s1[0] && s3[1] == s2[0], "ShapeMismatch: projector widths %lld x %lld, %lld x %lld, %lld x %lld do not chain",
                (long long)s1[0], (long long)s1[1], (long long)s2[0], (long long)s2[1], (long long)s3[0], (long long)s3[1]);
    for (int i = 0; i < 3; ++i) {
        const std::string b = std::string("fc") + char('1' + i) + ".bias";
        const auto& sw = p->st.shape[std::string("fc") + char('1' + i) + ".weight"];
        OMX_REQUIRE(!p->st.count(b) || p->st.count(b) == (size_t)sw[0], "ShapeMismatch: projector.%s has %zu elements, its weight %lld rows", b.c_str(), p->st.count(b), (long long)sw[0]);
    }
    *in_dim = (int)s1[1];
    *out_dim = (int)s3[0];
    return 0;
}

/* fc1 -> gelu -> fc2 -> gelu -> fc3 (projector.rs:34-40), the GELUs in the GEMMs' epilogues: three launches (+ a reduce where K splits).
 * x DEVICE f32 [rows, in] contiguous -> out DEVICE f32 [rows, out] contiguous. */
int omx_vlm_projector_forward(omx_vlm_projector p, const float* x, int rows, float* out, omx_stream stream) {
    OMX_REQUIRE(p && x && out && rows >= 1, "omx_vlm_projector_forward: bad argument");
    int in_dim = 0, out_dim = 0;
    if (omx_vlm_projector_dims(p, &in_dim, &out_dim)) return 1;
    hipStream_t s = (hipStream_t)stream;
    const int h1 = (int)p->st.shape["fc1.weight"][0], h2 = (int)p->st.shape["fc2.weight"][0];
    auto bias = [&](const char* k) -> const float* { auto it = p->st.w.find(k); return it == p->st.w.end() ? nullptr : it->second; };
    if (reserve(&p->buf[0], &p->cap[0], (size_t)rows * h1, s) || reserve(&p->buf[1], &p->cap[1], (size_t)rows * h2, s)) return 1;
    if (gemm({x, p->st.w["fc1.weight"], bias("fc1.bias"), nullptr, nullptr, p->buf[0], rows, h1, in_dim, 0, 0, 1}, s)) return 1;
    if (gemm({p->buf[0], p->st.w["fc2.weight"], bias("fc2.bias"), nullptr, nullptr, p->buf[1], rows, h2, h1, 0, 0, 1}, s)) return 1;
    return gemm({p->buf[1], p->st.w["fc3.weight"], bias("fc3.bias"), nullptr, nullptr, out, rows, out_dim, h2, 0, 0, 0}, s);
}

}  // extern "C"
