// The SAM ViT-B/16 tower of DeepSeek-OCR-2 (deepseek-ocr2-mlx/src/vision.rs, `ImageEncoderViT::forward` :385-431) in float32 over B stacked
// images: the reference feeds a float32 image into bf16 parameters and casts nothing, so MLX promotes every op to float32 -- the situation
// audio_encoder.hip and vit_encoder.hip describe.  Weights are widened once at load (the caller hands float32).
//   images [B, S, S, 3] in [-1, 1] -> im2col of the P x P x 3 patches -> the float32 matrix-core GEMM (+ bias) -> + pos_embed (gathered
//   nearest-neighbour where its grid differs, :435-454) -> the blocks -> neck (1x1 conv as a GEMM, LayerNorm2d = the row LayerNorm in NHWC,
//   3x3 conv as im2col + GEMM, LayerNorm2d) -> two 3x3 stride-2 convolutions -> [B * (G / 4)^2, 896] rows.
// Per block, seven launches (a product that splits K adds its reduce launch): GEMMs and norms over all B * G * G rows, attention per image:
//   LayerNorm | qkv GEMM (+ bias) | attention | proj GEMM (+ bias, + residual) | LayerNorm | lin1 GEMM (+ bias, tanh GELU) |
//   lin2 GEMM (+ bias, + residual)
// The attention is attn_stream_f32.hpp: global blocks stream all G * G keys with an online softmax; window blocks read the image-order
// rows IN PLACE, a padded position of the zero-padded grid (window_partition, :271-299, pads AFTER norm1) reading the qkv Linear's bias
// as its q | k | v -- no partitioned copy, and the qkv GEMM runs over G * G rows, not over the padded grid's.  The relative-position
// bias is built from two [64 rows, g] tables per block in LDS; nothing of N x N is written to device memory.
#include <math.h>

#include "attn_stream_f32.hpp"
#include "tower_f32.hpp"

namespace {

using namespace omx;
using tower::grid_for;
using tower::Linear;

// a checkpoint's convolution weight [O, I, KH, KW] as the [O, KH, KW, I] the reference transposes it to (vision.rs:472-475): rows of the GEMM's B
__global__ void sam_conv_weight_kernel(float* __restrict__ out, const float* __restrict__ w, int O, int I, int KH, int KW) {
    const int64_t n = (int64_t)O * I * KH * KW;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % I), kw = (int)((i / I) % KW), kh = (int)((i / ((int64_t)I * KW)) % KH), o = (int)(i / ((int64_t)I * KW * KH));
        out[i] = w[(((int64_t)o * I + c) * KH + kh) * KW + kw];
    }
}

// im2col of the stride-P, unpadded P x P convolution over NHWC images [B, S, S, 3]: A [B * G * G, P * P * 3], k = (kh * P + kw) * 3 + c
__global__ void sam_patch_im2col_kernel(float* __restrict__ A, const float* __restrict__ img, int B, int S, int P, int G) {
    const int K = P * P * 3;
    const int64_t n = (int64_t)B * G * G * K;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int k = (int)(i % K);
        const int64_t p = i / K;
        const int c = k % 3, kw = (k / 3) % P, kh = k / (3 * P), px = (int)(p % G), py = (int)((p / G) % G), b = (int)(p / ((int64_t)G * G));
        A[i] = img[(((int64_t)b * S + py * P + kh) * S + px * P + kw) * 3 + c];
    }
}

// h [B, G, G, d] = patches + pos_embed [Pg, Pg, d] at (min(int(y * scale), Pg - 1), min(int(x * scale), Pg - 1)), scale = float32(Pg) /
// float32(G) (nearest_interpolate_2d, vision.rs:435-454); scale 0: the grids agree, the position is the patch's own
__global__ void sam_pos_add_kernel(float* __restrict__ h, const float* __restrict__ patches, const float* __restrict__ pos, int B, int G, int Pg, int d, float scale) {
    const int64_t n = (int64_t)B * G * G * d;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int col = (int)(i % d);
        const int64_t p = i / d;
        const int x = (int)(p % G), y = (int)((p / G) % G);
        const int iy = scale != 0.f ? min((int)((float)y * scale), Pg - 1) : y, ix = scale != 0.f ? min((int)((float)x * scale), Pg - 1) : x;
        h[i] = patches[i] + pos[((int64_t)iy * Pg + ix) * d + col];
    }
}

// im2col of a 3x3 pad-1 convolution of the given stride over NHWC x [B, H, W, ch], output rows [row0, row0 + rows) of the B * OH * OW:
// A [rows, 9 * ch], k = (kh * 3 + kw) * ch + ic.  ch % 4 == 0: one float4 per thread and step.
__global__ void sam_im2col3_kernel(float* __restrict__ A, const float* __restrict__ x, int H, int W, int ch, int OH, int OW, int stride, int64_t row0,
                                   int64_t rows) {
    const int q = ch / 4;
    const int64_t n = rows * 9 * q;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int iq = (int)(i % q), tap = (int)((i / q) % 9);
        const int64_t lrow = i / ((int64_t)q * 9), row = row0 + lrow;
        const int ow = (int)(row % OW), oh = (int)((row / OW) % OH);
        const int64_t b = row / ((int64_t)OW * OH);
        const int ih = stride * oh - 1 + tap / 3, iw = stride * ow - 1 + tap % 3;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (ih >= 0 && ih < H && iw >= 0 && iw < W) v = *reinterpret_cast<const f32x4*>(x + ((b * H + ih) * W + iw) * ch + iq * 4);
        *reinterpret_cast<f32x4*>(A + lrow * 9 * ch + (int64_t)tap * ch + iq * 4) = v;
    }
}

// vision.rs:94-217 / :271-326 over `images` stacked images of a gh x gw grid; window 0: global
int sam_attention(float* out, int64_t ldo, const float* qkv, int64_t ld, int images, int gh, int gw, int heads, int window, const float* th, int Lh,
                  const float* tw, int Lw, const float* pad, hipStream_t s) {
    OMX_REQUIRE(out && qkv && th && tw, "sam attention: null tensor");
    OMX_REQUIRE(images >= 1 && gh >= 1 && gw >= 1 && heads >= 1 && window >= 0 && Lh >= 1 && Lw >= 1, "InvalidConfig: sam attention: images=%d grid=%d x %d heads=%d window=%d tables of %d / %d rows",
                images, gh, gw, heads, window, Lh, Lw);
    OMX_REQUIRE((int64_t)gh * gw <= (1 << 24), "InvalidConfig: sam attention: a %d x %d grid", gh, gw);
    OMX_REQUIRE(ld >= (int64_t)3 * heads * 64 && ldo >= (int64_t)heads * 64, "sam attention: leading dimensions %lld / %lld below 3 * heads * 64 = %d / heads * 64 = %d",
                (long long)ld, (long long)ldo, 3 * heads * 64, heads * 64);
    StreamAttn a = {};
    a.qkv = qkv; a.pad = pad; a.out = out; a.ld = ld; a.ldo = ldo;
    a.qoff = 0; a.koff = heads * 64; a.voff = 2 * heads * 64;
    a.heads = heads; a.group = 1; a.n = gh * gw; a.gh = gh; a.gw = gw; a.win = window;
    if (window > 0) {
        OMX_REQUIRE(pad || (gh % window == 0 && gw % window == 0),
                    "sam attention: a %d x %d grid is no multiple of the window %d: pad_qkv, the padded token's q | k | v row, is required", gh, gw, window);
        a.nwy = (gh + window - 1) / window; a.nwx = (gw + window - 1) / window;
        a.dom = window * window; a.ph = window; a.pw = window;
    } else {
        a.pad = nullptr;
        a.nwx = a.nwy = 1; a.dom = a.n; a.ph = gh; a.pw = gw;
    }
    a.th = th; a.tw = tw; a.Lh = Lh; a.Lw = Lw;
    // get_rel_pos_1d (vision.rs:186-196): a table of another length than 2 g - 1 is resampled nearest-neighbour, scale in float32
    a.sh = Lh != 2 * a.ph - 1 ? (float)Lh / (float)(2 * a.ph - 1) : 0.f;
    a.sw = Lw != 2 * a.pw - 1 ? (float)Lw / (float)(2 * a.pw - 1) : 0.f;
    a.scale = 0.125f;
    return launch_stream_attn(window > 0 ? SA_WINDOW : SA_GLOBAL, a, images, s);
}

enum { S_COL = 0, S_PATCH, S_H, S_LN, S_QKV, S_ATT, S_MLP, S_N0, S_N1, S_D2, S_OUT, S_KEEP, S_ROLES };

}  // namespace

struct omx_sam_encoder_ {
    omx_sam_config cfg;
    tower::Store st;
    std::map<std::string, float*> relaid;         // convolution weights as [O, KH, KW, I], made at the first forward that needs them
    tower::Scratch<S_ROLES> sc;
    int launches = 0;                             // of the last forward
    size_t rows = 0, out_rows = 0;                // of the last forward: B * G * G and B * (G / 4)^2
    ~omx_sam_encoder_() { for (auto& kv : relaid) (void)hipFree(kv.second); }
};

namespace {

bool is_global(const omx_sam_config& c, int l) {
    for (int i = 0; i < c.n_global; ++i) if (c.global_attn_indexes[i] == l) return true;
    return false;
}

// rows of a 3x3 pad-1 convolution's output axis
inline int conv_out(int n, int stride) { return (n - 1) / stride + 1; }

const float* relaid_conv(omx_sam_encoder e, const std::string& key, const float* w, int O, int I, int KH, int KW, hipStream_t s, int* err) {
    if (*err) return nullptr;
    auto it = e->relaid.find(key);
    if (it != e->relaid.end()) return it->second;
    float* dev = nullptr;
    if (hipMalloc((void**)&dev, (size_t)O * I * KH * KW * sizeof(float)) != hipSuccess) { *err = omx::set_error("omx_sam_encoder_forward: device allocation failed"); return nullptr; }
    sam_conv_weight_kernel<<<grid_for((int64_t)O * I * KH * KW), 256, 0, s>>>(dev, w, O, I, KH, KW);
    if (hipGetLastError() != hipSuccess) { (void)hipFree(dev); *err = omx::set_error("omx_sam_encoder_forward: launch failed"); return nullptr; }
    e->relaid[key] = dev;
    return dev;
}

struct SamBlockW {
    const float *n1w, *n1b, *qkvw, *qkvb, *rh, *rw, *pw, *pb, *n2w, *n2b, *l1w, *l1b, *l2w, *l2b;
    int Lh, Lw;
};

}  // namespace

extern "C" {

int omx_sam_encoder_create(omx_sam_encoder* out, const omx_sam_config* cfg) {
    OMX_REQUIRE(out && cfg, "omx_sam_encoder_create: null argument");
    const omx_sam_config& c = *cfg;
    OMX_REQUIRE(c.embed_dim >= 4 && c.depth >= 1 && c.num_heads >= 1 && c.mlp_dim >= 4 && c.window >= 1 && c.patch_size >= 1 && c.n_global >= 0 && c.n_global <= 16,
                "InvalidConfig: sam encoder embed_dim=%d depth=%d heads=%d mlp=%d window=%d patch=%d global blocks=%d (at most 16)", c.embed_dim, c.depth,
                c.num_heads, c.mlp_dim, c.window, c.patch_size, c.n_global);
    OMX_REQUIRE(c.embed_dim == c.num_heads * 64, "InvalidConfig: sam encoder head width %d (embed_dim %d / %d heads): the attention kernel is built for 64",
                c.embed_dim / c.num_heads, c.embed_dim, c.num_heads);
    OMX_REQUIRE(c.mlp_dim % 4 == 0, "InvalidConfig: sam encoder mlp_dim %d is no multiple of 4", c.mlp_dim);
    for (int i = 0; i < c.n_global; ++i)
        OMX_REQUIRE(c.global_attn_indexes[i] >= 0 && c.global_attn_indexes[i] < c.depth, "InvalidConfig: sam encoder global block %d of %d", c.global_attn_indexes[i], c.depth);
    omx_sam_encoder e = new omx_sam_encoder_();
    e->cfg = c;
    e->cfg.key_prefix[sizeof(e->cfg.key_prefix) - 1] = 0;
    e->st.prefix = e->cfg.key_prefix;
    if (!e->st.prefix.empty() && e->st.prefix.back() != '.') e->st.prefix += '.';
    *out = e;
    return 0;
}

int omx_sam_encoder_destroy(omx_sam_encoder e) {
    if (!e) return 0;
    (void)hipDeviceSynchronize();
    delete e;
    return 0;
}

int omx_sam_encoder_load(omx_sam_encoder e, const char* name, const float* host, const int64_t* shape, int ndim) {
    OMX_REQUIRE(e, "omx_sam_encoder_load: null handle");
    if (e->st.load("omx_sam_encoder_load", name, host, shape, ndim)) return 1;
    auto it = e->relaid.find(name);                // re-laid at the next forward
    if (it != e->relaid.end()) { (void)hipFree(it->second); e->relaid.erase(it); }
    return 0;
}

int omx_sam_encoder_tokens(omx_sam_encoder e, int image_size, int* grid, int* n_rows, int* out_dim) {
    OMX_REQUIRE(e && grid && n_rows && out_dim, "omx_sam_encoder_tokens: null argument");
    OMX_REQUIRE(image_size >= e->cfg.patch_size && image_size % e->cfg.patch_size == 0, "InvalidConfig: sam encoder image size %d is not a multiple of the patch %d",
                image_size, e->cfg.patch_size);
    OMX_REQUIRE(e->st.dim("net_3.weight", 0) > 0, "WeightNotFound: %snet_3.weight", e->st.prefix.c_str());
    const int G = image_size / e->cfg.patch_size, g4 = conv_out(conv_out(G, 2), 2);
    *grid = G;
    *n_rows = g4 * g4;
    *out_dim = (int)e->st.dim("net_3.weight", 0);
    return 0;
}

int omx_sam_encoder_launches(omx_sam_encoder e, int* n) {
    OMX_REQUIRE(e && n, "omx_sam_encoder_launches: null argument");
    *n = e->launches;
    return 0;
}

int omx_sam_encoder_scratch_bytes(omx_sam_encoder e, size_t* bytes) {
    OMX_REQUIRE(e && bytes, "omx_sam_encoder_scratch_bytes: null argument");
    *bytes = e->sc.bytes();
    return 0;
}

int omx_sam_encoder_forward(omx_sam_encoder e, const float* images, int n_images, int image_size, float* out_rows, omx_stream stream) {
    OMX_REQUIRE(e && images && out_rows, "omx_sam_encoder_forward: null argument");
    hipStream_t s = (hipStream_t)stream;
    const omx_sam_config& c = e->cfg;
    const int d = c.embed_dim, ffn = c.mlp_dim, P = c.patch_size, S = image_size, B = n_images, K0 = 3 * P * P;
    OMX_REQUIRE(B >= 1 && B <= 64, "InvalidConfig: omx_sam_encoder_forward: %d images (1 .. 64)", B);
    OMX_REQUIRE(S >= P && S % P == 0, "InvalidConfig: sam encoder image size %d is not a multiple of the patch %d", S, P);
    const int G = S / P, N = G * G;
    const int64_t R = (int64_t)B * N;
    OMX_REQUIRE(R * std::max(3 * d, ffn) < (1ll << 31), "InvalidConfig: omx_sam_encoder_forward: %d images of %d rows exceed one pass", B, N);

    // ---- every tensor the pass reads, before any launch ----
    tower::Store& st = e->st;
    int err = 0;
    auto W = [&](const std::string& key, size_t want) { return st.find(key, want, true, &err); };
    auto O = [&](const std::string& key, size_t want) { return st.find(key, want, false, &err); };
    const float* cw = W("patch_embed.proj.weight", (size_t)d * K0);
    const float* cb = O("patch_embed.proj.bias", d);
    if (err) return 1;
    const size_t pos_n = st.count("pos_embed");
    OMX_REQUIRE(pos_n, "WeightNotFound: %spos_embed", st.prefix.c_str());
    const int Pg = (int)lround(sqrt((double)(pos_n / d)));
    OMX_REQUIRE(pos_n == (size_t)Pg * Pg * d, "ShapeMismatch: %spos_embed has %zu elements: no square grid of %d", st.prefix.c_str(), pos_n, d);
    const float* pos = W("pos_embed", pos_n);
    std::vector<SamBlockW> bw(c.depth);
    bool needs_pad = G % c.window != 0;
    for (int l = 0; l < c.depth; ++l) {
        const std::string p = "blocks." + std::to_string(l) + ".";
        SamBlockW& b = bw[l];
        b.n1w = W(p + "norm1.weight", d); b.n1b = O(p + "norm1.bias", d);
        b.qkvw = W(p + "attn.qkv.weight", (size_t)3 * d * d);
        b.qkvb = (needs_pad && !is_global(c, l)) ? W(p + "attn.qkv.bias", (size_t)3 * d) : O(p + "attn.qkv.bias", (size_t)3 * d);
        b.Lh = (int)st.dim(p + "attn.rel_pos_h", 0); b.Lw = (int)st.dim(p + "attn.rel_pos_w", 0);
        b.rh = W(p + "attn.rel_pos_h", (size_t)b.Lh * 64); b.rw = W(p + "attn.rel_pos_w", (size_t)b.Lw * 64);
        b.pw = W(p + "attn.proj.weight", (size_t)d * d); b.pb = O(p + "attn.proj.bias", d);
        b.n2w = W(p + "norm2.weight", d); b.n2b = O(p + "norm2.bias", d);
        b.l1w = W(p + "mlp.lin1.weight", (size_t)ffn * d); b.l1b = O(p + "mlp.lin1.bias", ffn);
        b.l2w = W(p + "mlp.lin2.weight", (size_t)d * ffn); b.l2b = O(p + "mlp.lin2.bias", d);
    }
    if (err) return 1;
    const int c1 = (int)st.dim("neck.0.weight", 0), c2 = (int)st.dim("net_2.weight", 0), c3 = (int)st.dim("net_3.weight", 0);
    OMX_REQUIRE(c1 > 0, "WeightNotFound: %sneck.0.weight", st.prefix.c_str());
    OMX_REQUIRE(c2 > 0, "WeightNotFound: %snet_2.weight", st.prefix.c_str());
    OMX_REQUIRE(c3 > 0, "WeightNotFound: %snet_3.weight", st.prefix.c_str());
    OMX_REQUIRE(c1 % 4 == 0 && c2 % 4 == 0, "InvalidConfig: sam encoder neck widths %d / %d are no multiples of 4", c1, c2);
    const float* k0w = W("neck.0.weight", (size_t)c1 * d);
    const float* k1w = W("neck.1.weight", c1); const float* k1b = W("neck.1.bias", c1);
    const float* k2w = W("neck.2.weight", (size_t)c1 * c1 * 9);
    const float* k3w = W("neck.3.weight", c1); const float* k3b = W("neck.3.bias", c1);
    const float* n2w = W("net_2.weight", (size_t)c2 * c1 * 9);
    const float* n3w = W("net_3.weight", (size_t)c3 * c2 * 9);
    if (err) return 1;

    const int G2 = conv_out(G, 2), G4 = conv_out(G2, 2);
    const int64_t R2 = (int64_t)B * G2 * G2, R4 = (int64_t)B * G4 * G4;
    // the im2col scratch of the 3x3 convolutions is bounded: <= 64 MB whatever the batch, the rows go through in groups (audio_encoder.hip)
    const size_t col_budget = (size_t)16 << 20;                                        // floats
    auto group_rows = [&](int64_t rows, int ch) { return std::min<int64_t>(rows, std::max<int64_t>(64, (int64_t)(col_budget / ((size_t)9 * ch)) / 64 * 64)); };
    const int64_t gA = group_rows(R, c1), gB = group_rows(R2, c1), gC = group_rows(R4, c2);
    const size_t col_elems = std::max({(size_t)R * K0, (size_t)gA * 9 * c1, (size_t)gB * 9 * c1, (size_t)gC * 9 * c2});
    auto& sc = e->sc;
    if (sc.reserve(S_COL, col_elems, s) || sc.reserve(S_PATCH, (size_t)R * d, s) || sc.reserve(S_H, (size_t)R * d, s) || sc.reserve(S_LN, (size_t)R * d, s) ||
        sc.reserve(S_QKV, (size_t)R * 3 * d, s) || sc.reserve(S_ATT, (size_t)R * d, s) || sc.reserve(S_MLP, (size_t)R * ffn, s) ||
        sc.reserve(S_N0, (size_t)R * c1, s) || sc.reserve(S_N1, (size_t)R * c1, s) || sc.reserve(S_D2, (size_t)R2 * c2, s) || sc.reserve(S_OUT, (size_t)R4 * c3, s))
        return 1;
    if (c.keep_stages && sc.reserve(S_KEEP, (size_t)(c.depth + 1) * R * d, s)) return 1;
    float *col = sc.buf[S_COL], *patches = sc.buf[S_PATCH], *h = sc.buf[S_H], *ln = sc.buf[S_LN], *qkv = sc.buf[S_QKV], *att = sc.buf[S_ATT], *mlp = sc.buf[S_MLP],
          *n0 = sc.buf[S_N0], *n1 = sc.buf[S_N1], *d2 = sc.buf[S_D2], *out = sc.buf[S_OUT], *keep = sc.buf[S_KEEP];
    const float* cwr = relaid_conv(e, "patch_embed.proj.weight", cw, d, 3, P, P, s, &err);
    const float* k2r = relaid_conv(e, "neck.2.weight", k2w, c1, c1, 3, 3, s, &err);
    const float* n2r = relaid_conv(e, "net_2.weight", n2w, c2, c1, 3, 3, s, &err);
    const float* n3r = relaid_conv(e, "net_3.weight", n3w, c3, c2, 3, 3, s, &err);
    if (err) return 1;
    e->rows = (size_t)R; e->out_rows = (size_t)R4;

    int launches = 0;
    // ---- patch embedding and positions ----
    sam_patch_im2col_kernel<<<grid_for(R * K0), 256, 0, s>>>(col, images, B, S, P, G);
    OMX_LAUNCH_CHECK();
    if (tower::gemm({col, cwr, cb, nullptr, patches, (int)R, d, K0, 0, 0, 0}, s)) return 1;
    sam_pos_add_kernel<<<grid_for(R * d), 256, 0, s>>>(h, patches, pos, B, G, Pg, d, Pg == G ? 0.f : (float)Pg / (float)G);
    OMX_LAUNCH_CHECK();
    launches += 3;
    if (keep) OMX_HIP_CHECK(hipMemcpyAsync(keep, h, (size_t)R * d * sizeof(float), hipMemcpyDeviceToDevice, s));
    // ---- blocks (vision.rs:243-267) ----
    for (int l = 0; l < c.depth; ++l) {
        const SamBlockW& b = bw[l];
        if (omx_layer_norm(ln, h, b.n1w, b.n1b, R, d, 1e-6f, OMX_FLOAT32, s)) return 1;
        if (tower::gemm({ln, b.qkvw, b.qkvb, nullptr, qkv, (int)R, 3 * d, d, 0, 0, 0}, s)) return 1;
        // a padded token is zero AFTER norm1: its q | k | v is the qkv Linear's bias
        if (sam_attention(att, d, qkv, 3 * d, B, G, G, c.num_heads, is_global(c, l) ? 0 : c.window, b.rh, b.Lh, b.rw, b.Lw, b.qkvb, s)) return 1;
        // h += att . Wp^T + bp, in place: each element is read, then written, by its own thread
        if (tower::gemm({att, b.pw, b.pb, h, h, (int)R, d, d, 0, 0, 0}, s)) return 1;
        if (omx_layer_norm(ln, h, b.n2w, b.n2b, R, d, 1e-6f, OMX_FLOAT32, s)) return 1;
        if (tower::gemm({ln, b.l1w, b.l1b, nullptr, mlp, (int)R, ffn, d, 0, 0, 2}, s)) return 1;
        if (tower::gemm({mlp, b.l2w, b.l2b, h, h, (int)R, d, ffn, 0, 0, 0}, s)) return 1;
        launches += 7;
        if (keep) OMX_HIP_CHECK(hipMemcpyAsync(keep + (size_t)(l + 1) * R * d, h, (size_t)R * d * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    // ---- neck (vision.rs:405-418): LayerNorm2d over the channels of a pixel is the row LayerNorm in NHWC ----
    if (tower::gemm({h, k0w, nullptr, nullptr, n0, (int)R, c1, d, 0, 0, 0}, s)) return 1;
    if (omx_layer_norm(n1, n0, k1w, k1b, R, c1, 1e-6f, OMX_FLOAT32, s)) return 1;
    launches += 2;
    auto conv3 = [&](float* y, const float* x, const float* w, int H, int ch, int OH, int Cout, int stride, int64_t rows, int64_t group) -> int {
        for (int64_t r0 = 0; r0 < rows; r0 += group) {
            const int64_t m = std::min(group, rows - r0);
            sam_im2col3_kernel<<<grid_for(m * 9 * ch / 4), 256, 0, s>>>(col, x, H, H, ch, OH, OH, stride, r0, m);
            OMX_LAUNCH_CHECK();
            if (tower::gemm({col, w, nullptr, nullptr, y + r0 * Cout, (int)m, Cout, 9 * ch, 0, 0, 0}, s)) return 1;
            launches += 2;
        }
        return 0;
    };
    if (conv3(n0, n1, k2r, G, c1, G, c1, 1, R, gA)) return 1;
    if (omx_layer_norm(n1, n0, k3w, k3b, R, c1, 1e-6f, OMX_FLOAT32, s)) return 1;
    launches += 1;
    // ---- the two stride-2 convolutions (vision.rs:420-427) ----
    if (conv3(d2, n1, n2r, G, c1, G2, c2, 2, R2, gB)) return 1;
    if (conv3(out, d2, n3r, G2, c2, G4, c3, 2, R4, gC)) return 1;
    OMX_HIP_CHECK(hipMemcpyAsync(out_rows, out, (size_t)R4 * c3 * sizeof(float), hipMemcpyDeviceToDevice, s));
    e->launches = launches;
    return 0;
}

int omx_sam_encoder_debug_read(omx_sam_encoder e, const char* name, float* host, size_t n_elems) {
    OMX_REQUIRE(e && name && host, "omx_sam_encoder_debug_read: null argument");
    const std::string s(name);
    const float* src = nullptr;
    size_t have = 0;
    const size_t slot = e->rows * (size_t)e->cfg.embed_dim;
    if (s == "patches") { src = e->sc.buf[S_PATCH]; have = e->sc.cap[S_PATCH]; }
    else if (s == "neck") { src = e->sc.buf[S_N1]; have = e->sc.cap[S_N1]; }
    else if (s == "out") { src = e->sc.buf[S_OUT]; have = e->sc.cap[S_OUT]; }
    else if (s == "h0" || s.rfind("block", 0) == 0) {
        OMX_REQUIRE(e->cfg.keep_stages, "omx_sam_encoder_debug_read: %s is kept only by an encoder created with keep_stages", name);
        int idx = 0;
        if (s != "h0") {
            const std::string t = s.substr(5);
            OMX_REQUIRE(!t.empty() && t.size() <= 4 && t.find_first_not_of("0123456789") == std::string::npos && atoi(t.c_str()) < e->cfg.depth,
                        "omx_sam_encoder_debug_read: unknown stage %s", name);
            idx = atoi(t.c_str()) + 1;
        }
        OMX_REQUIRE(e->sc.buf[S_KEEP] && (size_t)(idx + 1) * slot <= e->sc.cap[S_KEEP], "omx_sam_encoder_debug_read: no forward has run");
        src = e->sc.buf[S_KEEP] + (size_t)idx * slot; have = slot;
    } else return omx::set_error("omx_sam_encoder_debug_read: unknown stage %s", name);
    OMX_REQUIRE(src && n_elems <= have, "omx_sam_encoder_debug_read: %zu elements of %s, the buffer holds %zu", n_elems, name, have);
    OMX_HIP_CHECK(hipDeviceSynchronize());
    OMX_HIP_CHECK(hipMemcpy(host, src, n_elems * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

int omx_sam_attention_f32(float* out, int64_t ldo, const float* qkv, int64_t ld, int images, int gh, int gw, int heads, int width, int window,
                          const float* rel_pos_h, int len_h, const float* rel_pos_w, int len_w, const float* pad_qkv, omx_stream stream) {
    OMX_REQUIRE(width == 64, "InvalidConfig: sam attention: head width %d: the kernel is built for 64", width);
    return sam_attention(out, ldo, qkv, ld, images, gh, gw, heads, window, rel_pos_h, len_h, rel_pos_w, len_w, pad_qkv, (hipStream_t)stream);
}

}  // extern "C"
