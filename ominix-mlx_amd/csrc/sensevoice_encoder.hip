// The Fun-ASR-Nano audio tower (funasr-nano-mlx/src/sensevoice_encoder.rs:453-478 SenseVoiceEncoder::forward, then adaptor.rs:247-261
// AudioAdaptor::forward) in float32, as the reference runs it -- over up to 8 utterances in ONE pass.  The utterances' LFR rows are stacked
// into one [sum T, lfr_dim] tensor (SegTable, gemm.hpp).  What works on a row alone (every GEMM, LayerNorm, ReLU, residual) runs over all
// rows at once: a 5 s utterance is 84 rows, a third of the chip per GEMM; eight of them fill it.  What looks across rows stops at the
// utterance's first and last row:
//   positions   x[t] + PE(t_local + 1), no scale (SinusoidalPositionEncoder::forward :288-304 -- Paraformer's embed scales by sqrt(512))
//   attention   attn_f32_kernel's segment form (attn_f32.hip): one launch per layer, a query tile reads its own utterance's keys
//   FSMN        the segment forms of fsmn_add_kernel / f32_epilogue_ln_kernel (sanm_f32.hpp): zero padding inside the utterance
// The layer is SenseVoiceEncoderLayer::forward (:368-384): pre-norm, out_proj(attn) + (conv(v) + v), no attention residual on the
// lfr_dim -> output_size layer, ReLU FFN; with the fused tails of the Paraformer path where the width allows them (512 / 1024 / 2048).
// A GEMM's split of K depends on its row count, so the last bits of a row may depend on how many rows share the pass.
#include <math.h>

#include <map>
#include <string>
#include <vector>

#include "gemm.hpp"
#include "sanm_f32.hpp"
#include "workspace.hpp"

namespace {

using namespace omx;

constexpr int kAdaptorHeads = 8, kAdaptorFfn = 256;     // adaptor.rs:226-227

// out[t, c] = x[t, c] + PE(t - first row of t's utterance + 1)[c];  PE[p, i] = sin(p * ts_i), PE[p, half + i] = cos(p * ts_i),
// ts_i = exp(-i * ln(1e4) / (half - 1))   (sensevoice_encoder.rs:257-304; the operations of paraformer_embed_kernel without its scale)
__global__ __launch_bounds__(256) void pos_add_seg_kernel(float* __restrict__ out, const float* __restrict__ x, int T, int dim, SegTable sg) {
    const int half = dim / 2;
    const float inc = logf(10000.0f) / ((float)half - 1.0f);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < (int64_t)T * dim; i += (int64_t)gridDim.x * 256) {
        const int row = (int)(i / dim), c = (int)(i % dim);
        int lo, hi;
        seg_bounds(sg, row, lo, hi);
        const int k = c < half ? c : c - half;
        const float st = (float)(row - lo + 1) * expf(-(float)k * inc);
        out[i] = x[i] + (c < half ? sinf(st) : cosf(st));
    }
}

inline unsigned grid_for(int64_t n) { return (unsigned)std::min<int64_t>((n + 255) / 256, 8192); }

int gemm(float* out, const float* a, const float* w, const float* bias, const float* resid, int M, int N, int K, int relu, hipStream_t s) {
    GemmF32 p = {a, w, bias, resid, out, M, N, K, K, K, N, N, 0, 0, 0, 1, relu, 0, 1.0f};
    return launch_gemm_f32(p, s);
}

// the utterances of a host offset list, checked: every refusal before anything is launched
int make_segments(SegTable* sg, const char* fn, const int* seg, int n_utt) {
    OMX_REQUIRE(seg, "%s: null segment list", fn);
    OMX_REQUIRE(n_utt >= 1 && n_utt <= kMaxSegments, "InvalidConfig: %s: %d utterances in one pass (1..%d)", fn, n_utt, kMaxSegments);
    OMX_REQUIRE(seg[0] == 0, "%s: the first utterance must start at row 0 (seg[0] = %d)", fn, seg[0]);
    *sg = SegTable{};
    sg->n = n_utt;
    for (int u = 0; u < n_utt; ++u) {
        const int len = seg[u + 1] - seg[u];
        OMX_REQUIRE(len >= 1, "%s: utterance %d has %d rows (at least 1)", fn, u, len);
        OMX_REQUIRE(len <= kMaxSegmentRows, "InvalidConfig: %s: utterance %d has %d rows, above the %d the one-launch attention holds as keys "
                    "(30 s of audio make 501)", fn, u, len, kMaxSegmentRows);
    }
    for (int u = 0; u <= n_utt; ++u) sg->off[u] = seg[u];
    return 0;
}

// SenseVoiceEncoderLayer::forward over the stacked utterances of sg.  h1_pre: norm1(x), already computed by the previous layer's last
// launch; next_ln_* / next_h1: this layer's last launch also leaves LayerNorm(out) there (the next layer's norm1, after_norm or tp_norm) --
// encoder_layer_impl's handover (paraformer.hip).
int sanm_layer_seg(float* out, const float* x, const omx_sanm_layer_weights* w, const SegTable& sg, int in_dim, int dim, int heads, int ffn_dim,
                   int kernel_size, hipStream_t s, const float* h1_pre = nullptr, const float* next_ln_w = nullptr, const float* next_ln_b = nullptr,
                   float* next_h1 = nullptr) {
    const int T = sg.off[sg.n];
    const size_t need = ((size_t)T * (in_dim + 3 * dim + 4 * dim + ffn_dim) + 1024) * sizeof(float);
    void* ws = nullptr;
    if (get_workspace(&ws, need)) return 1;
    float* h1 = (float*)ws;                      // [T, in_dim]  norm1(x)
    float* qkv = h1 + (size_t)T * in_dim;        // [T, 3 dim]
    float* att = qkv + (size_t)T * 3 * dim;      // [T, dim]
    float* prj = att + (size_t)T * dim;          // [T, dim]
    float* xr = prj + (size_t)T * dim;           // [T, dim]  after the attention block
    float* h2 = xr + (size_t)T * dim;            // [T, dim]  norm2
    float* ff = h2 + (size_t)T * dim;            // [T, ffn_dim]
    const float* h1r = h1_pre;
    if (!h1r) {
        if (omx_layer_norm(h1, x, w->norm1_w, w->norm1_b, T, in_dim, 1e-5f, OMX_FLOAT32, s)) return 1;
        h1r = h1;
    }
    if (gemm(qkv, h1r, (const float*)w->qkv_w, (const float*)w->qkv_b, nullptr, T, 3 * dim, in_dim, 0, s)) return 1;
    if (launch_attn_f32_seg(att, qkv, qkv + dim, qkv + 2 * dim, 3 * (int64_t)dim, 3 * (int64_t)dim, dim, sg, heads, 1.0f / sqrtf(128.0f), s)) return 1;
    const float* skip = in_dim == dim ? x : nullptr;          // (:374-378: the first layer changes the width and has no skip connection)
    const bool fuse = fuse_f32_tails() && f32_tail_width_ok(dim);
    if (fuse) {
        // out_proj's split sum + bias, the FSMN block inside each utterance, the skip connection and norm2 in one launch behind the product
        F32Tail t; t.bias = (const float*)w->out_b; t.v = qkv + 2 * dim; t.ldv = 3 * (int64_t)dim; t.fw = (const float*)w->fsmn_w; t.ksize = kernel_size;
        t.resid2 = skip; t.ln_w = (const float*)w->norm2_w; t.ln_b = (const float*)w->norm2_b; t.ln_out = h2; t.seg = &sg;
        if (gemm_f32_with_tail(xr, att, (const float*)w->out_w, T, dim, dim, t, prj, s)) return 1;
    } else {
        if (gemm(prj, att, (const float*)w->out_w, (const float*)w->out_b, nullptr, T, dim, dim, 0, s)) return 1;
        fsmn_add_kernel<OMX_FLOAT32, true><<<1024, 256, 0, s>>>(xr, prj, qkv + 2 * dim, 3 * (int64_t)dim, (const float*)w->fsmn_w, T, dim, kernel_size, skip, sg);
        OMX_LAUNCH_CHECK();
        if (omx_layer_norm(h2, xr, w->norm2_w, w->norm2_b, T, dim, 1e-5f, OMX_FLOAT32, s)) return 1;
    }
    if (gemm(ff, h2, (const float*)w->ffn_up_w, (const float*)w->ffn_up_b, nullptr, T, ffn_dim, dim, 1, s)) return 1;
    if (next_h1 && fuse) {
        F32Tail t; t.bias = (const float*)w->ffn_down_b; t.resid = xr; t.ldr = dim; t.ln_w = next_ln_w; t.ln_b = next_ln_b; t.ln_out = next_h1;
        return gemm_f32_with_tail(out, ff, (const float*)w->ffn_down_w, T, dim, ffn_dim, t, nullptr, s);
    }
    if (gemm(out, ff, (const float*)w->ffn_down_w, (const float*)w->ffn_down_b, xr, T, dim, ffn_dim, 0, s)) return 1;
    if (next_h1) return omx_layer_norm(next_h1, out, next_ln_w, next_ln_b, T, dim, 1e-5f, OMX_FLOAT32, s);
    return 0;
}

int check_layer_shape(const char* fn, int in_dim, int dim, int heads, int ffn_dim, int kernel_size) {
    OMX_REQUIRE(in_dim >= 4 && dim >= 4 && heads >= 1 && ffn_dim >= 4, "InvalidConfig: %s: in_dim=%d dim=%d heads=%d ffn=%d", fn, in_dim, dim, heads, ffn_dim);
    OMX_REQUIRE(dim % heads == 0 && dim / heads == 128, "InvalidConfig: %s: head width %d (dim %d / %d heads): the float32 attention is built for 128",
                fn, dim / heads, dim, heads);
    OMX_REQUIRE(kernel_size >= 1 && kernel_size % 2 == 1 && kernel_size <= 31, "InvalidConfig: %s: kernel_size %d: an odd kernel_size <= 31 expected", fn, kernel_size);
    OMX_REQUIRE(in_dim % 4 == 0 && dim % 4 == 0 && ffn_dim % 4 == 0, "InvalidConfig: %s: widths must be multiples of 4 (in %d, dim %d, ffn %d)", fn, in_dim, dim, ffn_dim);
    return 0;
}

}  // namespace

struct omx_funasr_nano_encoder_ {
    omx_funasr_nano_encoder_config cfg;
    std::map<std::string, float*> w;              // device float32 tensors by key
    std::vector<float*> ad_qkv_w, ad_qkv_b;       // per adaptor block: linear_q | linear_k | linear_v stacked [3 llm, llm] / [3 llm]
    float* buf[12] = {};
    size_t cap[12] = {};
    size_t rows = 0;                              // rows of the last forward
};

namespace {

enum { B_POS = 0, B_ACT0, B_ACT1, B_NRM0, B_NRM1, B_AN, B_TP, B_A1, B_L2, B_HA, B_HB, B_T0, B_N };

int reserve(omx_funasr_nano_encoder e, int role, size_t elems, hipStream_t s) {
    if (elems <= e->cap[role]) return 0;
    OMX_HIP_CHECK(hipStreamSynchronize(s));
    if (e->buf[role]) OMX_HIP_CHECK(hipFree(e->buf[role]));
    e->buf[role] = nullptr; e->cap[role] = 0;
    OMX_HIP_CHECK(hipMalloc((void**)&e->buf[role], elems * sizeof(float)));
    e->cap[role] = elems;
    return 0;
}

// the shape the config implies for a key (empty: not a key of this model)
std::vector<int64_t> expected_shape(const omx_funasr_nano_encoder_config& c, const std::string& key) {
    const int64_t dim = c.output_size, ffn = c.linear_units, llm = c.llm_dim;
    auto norm = [](const std::string& r, const char* name, int64_t n, std::vector<int64_t>* out) {
        if (r == std::string(name) + ".weight" || r == std::string(name) + ".bias") { *out = {n}; return true; }
        return false;
    };
    auto linear = [](const std::string& r, const char* name, int64_t n_out, int64_t n_in, std::vector<int64_t>* out) {
        if (r == std::string(name) + ".weight") { *out = {n_out, n_in}; return true; }
        if (r == std::string(name) + ".bias") { *out = {n_out}; return true; }
        return false;
    };
    // "<group>.<index>.<rest>" -> index, rest
    auto indexed = [](const std::string& k, const char* group, int count, std::string* rest) {
        const std::string g = std::string(group) + ".";
        if (k.rfind(g, 0) != 0) return false;
        const size_t dot = k.find('.', g.size());
        if (dot == std::string::npos || dot == g.size()) return false;
        const std::string idx = k.substr(g.size(), dot - g.size());
        if (idx.size() > 6 || idx.find_first_not_of("0123456789") != std::string::npos) return false;
        if (atoi(idx.c_str()) >= count) return false;
        *rest = k.substr(dot + 1);
        return true;
    };
    std::vector<int64_t> sh;
    if (key.rfind("encoder.", 0) == 0) {
        const std::string k = key.substr(8);
        if (norm(k, "after_norm", dim, &sh) || norm(k, "tp_norm", dim, &sh)) return sh;
        std::string r;
        int64_t in_dim = dim;
        if (indexed(k, "encoders0", 1, &r)) in_dim = c.lfr_dim;
        else if (!indexed(k, "encoders", c.num_blocks - 1, &r) && !indexed(k, "tp_encoders", c.tp_blocks, &r)) return {};
        if (norm(r, "norm1", in_dim, &sh) || norm(r, "norm2", dim, &sh) || linear(r, "self_attn.linear_q_k_v", 3 * dim, in_dim, &sh) ||
            linear(r, "self_attn.linear_out", dim, dim, &sh) || linear(r, "feed_forward.w_1", ffn, dim, &sh) || linear(r, "feed_forward.w_2", dim, ffn, &sh))
            return sh;
        if (r == "self_attn.fsmn.weight") return {dim, 1, c.kernel_size};
        return {};
    }
    if (key.rfind("adaptor.", 0) == 0) {
        const std::string k = key.substr(8);
        if (linear(k, "linear1", c.ffn_dim, c.encoder_dim, &sh) || linear(k, "linear2", llm, c.ffn_dim, &sh)) return sh;
        std::string r;
        if (!indexed(k, "blocks", c.n_layer, &r)) return {};
        if (norm(r, "norm1", llm, &sh) || norm(r, "norm2", llm, &sh) || linear(r, "self_attn.linear_q", llm, llm, &sh) ||
            linear(r, "self_attn.linear_k", llm, llm, &sh) || linear(r, "self_attn.linear_v", llm, llm, &sh) || linear(r, "self_attn.linear_out", llm, llm, &sh) ||
            linear(r, "feed_forward.w_1", kAdaptorFfn, llm, &sh) || linear(r, "feed_forward.w_2", llm, kAdaptorFfn, &sh))
            return sh;
    }
    return {};
}

const float* weight(omx_funasr_nano_encoder e, const std::string& name, int* err) {
    if (*err) return nullptr;                     // the first missing tensor is the one reported
    auto it = e->w.find(name);
    if (it == e->w.end()) { *err = omx::set_error("WeightNotFound: %s", name.c_str()); return nullptr; }
    return it->second;
}

int layer_weights(omx_funasr_nano_encoder e, const std::string& p, omx_sanm_layer_weights* w) {
    int err = 0;
    auto W = [&](const char* r) { return (const void*)weight(e, p + r, &err); };
    w->norm1_w = W("norm1.weight"); w->norm1_b = W("norm1.bias");
    w->qkv_w = W("self_attn.linear_q_k_v.weight"); w->qkv_b = W("self_attn.linear_q_k_v.bias");
    w->out_w = W("self_attn.linear_out.weight"); w->out_b = W("self_attn.linear_out.bias");
    w->fsmn_w = W("self_attn.fsmn.weight");
    w->norm2_w = W("norm2.weight"); w->norm2_b = W("norm2.bias");
    w->ffn_up_w = W("feed_forward.w_1.weight"); w->ffn_up_b = W("feed_forward.w_1.bias");
    w->ffn_down_w = W("feed_forward.w_2.weight"); w->ffn_down_b = W("feed_forward.w_2.bias");
    return err;
}

}  // namespace

extern "C" {

int omx_funasr_nano_encoder_create(omx_funasr_nano_encoder* out, const omx_funasr_nano_encoder_config* cfg) {
    OMX_REQUIRE(out && cfg, "omx_funasr_nano_encoder_create: null argument");
    const omx_funasr_nano_encoder_config& c = *cfg;
    OMX_REQUIRE(c.num_blocks >= 1 && c.tp_blocks >= 0 && c.n_layer >= 0 && c.attention_heads >= 1,
                "InvalidConfig: funasr-nano encoder num_blocks=%d tp_blocks=%d n_layer=%d heads=%d", c.num_blocks, c.tp_blocks, c.n_layer, c.attention_heads);
    if (check_layer_shape("funasr-nano encoder", c.lfr_dim, c.output_size, c.attention_heads, c.linear_units, c.kernel_size)) return 1;
    OMX_REQUIRE(c.encoder_dim == c.output_size, "InvalidConfig: funasr-nano adaptor: encoder_dim %d is not the encoder's output_size %d", c.encoder_dim, c.output_size);
    OMX_REQUIRE(c.ffn_dim >= 4 && c.ffn_dim % 4 == 0 && c.llm_dim >= 4 && c.llm_dim % 4 == 0, "InvalidConfig: funasr-nano adaptor: ffn_dim %d / llm_dim %d must be multiples of 4",
                c.ffn_dim, c.llm_dim);
    OMX_REQUIRE(c.llm_dim % kAdaptorHeads == 0 && c.llm_dim / kAdaptorHeads == 128,
                "InvalidConfig: funasr-nano adaptor: head width %d (llm_dim %d / %d heads): the float32 attention is built for 128", c.llm_dim / kAdaptorHeads,
                c.llm_dim, kAdaptorHeads);
    omx_funasr_nano_encoder e = new omx_funasr_nano_encoder_();
    e->cfg = c;
    e->ad_qkv_w.assign(c.n_layer, nullptr);
    e->ad_qkv_b.assign(c.n_layer, nullptr);
    *out = e;
    return 0;
}

int omx_funasr_nano_encoder_destroy(omx_funasr_nano_encoder e) {
    if (!e) return 0;
    (void)hipDeviceSynchronize();
    for (auto& kv : e->w) (void)hipFree(kv.second);
    for (float* p : e->ad_qkv_w) if (p) (void)hipFree(p);
    for (float* p : e->ad_qkv_b) if (p) (void)hipFree(p);
    for (float* p : e->buf) if (p) (void)hipFree(p);
    delete e;
    return 0;
}

int omx_funasr_nano_encoder_load(omx_funasr_nano_encoder e, const char* name, const float* host, const int64_t* shape, int ndim) {
    OMX_REQUIRE(e && name, "omx_funasr_nano_encoder_load: null argument");
    OMX_REQUIRE(host && shape, "omx_funasr_nano_encoder_load: %s: null tensor", name);
    OMX_REQUIRE(ndim >= 1 && ndim <= 4, "omx_funasr_nano_encoder_load: %s: %d dimensions", name, ndim);
    const std::string key(name);
    const std::vector<int64_t> want = expected_shape(e->cfg, key);
    OMX_REQUIRE(!want.empty(), "omx_funasr_nano_encoder_load: %s is not a tensor of this model (encoder.* / adaptor.* after the key map, layer indices "
                "inside the config's counts)", name);
    // dimensions of 1 do not count: the FSMN taps come as [dim, 1, k] or [dim, k]
    std::vector<int64_t> got, exp;
    for (int i = 0; i < ndim; ++i) if (shape[i] != 1) got.push_back(shape[i]);
    for (int64_t d : want) if (d != 1) exp.push_back(d);
    std::string gs, ws;
    for (int i = 0; i < ndim; ++i) gs += (i ? ", " : "") + std::to_string(shape[i]);
    for (size_t i = 0; i < want.size(); ++i) ws += (i ? ", " : "") + std::to_string(want[i]);
    OMX_REQUIRE(got == exp, "ShapeMismatch: %s has shape [%s], the config expects [%s]", name, gs.c_str(), ws.c_str());
    size_t n = 1;
    for (int64_t d : want) n *= (size_t)d;
    auto it = e->w.find(key);
    if (it != e->w.end()) { (void)hipDeviceSynchronize(); (void)hipFree(it->second); e->w.erase(it); }
    float* dev = nullptr;
    OMX_HIP_CHECK(hipMalloc((void**)&dev, n * sizeof(float)));
    if (hipMemcpy(dev, host, n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(dev);
        return omx::set_error("omx_funasr_nano_encoder_load: %s: copy to the device failed", name);
    }
    e->w[key] = dev;
    // a q / k / v projection of the adaptor changed: the block's stacked copy is rebuilt at the next forward
    for (int l = 0; l < e->cfg.n_layer; ++l)
        if (key.rfind("adaptor.blocks." + std::to_string(l) + ".self_attn.", 0) == 0 && e->ad_qkv_w[l]) {
            (void)hipDeviceSynchronize();
            (void)hipFree(e->ad_qkv_w[l]); (void)hipFree(e->ad_qkv_b[l]);
            e->ad_qkv_w[l] = e->ad_qkv_b[l] = nullptr;
        }
    return 0;
}

int omx_funasr_nano_encoder_forward(omx_funasr_nano_encoder e, const float* lfr_rows, const int* seg, int n_utt, float* out_rows, omx_stream stream) {
    OMX_REQUIRE(e && lfr_rows && out_rows, "omx_funasr_nano_encoder_forward: null argument");
    SegTable sg;
    if (make_segments(&sg, "omx_funasr_nano_encoder_forward", seg, n_utt)) return 1;
    hipStream_t s = (hipStream_t)stream;
    const omx_funasr_nano_encoder_config& c = e->cfg;
    const int T = sg.off[sg.n], lfr = c.lfr_dim, dim = c.output_size, heads = c.attention_heads, ffn = c.linear_units, ks = c.kernel_size;
    const int llm = c.llm_dim;

    // ---- every tensor resolved before the first launch ----
    const int n_main = c.num_blocks, n_tp = c.tp_blocks;
    std::vector<omx_sanm_layer_weights> layers(n_main + n_tp);
    if (layer_weights(e, "encoder.encoders0.0.", &layers[0])) return 1;
    for (int l = 1; l < n_main; ++l) if (layer_weights(e, "encoder.encoders." + std::to_string(l - 1) + ".", &layers[l])) return 1;
    for (int l = 0; l < n_tp; ++l) if (layer_weights(e, "encoder.tp_encoders." + std::to_string(l) + ".", &layers[n_main + l])) return 1;
    int err = 0;
    auto W = [&](const std::string& name) { return weight(e, name, &err); };
    const float* anw = W("encoder.after_norm.weight"); const float* anb = W("encoder.after_norm.bias");
    const float* tnw = W("encoder.tp_norm.weight"); const float* tnb = W("encoder.tp_norm.bias");
    const float* l1w = W("adaptor.linear1.weight"); const float* l1b = W("adaptor.linear1.bias");
    const float* l2w = W("adaptor.linear2.weight"); const float* l2b = W("adaptor.linear2.bias");
    struct Block { const float *n1w, *n1b, *ow, *ob, *n2w, *n2b, *f1w, *f1b, *f2w, *f2b; };
    std::vector<Block> blocks(c.n_layer);
    for (int l = 0; l < c.n_layer; ++l) {
        const std::string p = "adaptor.blocks." + std::to_string(l) + ".";
        Block& b = blocks[l];
        b.n1w = W(p + "norm1.weight"); b.n1b = W(p + "norm1.bias");
        b.ow = W(p + "self_attn.linear_out.weight"); b.ob = W(p + "self_attn.linear_out.bias");
        b.n2w = W(p + "norm2.weight"); b.n2b = W(p + "norm2.bias");
        b.f1w = W(p + "feed_forward.w_1.weight"); b.f1b = W(p + "feed_forward.w_1.bias");
        b.f2w = W(p + "feed_forward.w_2.weight"); b.f2b = W(p + "feed_forward.w_2.bias");
        const char* nm[3] = {"linear_q", "linear_k", "linear_v"};
        const float *pw[3], *pb[3];
        for (int i = 0; i < 3; ++i) { pw[i] = W(p + "self_attn." + nm[i] + ".weight"); pb[i] = W(p + "self_attn." + nm[i] + ".bias"); }
        if (err) return 1;
        if (!e->ad_qkv_w[l]) {
            OMX_HIP_CHECK(hipMalloc((void**)&e->ad_qkv_w[l], (size_t)3 * llm * llm * sizeof(float)));
            OMX_HIP_CHECK(hipMalloc((void**)&e->ad_qkv_b[l], (size_t)3 * llm * sizeof(float)));
            for (int i = 0; i < 3; ++i) {
                OMX_HIP_CHECK(hipMemcpyAsync(e->ad_qkv_w[l] + (size_t)i * llm * llm, pw[i], (size_t)llm * llm * sizeof(float), hipMemcpyDeviceToDevice, s));
                OMX_HIP_CHECK(hipMemcpyAsync(e->ad_qkv_b[l] + (size_t)i * llm, pb[i], (size_t)llm * sizeof(float), hipMemcpyDeviceToDevice, s));
            }
        }
    }
    if (err) return 1;

    const size_t wide = (size_t)std::max(lfr, dim);
    if (reserve(e, B_POS, (size_t)T * lfr, s) || reserve(e, B_ACT0, (size_t)T * dim, s) || reserve(e, B_ACT1, (size_t)T * dim, s) ||
        reserve(e, B_NRM0, (size_t)T * wide, s) || reserve(e, B_NRM1, (size_t)T * wide, s) || reserve(e, B_AN, (size_t)T * dim, s) ||
        reserve(e, B_TP, (size_t)T * dim, s) || reserve(e, B_A1, (size_t)T * c.ffn_dim, s) || reserve(e, B_L2, (size_t)T * llm, s) ||
        reserve(e, B_HA, (size_t)T * llm, s) || reserve(e, B_HB, (size_t)T * llm, s) || reserve(e, B_T0, (size_t)T * 4 * llm, s))
        return 1;
    e->rows = (size_t)T;
    float *pos = e->buf[B_POS], *an = e->buf[B_AN], *tp = e->buf[B_TP], *a1 = e->buf[B_A1], *l2 = e->buf[B_L2], *ha = e->buf[B_HA], *hb = e->buf[B_HB];
    float* act[2] = {e->buf[B_ACT0], e->buf[B_ACT1]};
    float* nrm[2] = {e->buf[B_NRM0], e->buf[B_NRM1]};

    pos_add_seg_kernel<<<grid_for((int64_t)T * lfr), 256, 0, s>>>(pos, lfr_rows, T, lfr, sg);
    OMX_LAUNCH_CHECK();

    // ---- encoders0 + encoders -> after_norm ; tp_encoders -> tp_norm: each layer's last launch leaves the next norm of its output ----
    const float* h = pos;
    const float* pre = nullptr;
    int d_in = lfr;
    for (int l = 0; l < n_main; ++l) {
        const bool last = l + 1 == n_main;
        float* nh = last ? an : nrm[l & 1];
        if (sanm_layer_seg(act[l & 1], h, &layers[l], sg, d_in, dim, heads, ffn, ks, s, pre, last ? anw : (const float*)layers[l + 1].norm1_w,
                           last ? anb : (const float*)layers[l + 1].norm1_b, nh))
            return 1;
        h = act[l & 1]; pre = nh; d_in = dim;
    }
    h = an; pre = nullptr;                      // the tp layers work on the NORMALISED rows (:469-474): after_norm's output is their x
    for (int l = 0; l < n_tp; ++l) {
        const bool last = l + 1 == n_tp;
        const omx_sanm_layer_weights* nx = last ? nullptr : &layers[n_main + l + 1];
        float* nh = last ? tp : nrm[l & 1];
        if (sanm_layer_seg(act[l & 1], h, &layers[n_main + l], sg, dim, dim, heads, ffn, ks, s, pre, last ? tnw : (const float*)nx->norm1_w,
                           last ? tnb : (const float*)nx->norm1_b, nh))
            return 1;
        h = act[l & 1]; pre = nh;
    }
    if (n_tp == 0 && omx_layer_norm(tp, an, tnw, tnb, T, dim, 1e-5f, OMX_FLOAT32, s)) return 1;

    // ---- adaptor: linear1 + ReLU, linear2, pre-norm blocks (adaptor.rs:247-261, :176-187) ----
    if (gemm(a1, tp, l1w, l1b, nullptr, T, c.ffn_dim, dim, 1, s)) return 1;
    if (gemm(l2, a1, l2w, l2b, nullptr, T, llm, c.ffn_dim, 0, s)) return 1;
    if (c.n_layer == 0) {
        OMX_HIP_CHECK(hipMemcpyAsync(out_rows, l2, (size_t)T * llm * sizeof(float), hipMemcpyDeviceToDevice, s));
        return 0;
    }
    float* qkv = e->buf[B_T0];                  // [T, 3 llm]
    float* t1 = qkv + (size_t)T * 3 * llm;      // [T, llm]
    const float* hin = l2;
    for (int l = 0; l < c.n_layer; ++l) {
        const Block& b = blocks[l];
        float* hout = l + 1 == c.n_layer ? out_rows : hb;
        if (omx_layer_norm(t1, hin, b.n1w, b.n1b, T, llm, 1e-5f, OMX_FLOAT32, s)) return 1;
        if (gemm(qkv, t1, e->ad_qkv_w[l], e->ad_qkv_b[l], nullptr, T, 3 * llm, llm, 0, s)) return 1;
        if (launch_attn_f32_seg(t1, qkv, qkv + llm, qkv + 2 * llm, 3 * (int64_t)llm, 3 * (int64_t)llm, llm, sg, kAdaptorHeads, 1.0f / sqrtf(128.0f), s)) return 1;
        if (gemm(ha, t1, b.ow, b.ob, hin, T, llm, llm, 0, s)) return 1;                         // residual + attention
        if (omx_layer_norm(t1, ha, b.n2w, b.n2b, T, llm, 1e-5f, OMX_FLOAT32, s)) return 1;
        if (gemm(qkv, t1, b.f1w, b.f1b, nullptr, T, kAdaptorFfn, llm, 1, s)) return 1;          // (the FFN's 256 columns in the free projection buffer)
        if (gemm(hout, qkv, b.f2w, b.f2b, ha, T, llm, kAdaptorFfn, 0, s)) return 1;
        hin = hout;
    }
    return 0;
}

int omx_funasr_nano_encoder_debug_read(omx_funasr_nano_encoder e, const char* name, float* host, size_t n_elems) {
    OMX_REQUIRE(e && name && host, "omx_funasr_nano_encoder_debug_read: null argument");
    const std::string s(name);
    const omx_funasr_nano_encoder_config& c = e->cfg;
    const int role = s == "pos" ? B_POS : s == "after_norm" ? B_AN : s == "tp_norm" ? B_TP : s == "linear2" ? B_L2 : -1;
    OMX_REQUIRE(role >= 0, "omx_funasr_nano_encoder_debug_read: unknown stage %s", name);
    const size_t width = role == B_POS ? c.lfr_dim : role == B_L2 ? c.llm_dim : c.output_size;
    OMX_REQUIRE(e->buf[role] && n_elems <= e->rows * width, "omx_funasr_nano_encoder_debug_read: %zu elements of %s, the last forward made %zu", n_elems, name,
                e->rows * width);
    OMX_HIP_CHECK(hipDeviceSynchronize());
    OMX_HIP_CHECK(hipMemcpy(host, e->buf[role], n_elems * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

int omx_segment_attention_f32(float* out, const float* q, const float* k, const float* v, int64_t ldq, int64_t ldkv, int64_t ldo, const int* seg,
                              int n_utt, int heads, omx_stream stream) {
    OMX_REQUIRE(out && q && k && v, "omx_segment_attention_f32: null argument");
    SegTable sg;
    if (make_segments(&sg, "omx_segment_attention_f32", seg, n_utt)) return 1;
    return launch_attn_f32_seg(out, q, k, v, ldq, ldkv, ldo, sg, heads, 1.0f / sqrtf(128.0f), (hipStream_t)stream);
}

int omx_sanm_segment_layer_f32(float* out, const float* x, const omx_sanm_layer_weights* w, const int* seg, int n_utt, int in_dim, int dim,
                               int heads, int ffn_dim, int kernel_size, omx_stream stream) {
    OMX_REQUIRE(out && x && w, "omx_sanm_segment_layer_f32: null argument");
    OMX_REQUIRE(w->norm1_w && w->norm1_b && w->qkv_w && w->qkv_b && w->out_w && w->out_b && w->fsmn_w && w->norm2_w && w->norm2_b && w->ffn_up_w &&
                w->ffn_up_b && w->ffn_down_w && w->ffn_down_b, "omx_sanm_segment_layer_f32: null tensor in the layer's weights");
    if (check_layer_shape("omx_sanm_segment_layer_f32", in_dim, dim, heads, ffn_dim, kernel_size)) return 1;
    SegTable sg;
    if (make_segments(&sg, "omx_sanm_segment_layer_f32", seg, n_utt)) return 1;
    return sanm_layer_seg(out, x, w, sg, in_dim, dim, heads, ffn_dim, kernel_size, (hipStream_t)stream);
}

}  // extern "C"
