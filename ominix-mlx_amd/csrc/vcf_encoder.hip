// The visual-causal-flow encoder of DeepSeek-OCR-2 (deepseek-ocr2-mlx/src/qwen2_encoder.rs, `Qwen2Encoder::forward_vision` :198-244): a
// Qwen2 decoder used as an encoder over B stacked images, in float32 like the SAM tower in front of it (sam_encoder.hip).  Per image the
// sequence is its n_img rows followed by a learned query table (query_768 for exactly 144 rows, query_1024 otherwise, :209-213); image rows
// see each other, a query row sees every image row and the query rows up to itself (:249-288); only the query rows come out, after the
// final RMSNorm.
// Per layer, nine launches (a product that splits K adds its reduce launch), GEMMs and norms over all B * L rows:
//   RMSNorm | q | k | v GEMM (+ bias; the three Linears stacked at load into one [(heads + 2 kv) * 64, hidden] matrix) | RoPE in place on
//   the q and k columns | attention | o_proj GEMM (+ residual) | RMSNorm | gate | up GEMM (stacked at load) | SwiGLU | down GEMM (+ residual)
// RoPE is its own small launch, from a cos / sin table [L, 32] computed once per sequence length in double precision on the host:
// non-traditional pairs (i, i + 32) over the full 64 dims, theta_i = base^(-i / 32), positions 0 .. L - 1 across image rows and queries.
// The attention is attn_stream_f32.hpp in its prefix form: row i sees keys j < max(n_prefix, i + 1), query head h reads key/value head
// h / (heads / kv_heads), the [L, L] mask is never built.
#include <math.h>

#include "attn_stream_f32.hpp"
#include "tower_f32.hpp"

namespace {

using namespace omx;
using tower::grid_for;

// h [B * L, d]: per image its n_img rows, then the query table
__global__ void vcf_assemble_kernel(float* __restrict__ h, const float* __restrict__ x, const float* __restrict__ query, int B, int n_img, int n_query, int d) {
    const int L = n_img + n_query;
    const int64_t n = (int64_t)B * L * d;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int col = (int)(i % d), r = (int)((i / d) % L), b = (int)(i / ((int64_t)d * L));
        h[i] = r < n_img ? x[((int64_t)b * n_img + r) * d + col] : query[(int64_t)(r - n_img) * d + col];
    }
}

// the query rows of every image, contiguous
__global__ void vcf_query_rows_kernel(float* __restrict__ out, const float* __restrict__ h, int B, int n_img, int n_query, int d) {
    const int L = n_img + n_query;
    const int64_t n = (int64_t)B * n_query * d;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int col = (int)(i % d), r = (int)((i / d) % n_query), b = (int)(i / ((int64_t)d * n_query));
        out[i] = h[((int64_t)b * L + n_img + r) * d + col];
    }
}

// nn::Rope, traditional = false, over the first n_heads heads of 64 of every row, in place: row r is position r % L
__global__ void vcf_rope_kernel(float* __restrict__ qkv, int64_t ld, int64_t rows, int L, int n_heads, const float* __restrict__ cs) {
    const int64_t n = rows * n_heads * 32;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int j = (int)(i % 32), hd = (int)((i / 32) % n_heads);
        const int64_t r = i / ((int64_t)32 * n_heads);
        const int pos = (int)(r % L);
        const float c = cs[(pos * 32 + j) * 2], sn = cs[(pos * 32 + j) * 2 + 1];
        float* p = qkv + r * ld + hd * 64 + j;
        const float x1 = p[0], x2 = p[32];
        p[0] = x1 * c - x2 * sn;
        p[32] = x1 * sn + x2 * c;
    }
}

// fused_swiglu(up, gate) = silu(gate) * up (qwen2_encoder.rs:136-141) over rows of [gate | up]
__global__ void vcf_swiglu_kernel(float* __restrict__ act, const float* __restrict__ gu, int64_t rows, int I) {
    const int64_t n = rows * I;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / I;
        const int col = (int)(i % I);
        const float gt = gu[r * 2 * I + col], up = gu[r * 2 * I + I + col];
        act[i] = gt / (1.0f + expf(-gt)) * up;
    }
}

int prefix_attention(float* out, int64_t ldo, const float* qkv, int64_t ld, int images, int L, int heads, int kv_heads, int n_prefix, hipStream_t s) {
    OMX_REQUIRE(out && qkv, "prefix-causal attention: null tensor");
    OMX_REQUIRE(images >= 1 && L >= 1 && heads >= 1 && kv_heads >= 1 && heads % kv_heads == 0 && n_prefix >= 0 && n_prefix <= L,
                "InvalidConfig: prefix-causal attention: images=%d rows=%d heads=%d kv_heads=%d prefix=%d", images, L, heads, kv_heads, n_prefix);
    OMX_REQUIRE(ld >= (int64_t)(heads + 2 * kv_heads) * 64 && ldo >= (int64_t)heads * 64, "prefix-causal attention: leading dimensions %lld / %lld below (heads + 2 kv_heads) * 64 = %d / heads * 64 = %d",
                (long long)ld, (long long)ldo, (heads + 2 * kv_heads) * 64, heads * 64);
    StreamAttn a = {};
    a.qkv = qkv; a.out = out; a.ld = ld; a.ldo = ldo;
    a.qoff = 0; a.koff = heads * 64; a.voff = (heads + kv_heads) * 64;
    a.heads = heads; a.group = heads / kv_heads; a.n = L; a.dom = L; a.n_prefix = n_prefix;
    a.nwx = a.nwy = 1;
    a.scale = 0.125f;
    return launch_stream_attn(SA_PREFIX, a, images, s);
}

enum { V_H = 0, V_LN, V_QKV, V_ATT, V_GU, V_ACT, V_TMP, V_OUT, V_KEEP, V_ROLES };
enum { M_QW = 1, M_KW = 2, M_VW = 4, M_QB = 8, M_KB = 16, M_VB = 32, M_GATE = 64, M_UP = 128 };

struct VcfLayer {
    float *qkv_w = nullptr, *qkv_b = nullptr, *gu_w = nullptr;   // q | k | v and gate | up, stacked as the parts arrive
    int have = 0;
};

}  // namespace

struct omx_vcf_encoder_ {
    omx_vcf_config cfg;
    tower::Store st;
    std::vector<VcfLayer> layer;
    std::map<int, float*> rope;                   // cos | sin pairs [L, 32, 2] by sequence length
    tower::Scratch<V_ROLES> sc;
    int launches = 0;
    size_t rows = 0;                              // B * L of the last forward
    ~omx_vcf_encoder_() {
        for (auto& l : layer) { if (l.qkv_w) (void)hipFree(l.qkv_w); if (l.qkv_b) (void)hipFree(l.qkv_b); if (l.gu_w) (void)hipFree(l.gu_w); }
        for (auto& kv : rope) (void)hipFree(kv.second);
    }
};

namespace {

// "model.model.layers.<n>.<rest>" -> n, rest
bool layer_key(const std::string& k, int layers, int* n, std::string* rest) {
    const std::string g = "model.model.layers.";
    if (k.rfind(g, 0) != 0) return false;
    const size_t dot = k.find('.', g.size());
    if (dot == std::string::npos || dot == g.size()) return false;
    const std::string idx = k.substr(g.size(), dot - g.size());
    if (idx.size() > 6 || idx.find_first_not_of("0123456789") != std::string::npos || atoi(idx.c_str()) >= layers) return false;
    *n = atoi(idx.c_str());
    *rest = k.substr(dot + 1);
    return true;
}

// a part of a stacked matrix: rows [row0, row0 + rows) of `cols` floats each
int load_part(float** dst, size_t total_rows, size_t row0, size_t rows, size_t cols, const char* name, const float* host, const int64_t* shp, int ndim) {
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) n *= (size_t)std::max<int64_t>(shp[i], 0);
    OMX_REQUIRE(n == rows * cols, "ShapeMismatch: %s has %zu elements, the config expects %zu", name, n, rows * cols);
    if (!*dst) OMX_HIP_CHECK(hipMalloc((void**)dst, total_rows * cols * sizeof(float)));
    else OMX_HIP_CHECK(hipDeviceSynchronize());
    OMX_HIP_CHECK(hipMemcpy(*dst + row0 * cols, host, n * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

}  // namespace

extern "C" {

int omx_vcf_encoder_create(omx_vcf_encoder* out, const omx_vcf_config* cfg) {
    OMX_REQUIRE(out && cfg, "omx_vcf_encoder_create: null argument");
    const omx_vcf_config& c = *cfg;
    OMX_REQUIRE(c.hidden >= 4 && c.layers >= 1 && c.heads >= 1 && c.kv_heads >= 1 && c.intermediate >= 4 && c.rope_theta > 0.f && c.eps > 0.f,
                "InvalidConfig: vcf encoder hidden=%d layers=%d heads=%d kv_heads=%d intermediate=%d rope_theta=%g eps=%g", c.hidden, c.layers, c.heads,
                c.kv_heads, c.intermediate, c.rope_theta, c.eps);
    OMX_REQUIRE(c.hidden == c.heads * 64, "InvalidConfig: vcf encoder head width %d (hidden %d / %d heads): the attention kernel is built for 64", c.hidden / c.heads,
                c.hidden, c.heads);
    OMX_REQUIRE(c.heads % c.kv_heads == 0, "InvalidConfig: vcf encoder: %d heads over %d key/value heads", c.heads, c.kv_heads);
    OMX_REQUIRE(c.hidden % 4 == 0 && c.intermediate % 4 == 0, "InvalidConfig: vcf encoder widths %d / %d are no multiples of 4", c.hidden, c.intermediate);
    omx_vcf_encoder e = new omx_vcf_encoder_();
    e->cfg = c;
    e->cfg.key_prefix[sizeof(e->cfg.key_prefix) - 1] = 0;
    e->st.prefix = e->cfg.key_prefix;
    if (!e->st.prefix.empty() && e->st.prefix.back() != '.') e->st.prefix += '.';
    e->layer.resize(c.layers);
    *out = e;
    return 0;
}

int omx_vcf_encoder_destroy(omx_vcf_encoder e) {
    if (!e) return 0;
    (void)hipDeviceSynchronize();
    delete e;
    return 0;
}

int omx_vcf_encoder_load(omx_vcf_encoder e, const char* name, const float* host, const int64_t* shape, int ndim) {
    OMX_REQUIRE(e && name && host && shape && ndim >= 1 && ndim <= 4, "omx_vcf_encoder_load: bad argument");
    const omx_vcf_config& c = e->cfg;
    int l = 0;
    std::string rest;
    if (layer_key(name, c.layers, &l, &rest)) {
        VcfLayer& L = e->layer[l];
        const size_t H = (size_t)c.heads * 64, KV = (size_t)c.kv_heads * 64, d = c.hidden, I = c.intermediate, NQ = H + 2 * KV;
        struct Part { const char* leaf; float** dst; size_t total, row0, rows, cols; int bit; };
        const Part parts[] = {
            {"self_attn.q_proj.weight", &L.qkv_w, NQ, 0, H, d, M_QW}, {"self_attn.k_proj.weight", &L.qkv_w, NQ, H, KV, d, M_KW},
            {"self_attn.v_proj.weight", &L.qkv_w, NQ, H + KV, KV, d, M_VW}, {"self_attn.q_proj.bias", &L.qkv_b, NQ, 0, H, 1, M_QB},
            {"self_attn.k_proj.bias", &L.qkv_b, NQ, H, KV, 1, M_KB}, {"self_attn.v_proj.bias", &L.qkv_b, NQ, H + KV, KV, 1, M_VB},
            {"mlp.gate_proj.weight", &L.gu_w, 2 * I, 0, I, d, M_GATE}, {"mlp.up_proj.weight", &L.gu_w, 2 * I, I, I, d, M_UP}};
        for (const Part& p : parts)
            if (rest == p.leaf) {
                if (load_part(p.dst, p.total, p.row0, p.rows, p.cols, name, host, shape, ndim)) return 1;
                L.have |= p.bit;
                return 0;
            }
    }
    return e->st.load("omx_vcf_encoder_load", name, host, shape, ndim);
}

int omx_vcf_encoder_tokens(omx_vcf_encoder e, int n_img, int* n_query, int* seq_len) {
    OMX_REQUIRE(e && n_query && seq_len && n_img >= 1, "omx_vcf_encoder_tokens: bad argument");
    const char* key = n_img == 144 ? "query_768.weight" : "query_1024.weight";       // qwen2_encoder.rs:209-213
    const size_t n = e->st.count(key);
    OMX_REQUIRE(n, "WeightNotFound: %s%s", e->st.prefix.c_str(), key);
    OMX_REQUIRE(n % e->cfg.hidden == 0, "ShapeMismatch: %s%s has %zu elements: no rows of %d", e->st.prefix.c_str(), key, n, e->cfg.hidden);
    *n_query = (int)(n / e->cfg.hidden);
    *seq_len = n_img + *n_query;
    return 0;
}

int omx_vcf_encoder_launches(omx_vcf_encoder e, int* n) {
    OMX_REQUIRE(e && n, "omx_vcf_encoder_launches: null argument");
    *n = e->launches;
    return 0;
}

int omx_vcf_encoder_scratch_bytes(omx_vcf_encoder e, size_t* bytes) {
    OMX_REQUIRE(e && bytes, "omx_vcf_encoder_scratch_bytes: null argument");
    *bytes = e->sc.bytes();
    return 0;
}

int omx_vcf_encoder_forward(omx_vcf_encoder e, const float* x, int n_images, int n_img, float* out_rows, omx_stream stream) {
    OMX_REQUIRE(e && x && out_rows, "omx_vcf_encoder_forward: null argument");
    hipStream_t s = (hipStream_t)stream;
    const omx_vcf_config& c = e->cfg;
    const int d = c.hidden, I = c.intermediate, B = n_images, H = c.heads, KV = c.kv_heads, NQ = (H + 2 * KV) * 64;
    OMX_REQUIRE(B >= 1 && B <= 64 && n_img >= 1, "InvalidConfig: omx_vcf_encoder_forward: %d images of %d rows", B, n_img);
    int nq = 0, L = 0;
    if (omx_vcf_encoder_tokens(e, n_img, &nq, &L)) return 1;
    const int64_t R = (int64_t)B * L;
    OMX_REQUIRE(R * std::max(2 * I, NQ) < (1ll << 31) && L <= (1 << 20), "InvalidConfig: omx_vcf_encoder_forward: %d images of %d rows exceed one pass", B, L);

    // ---- every tensor the pass reads, before any launch ----
    tower::Store& st = e->st;
    int err = 0;
    auto W = [&](const std::string& key, size_t want) { return st.find(key, want, true, &err); };
    const float* query = W(n_img == 144 ? "query_768.weight" : "query_1024.weight", (size_t)nq * d);
    const float* fnorm = W("model.model.norm.weight", d);
    struct LW { const float *n1, *ow, *n2, *dw; };
    std::vector<LW> lw(c.layers);
    for (int l = 0; l < c.layers && !err; ++l) {
        const std::string p = "model.model.layers." + std::to_string(l) + ".";
        static const char* part_names[8] = {"self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight", "self_attn.q_proj.bias",
                                            "self_attn.k_proj.bias",   "self_attn.v_proj.bias",   "mlp.gate_proj.weight",    "mlp.up_proj.weight"};
        for (int b = 0; b < 8; ++b)
            if (!(e->layer[l].have & (1 << b))) { err = omx::set_error("WeightNotFound: %s%s%s", st.prefix.c_str(), p.c_str(), part_names[b]); break; }
        lw[l].n1 = W(p + "input_layernorm.weight", d);
        lw[l].ow = W(p + "self_attn.o_proj.weight", (size_t)d * d);
        lw[l].n2 = W(p + "post_attention_layernorm.weight", d);
        lw[l].dw = W(p + "mlp.down_proj.weight", (size_t)d * I);
    }
    if (err) return 1;

    // ---- the RoPE table of this sequence length ----
    float* cs = nullptr;
    {
        auto it = e->rope.find(L);
        if (it == e->rope.end()) {
            std::vector<float> t((size_t)L * 64);
            for (int p = 0; p < L; ++p)
                for (int j = 0; j < 32; ++j) {
                    const double ang = (double)p * pow((double)c.rope_theta, -(double)j / 32.0);
                    t[((size_t)p * 32 + j) * 2] = (float)cos(ang);
                    t[((size_t)p * 32 + j) * 2 + 1] = (float)sin(ang);
                }
            OMX_HIP_CHECK(hipMalloc((void**)&cs, t.size() * sizeof(float)));
            if (hipMemcpy(cs, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(cs); return omx::set_error("omx_vcf_encoder_forward: copy to the device failed"); }
            e->rope[L] = cs;
        } else cs = it->second;
    }

    auto& sc = e->sc;
    if (sc.reserve(V_H, (size_t)R * d, s) || sc.reserve(V_LN, (size_t)R * d, s) || sc.reserve(V_QKV, (size_t)R * NQ, s) || sc.reserve(V_ATT, (size_t)R * d, s) ||
        sc.reserve(V_GU, (size_t)R * 2 * I, s) || sc.reserve(V_ACT, (size_t)R * I, s) || sc.reserve(V_TMP, (size_t)B * nq * d, s) || sc.reserve(V_OUT, (size_t)B * nq * d, s))
        return 1;
    if (c.keep_stages && sc.reserve(V_KEEP, (size_t)c.layers * R * d, s)) return 1;
    float *h = sc.buf[V_H], *ln = sc.buf[V_LN], *qkv = sc.buf[V_QKV], *att = sc.buf[V_ATT], *gu = sc.buf[V_GU], *act = sc.buf[V_ACT], *tmp = sc.buf[V_TMP],
          *out = sc.buf[V_OUT], *keep = sc.buf[V_KEEP];
    e->rows = (size_t)R;

    int launches = 0;
    vcf_assemble_kernel<<<grid_for(R * d), 256, 0, s>>>(h, x, query, B, n_img, nq, d);
    OMX_LAUNCH_CHECK();
    launches += 1;
    for (int l = 0; l < c.layers; ++l) {
        const VcfLayer& Lw = e->layer[l];
        if (omx_rms_norm(ln, h, lw[l].n1, R, d, c.eps, OMX_FLOAT32, s)) return 1;
        if (tower::gemm({ln, Lw.qkv_w, Lw.qkv_b, nullptr, qkv, (int)R, NQ, d, 0, 0, 0}, s)) return 1;
        vcf_rope_kernel<<<grid_for(R * (H + KV) * 32), 256, 0, s>>>(qkv, NQ, R, L, H + KV, cs);
        OMX_LAUNCH_CHECK();
        if (prefix_attention(att, d, qkv, NQ, B, L, H, KV, n_img, s)) return 1;
        if (tower::gemm({att, lw[l].ow, nullptr, h, h, (int)R, d, d, 0, 0, 0}, s)) return 1;
        if (omx_rms_norm(ln, h, lw[l].n2, R, d, c.eps, OMX_FLOAT32, s)) return 1;
        if (tower::gemm({ln, Lw.gu_w, nullptr, nullptr, gu, (int)R, 2 * I, d, 0, 0, 0}, s)) return 1;
        vcf_swiglu_kernel<<<grid_for(R * I), 256, 0, s>>>(act, gu, R, I);
        OMX_LAUNCH_CHECK();
        if (tower::gemm({act, lw[l].dw, nullptr, h, h, (int)R, d, I, 0, 0, 0}, s)) return 1;
        launches += 9;
        if (keep) OMX_HIP_CHECK(hipMemcpyAsync(keep + (size_t)l * R * d, h, (size_t)R * d * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    vcf_query_rows_kernel<<<grid_for((int64_t)B * nq * d), 256, 0, s>>>(tmp, h, B, n_img, nq, d);
    OMX_LAUNCH_CHECK();
    if (omx_rms_norm(out, tmp, fnorm, (int64_t)B * nq, d, c.eps, OMX_FLOAT32, s)) return 1;
    launches += 2;
    OMX_HIP_CHECK(hipMemcpyAsync(out_rows, out, (size_t)B * nq * d * sizeof(float), hipMemcpyDeviceToDevice, s));
    e->launches = launches;
    return 0;
}

int omx_vcf_encoder_debug_read(omx_vcf_encoder e, const char* name, float* host, size_t n_elems) {
    OMX_REQUIRE(e && name && host, "omx_vcf_encoder_debug_read: null argument");
    const std::string s(name);
    const float* src = nullptr;
    size_t have = 0;
    if (s == "out") { src = e->sc.buf[V_OUT]; have = e->sc.cap[V_OUT]; }
    else if (s.rfind("layer", 0) == 0) {
        OMX_REQUIRE(e->cfg.keep_stages, "omx_vcf_encoder_debug_read: %s is kept only by an encoder created with keep_stages", name);
        const std::string t = s.substr(5);
        OMX_REQUIRE(!t.empty() && t.size() <= 4 && t.find_first_not_of("0123456789") == std::string::npos && atoi(t.c_str()) < e->cfg.layers,
                    "omx_vcf_encoder_debug_read: unknown stage %s", name);
        const size_t slot = e->rows * (size_t)e->cfg.hidden, idx = (size_t)atoi(t.c_str());
        OMX_REQUIRE(e->sc.buf[V_KEEP] && (idx + 1) * slot <= e->sc.cap[V_KEEP], "omx_vcf_encoder_debug_read: no forward has run");
        src = e->sc.buf[V_KEEP] + idx * slot; have = slot;
    } else return omx::set_error("omx_vcf_encoder_debug_read: unknown stage %s", name);
    OMX_REQUIRE(src && n_elems <= have, "omx_vcf_encoder_debug_read: %zu elements of %s, the buffer holds %zu", n_elems, name, have);
    OMX_HIP_CHECK(hipDeviceSynchronize());
    OMX_HIP_CHECK(hipMemcpy(host, src, n_elems * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

int omx_prefix_causal_attention_f32(float* out, int64_t ldo, const float* qkv, int64_t ld, int images, int n_rows, int heads, int kv_heads, int width,
                                    int n_prefix, omx_stream stream) {
    OMX_REQUIRE(width == 64, "InvalidConfig: prefix-causal attention: head width %d: the kernel is built for 64", width);
    return prefix_attention(out, ldo, qkv, ld, images, n_rows, heads, kv_heads, n_prefix, (hipStream_t)stream);
}

}  // extern "C"
