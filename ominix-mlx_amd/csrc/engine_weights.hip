// Checkpoint tensors of the Qwen3 engine (engine.hip): registered by name (omx_qwen3_set_weight) or synthesised on the device, sized
// against the config, and resolved into the per-layer tables the passes read.
#include "engine_model.hpp"

static uint32_t crc32_str(const char* s) {
    uint32_t crc = 0xFFFFFFFFu;
    for (; *s; ++s) {
        crc ^= (uint8_t)*s;
        for (int k = 0; k < 8; ++k) crc = (crc >> 1) ^ (0xEDB88320u & (0u - (crc & 1u)));
    }
    return ~crc;
}

namespace omx {

std::pair<int, int> quant_format_of(omx_qwen3 m, const std::string& prefix) {
    auto it = m->quant_formats.find(prefix);
    return it != m->quant_formats.end() ? it->second : std::make_pair(m->cfg.quant_bits, m->cfg.quant_group);
}

// The packed Linear / embedding the forward reads at module path `prefix` of a dense model: its contraction width K, or 0 for a path
// that names none (layer index out of range, a norm, an lm_head the tied model does not have)
static int packed_module_k(omx_qwen3 m, const std::string& prefix) {
    const EngineConfig& c = m->cfg;
    if (prefix == "model.embed_tokens") return c.hidden_size;
    if (prefix == "lm_head") return c.tie_word_embeddings ? 0 : c.hidden_size;
    if (prefix.compare(0, 13, "model.layers.") != 0) return 0;
    const size_t dot = prefix.find('.', 13);
    if (dot == std::string::npos || dot == 13) return 0;
    const std::string idx = prefix.substr(13, dot - 13);
    if (idx.find_first_not_of("0123456789") != std::string::npos || idx.size() > 6 || atoi(idx.c_str()) >= c.num_hidden_layers) return 0;
    const std::string sub = prefix.substr(dot + 1);
    if (sub == "self_attn.q_proj" || sub == "self_attn.k_proj" || sub == "self_attn.v_proj" || sub == "mlp.gate_proj" || sub == "mlp.up_proj") return c.hidden_size;
    if (sub == "self_attn.o_proj") return m->H * c.head_dim;
    if (sub == "mlp.down_proj") return m->I;
    return 0;
}

int resolve_weights(omx_qwen3 m) {
    if (m->weights_resolved) return 0;
    if (!m->dq_cache.empty()) {   // the weights changed under the dequantised copies of the prompt pass
        (void)hipStreamSynchronize(m->stream);
        m->dq_cache.clear();          // (the slab stays: the same shapes come back)
        m->dq_cache_bytes = 0;
    }
    const EngineConfig& c = m->cfg;
    const bool quant = c.quant_bits != 0;
    const int D = c.head_dim, hd = c.hidden_size;
    auto get = [&](const std::string& n, const bf16_t** out) -> int {
        auto it = m->named.find(n);
        if (it == m->named.end()) return set_error("WeightNotFound: %s", n.c_str());   // error.rs:6-32
        *out = (const bf16_t*)it->second;
        return 0;
    };
    const bool interleave = quant && !env_off("OMX_QUANT_INTERLEAVE");
    // a packed Linear's (weight, scales, biases) triplet -- K: contraction width; stack: matrices stacked in the tensor (experts)
    auto getq = [&](const std::string& prefix, int n, QMat* out, int K = 0, int stack = 1) -> int {
        const bf16_t *w = nullptr, *sc = nullptr, *bi = nullptr;
        if (get(prefix + ".weight", &w) || get(prefix + ".scales", &sc) || get(prefix + ".biases", &bi)) return 1;
        *out = QMat{(const uint32_t*)w, sc, bi, n};
        const std::pair<int, int> fmt = quant_format_of(m, prefix);   // the matrix's own format travels with it
        out->bits = fmt.first; out->group = fmt.second;
        if (interleave && K > 0 && K % 2048 == 0) {   // (scale, bias) words for the packed-weight GEMV (quant.hpp)
            const size_t ng = (size_t)stack * n * (K / fmt.second);
            uint32_t* sb = nullptr;
            if (dev_alloc(m, &sb, ng) || launch_quant_interleave(sb, sc, bi, ng, m->stream)) return 1;
            out->sb = sb;
            quant_register_sb(sc, sb);
            m->sb_keys.push_back(sc);
        }
        // the dense decode step's matrices once more as matrix-core tiles (qgemv_mfma.hip; OMX_QGEMV_MFMA=0: the VALU kernel only)
        const bool tiles_off = env_off("OMX_QGEMV_MFMA");        // (read per model: tests compare the two kernels in one process)
        if (!tiles_off && stack == 1 && K > 0 && !c.quant_scales_f16 && qgemv4m_shape_ok(K, fmt.second, fmt.first)) {
            uint32_t* tiles = nullptr;
            if (dev_alloc(m, &tiles, qgemv4m_tile_words(n, K)) || launch_qgemv4m_repack(tiles, (const uint32_t*)w, sc, bi, n, K, m->stream)) return 1;
            out->tiles = tiles;
        }
        return 0;
    };
    // one Linear of the checkpoint by its name: the bf16 matrix (quant_bits 0, float16 alike) or the packed triplet
    auto lin = [&](const std::string& prefix, int n, const bf16_t** dense, QMat* packed, int K, int stack = 1) -> int {
        return quant ? getq(prefix, n, packed, K, stack) : get(prefix + ".weight", dense);
    };
    m->layers.resize(c.num_hidden_layers);
    if (quant) m->qlayers.resize(c.num_hidden_layers);
    LayerQ no_q = {};
    for (int i = 0; i < c.num_hidden_layers; ++i) {
        const std::string p = "model.layers." + std::to_string(i) + ".";
        LayerW& L = m->layers[i];
        LayerQ& Q = quant ? m->qlayers[i] : no_q;
        L = LayerW{};
        if (lin(p + "self_attn.q_proj", m->H * D, &L.q, &Q.q, hd) || lin(p + "self_attn.k_proj", m->Hkv * D, &L.k, &Q.k, hd) ||
            lin(p + "self_attn.v_proj", m->Hkv * D, &L.v, &Q.v, hd) || lin(p + "self_attn.o_proj", hd, &L.o, &Q.o, m->H * D) ||
            get(p + "input_layernorm.weight", &L.in_ln) || get(p + "post_attention_layernorm.weight", &L.post_ln))
            return 1;
        if (!c.no_qk_norm && (get(p + "self_attn.q_norm.weight", &L.q_norm) || get(p + "self_attn.k_norm.weight", &L.k_norm))) return 1;
        if (c.attention_bias) {   // qwen2.rs:112-124: Linear with bias for q/k/v only (bf16 checkpoints: omx_qwen3_create)
            if (get(p + "self_attn.q_proj.bias", &L.q_bias) || get(p + "self_attn.k_proj.bias", &L.k_bias) || get(p + "self_attn.v_proj.bias", &L.v_bias)) return 1;
            const size_t nq = (size_t)m->H * D, nk = (size_t)m->Hkv * D;
            bf16_t* cat = nullptr;
            if (dev_alloc(m, &cat, nq + 2 * nk)) return 1;
            OMX_HIP_CHECK(hipMemcpyAsync(cat, L.q_bias, nq * 2, hipMemcpyDeviceToDevice, m->stream));
            OMX_HIP_CHECK(hipMemcpyAsync(cat + nq, L.k_bias, nk * 2, hipMemcpyDeviceToDevice, m->stream));
            OMX_HIP_CHECK(hipMemcpyAsync(cat + nq + nk, L.v_bias, nk * 2, hipMemcpyDeviceToDevice, m->stream));
            L.qkv_bias = cat;
        }
        if (layer_is_moe(c, i)) {
            const std::string mp = p + (c.moe_mode == 0 ? "block_sparse_moe." : "mlp.");
            // (expert tensor parallel: this rank's columns of every expert; expert parallel: this rank's experts)
            const int Im = c.tp_size > 1 ? m->moe_I : c.moe_intermediate_size;
            const int E = c.num_experts, El = c.ep_size > 1 ? E / c.ep_size : E;
            if (lin(mp + "gate", E, &L.moe_gate, &Q.moe_router, hd) || lin(mp + "switch_mlp.gate_proj", Im, &L.moe_wg, &Q.moe_g, hd, El) ||
                lin(mp + "switch_mlp.up_proj", Im, &L.moe_wu, &Q.moe_u, hd, El) || lin(mp + "switch_mlp.down_proj", hd, &L.moe_wd, &Q.moe_d, Im, El))
                return 1;
            if (c.moe_mode == 2 && c.n_shared_experts > 0) {
                if (get(mp + "shared_experts.gate_proj.weight", &L.sh_gate) || get(mp + "shared_experts.up_proj.weight", &L.sh_up) ||
                    get(mp + "shared_experts.down_proj.weight", &L.sh_down))
                    return 1;
                // the decode form streams the shared MLP as n_shared pseudo-experts BEHIND the routed ones, through the same two
                // expert-selected launches: stacks of E + n_shared matrices, the tail being the shared gate / up row blocks and the
                // shared down projection's column blocks (moe.hip).  OMX_MOE_SHARED_SLOTS=0: the checkpoint's stacks as they are.
                if (!env_off("OMX_MOE_SHARED_SLOTS")) {
                    const size_t ns = c.n_shared_experts, per = (size_t)Im * hd, routed = (size_t)E * per;
                    bf16_t *wg = nullptr, *wu = nullptr, *wd = nullptr;
                    if (dev_alloc(m, &wg, routed + ns * per) || dev_alloc(m, &wu, routed + ns * per) || dev_alloc(m, &wd, routed + ns * per)) return 1;
                    OMX_HIP_CHECK(hipMemcpyAsync(wg, L.moe_wg, routed * 2, hipMemcpyDeviceToDevice, m->stream));
                    OMX_HIP_CHECK(hipMemcpyAsync(wu, L.moe_wu, routed * 2, hipMemcpyDeviceToDevice, m->stream));
                    OMX_HIP_CHECK(hipMemcpyAsync(wd, L.moe_wd, routed * 2, hipMemcpyDeviceToDevice, m->stream));
                    OMX_HIP_CHECK(hipMemcpyAsync(wg + routed, L.sh_gate, ns * per * 2, hipMemcpyDeviceToDevice, m->stream));
                    OMX_HIP_CHECK(hipMemcpyAsync(wu + routed, L.sh_up, ns * per * 2, hipMemcpyDeviceToDevice, m->stream));
                    for (size_t j = 0; j < ns; ++j)      // pseudo-expert j of down: columns [j Im, (j + 1) Im) of [hidden, ns Im]
                        OMX_HIP_CHECK(hipMemcpy2DAsync(wd + routed + j * per, (size_t)Im * 2, L.sh_down + j * Im, ns * Im * 2, (size_t)Im * 2, hd,
                                                       hipMemcpyDeviceToDevice, m->stream));
                    L.moe_wg = wg; L.moe_wu = wu; L.moe_wd = wd; L.moe_tail = (int)ns;
                }
            }
        } else if (lin(p + "mlp.gate_proj", m->I, &L.gate, &Q.gate, hd) || lin(p + "mlp.up_proj", m->I, &L.up, &Q.up, hd) ||
                   lin(p + "mlp.down_proj", hd, &L.down, &Q.down, m->I)) {
            return 1;
        }
        // the SwiGLU launch computes a (gate, up) row pair in one wave: one format for the two
        OMX_REQUIRE(!quant || c.num_experts > 0 || (Q.gate.bits == Q.up.bits && Q.gate.group == Q.up.group),
                    "InvalidConfig: layer %d: mlp.gate_proj (%d-bit group %d) and mlp.up_proj (%d-bit group %d) must share a quantization format",
                    i, Q.gate.bits, Q.gate.group, Q.up.bits, Q.up.group);
    }
    if (lin("model.embed_tokens", c.vocab_size, &m->embed, &m->q_embed, 0) || get("model.norm.weight", &m->final_norm)) return 1;
    if (quant) {
        if (c.tie_word_embeddings && c.tp_size <= 1) m->q_head = m->q_embed;   // QuantizedEmbedding::as_linear (quantized.rs:166-180)
        else if (getq("lm_head", m->V, &m->q_head, hd)) return 1;              // (tied under TP: the caller registers the table's vocabulary shard as lm_head.*)
        m->weights_resolved = true;
        return 0;
    }
    if (c.tie_word_embeddings) {
        // tied head = Embedding::as_linear (model.rs:485-488); under TP the caller registers the vocab shard
        auto it = m->named.find("lm_head.weight");
        m->lm_head = it != m->named.end() ? (const bf16_t*)it->second : m->embed;
        OMX_REQUIRE(c.tp_size == 1 || it != m->named.end(), "tied lm_head under TP needs a vocab shard registered as lm_head.weight");
    } else if (get("lm_head.weight", &m->lm_head)) {
        return 1;
    }
    if (m->cfg.num_experts == 0) {   // layer table of the persistent step (step_engine.hip; it stands down for any model with experts)
        m->se_layers_host.resize(m->cfg.num_hidden_layers);
        for (int i = 0; i < m->cfg.num_hidden_layers; ++i) {
            const LayerW& L = m->layers[i];
            m->se_layers_host[i] = StepEngineLayer{L.q, L.k, L.v, L.o, L.gate, L.up, L.down, L.in_ln, L.post_ln, L.q_norm, L.k_norm,
                                                   m->kcache[i], m->vcache[i]};
        }
        if (!m->se_layers && dev_alloc(m, &m->se_layers, m->se_layers_host.size())) return 1;
        OMX_HIP_CHECK(hipMemcpyAsync(m->se_layers, m->se_layers_host.data(), m->se_layers_host.size() * sizeof(StepEngineLayer),
                                     hipMemcpyHostToDevice, m->stream));
    }
    m->weights_resolved = true;
    return 0;
}

}  // namespace omx

// bytes the forward will read behind checkpoint tensor `name` on THIS rank (after the TP / EP slicing), 0 for a name it does not
// use; mirrors resolve_weights above (and engine.py expected_shape, which reports the same thing as a shape)
static size_t expected_weight_bytes(omx_qwen3 m, const std::string& name) {
    const EngineConfig& c = m->cfg;
    const size_t hd = c.hidden_size, D = c.head_dim, H = m->H, Hkv = m->Hkv, I = m->I, Im = c.tp_size > 1 && c.num_experts > 0 ? m->moe_I : c.moe_intermediate_size;   // (expert tensor parallel: this rank's columns)
    const size_t E = c.num_experts, El = c.ep_size > 1 ? E / c.ep_size : E;
    static const char* kSuffix[] = {".weight", ".scales", ".biases", ".bias"};
    int kind = -1;
    std::string stem;
    for (int i = 0; i < 4; ++i) {
        const size_t n = strlen(kSuffix[i]);
        if (name.size() > n && name.compare(name.size() - n, n, kSuffix[i]) == 0) { kind = i; stem = name.substr(0, name.size() - n); break; }
    }
    if (kind < 0) return 0;
    const bool quant = c.quant_bits != 0;
    // [n, k] Linear (x stack): dense bf16, or the packed triplet of a quantized checkpoint; bias [n]
    const std::pair<int, int> fmt = quant_format_of(m, stem);   // the matrix's own format
    auto lin = [&](size_t n, size_t k, size_t stack = 1) -> size_t {
        if (kind == 3) return n * 2;
        if (!quant) return kind == 0 ? stack * n * k * 2 : 0;
        if (kind == 0) return stack * n * (k * fmt.first / 32) * 4;
        return stack * n * (k / fmt.second) * 2;
    };
    auto vec = [&](size_t n) -> size_t { return kind == 0 ? n * 2 : 0; };
    if (stem == "model.embed_tokens") return lin(c.vocab_size, hd);
    if (stem == "lm_head") return lin(m->V, hd);
    if (stem == "model.norm") return vec(hd);
    if (stem.compare(0, 13, "model.layers.") != 0) return 0;
    const size_t dot = stem.find('.', 13);
    if (dot == std::string::npos) return 0;
    const std::string sub = stem.substr(dot + 1);
    const bool ds = E > 0 && c.moe_mode == 2;
    const int layer = atoi(stem.c_str() + 13);
    if (ds) {   // the per-layer plan: a name the layer does not read has no expected size
        const bool dense_name = sub == "mlp.gate_proj" || sub == "mlp.up_proj" || sub == "mlp.down_proj";
        const bool moe_name = sub == "mlp.gate" || sub.compare(0, 15, "mlp.switch_mlp.") == 0 || sub.compare(0, 19, "mlp.shared_experts.") == 0;
        if ((dense_name && layer_is_moe(c, layer)) || (moe_name && !layer_is_moe(c, layer))) return 0;
        const size_t Ws = (size_t)c.n_shared_experts * Im;
        if (Ws > 0 && (sub == "mlp.shared_experts.gate_proj" || sub == "mlp.shared_experts.up_proj")) return lin(Ws, hd);
        if (Ws > 0 && sub == "mlp.shared_experts.down_proj") return lin(hd, Ws);
    }
    if (sub == "self_attn.q_proj") return lin(H * D, hd);
    if (sub == "self_attn.k_proj" || sub == "self_attn.v_proj") return lin(Hkv * D, hd);
    if (sub == "self_attn.o_proj") return lin(hd, H * D);
    if (sub == "mlp.gate_proj" || sub == "mlp.up_proj") return lin(I, hd);
    if (sub == "mlp.down_proj") return lin(hd, I);
    if (sub == "input_layernorm" || sub == "post_attention_layernorm") return vec(hd);
    if (sub == "self_attn.q_norm" || sub == "self_attn.k_norm") return vec(D);
    if (E > 0)
        for (const char* mp : {"block_sparse_moe.", "mlp."}) {
            const std::string p = mp;
            if (sub == p + "gate") return lin(E, hd);
            if (sub == p + "switch_mlp.gate_proj" || sub == p + "switch_mlp.up_proj") return lin(Im, hd, El);
            if (sub == p + "switch_mlp.down_proj") return lin(hd, Im, El);
        }
    return 0;
}

extern "C" {

int omx_qwen3_set_weight(omx_qwen3 m, const char* name, const void* ptr, size_t nbytes) {
    OMX_REQUIRE(m && name && ptr, "omx_qwen3_set_weight: null argument");
    // the engine reads raw device pointers: a tensor shorter than the config implies would be read past its end, so the size is part
    // of the call (the reference raises a shape error on load)
    const size_t want = expected_weight_bytes(m, name);
    OMX_REQUIRE(want == 0 || nbytes == want, "ShapeMismatch: %s holds %zu bytes, the config expects %zu", name, nbytes, want);
    OMX_REQUIRE(((uintptr_t)ptr & 15u) == 0, "omx_qwen3_set_weight: %s is not 16-byte aligned", name);
    OMX_REQUIRE(m->g_full == nullptr, "omx_qwen3_set_weight: weights are frozen once the decode step is built");
    m->named[name] = ptr;
    m->weights_resolved = false;
    return 0;
}

// The MLX format of ONE packed matrix (a mixed-precision checkpoint: config.json "quantization" carries an entry per module path next to
// the global bits / group_size).  Legal until a tensor of that prefix is registered or synthesised: its byte counts, repacks and tiles
// follow the format.
int omx_qwen3_set_quant_format(omx_qwen3 m, const char* prefix, int bits, int group_size) {
    OMX_REQUIRE(m && prefix, "omx_qwen3_set_quant_format: null argument");
    const EngineConfig& c = m->cfg;
    OMX_REQUIRE(c.quant_bits != 0, "omx_qwen3_set_quant_format: %s: the model has no base quantization (a bf16 / float16 checkpoint)", prefix);
    OMX_REQUIRE(c.num_experts == 0, "omx_qwen3_set_quant_format: %s: per-matrix formats with experts (num_experts %d) are not supported", prefix, c.num_experts);
    OMX_REQUIRE(c.tp_size <= 1 && c.ep_size <= 1, "omx_qwen3_set_quant_format: %s: per-matrix formats under tensor / expert parallelism (tp_size %d, ep_size %d) are not supported",
                prefix, c.tp_size, c.ep_size);
    OMX_REQUIRE(!c.quant_scales_f16, "omx_qwen3_set_quant_format: %s: per-matrix formats with float16 triplets (scales_dtype float16) are not supported", prefix);
    OMX_REQUIRE(!c.attention_bias, "omx_qwen3_set_quant_format: %s: per-matrix formats with attention_bias are not supported", prefix);
    const int K = packed_module_k(m, prefix);
    OMX_REQUIRE(K > 0, "omx_qwen3_set_quant_format: unknown prefix %s (a packed module of this model: model.embed_tokens, lm_head of an untied model, "
                "model.layers.<i>.self_attn.{q,k,v,o}_proj, model.layers.<i>.mlp.{gate,up,down}_proj)", prefix);
    OMX_REQUIRE(quant_bits_ok(bits), "omx_qwen3_set_quant_format: %s: bits must be 2, 3, 4, 5, 6 or 8 (got %d)", prefix, bits);
    OMX_REQUIRE(group_size == 32 || group_size == 64 || group_size == 128, "omx_qwen3_set_quant_format: %s: group_size must be 32, 64 or 128 (got %d)", prefix, group_size);
    OMX_REQUIRE(K % group_size == 0, "omx_qwen3_set_quant_format: %s: the contraction width (%d) must be divisible by the group size (%d)", prefix, K, group_size);
    const std::string p = prefix;
    for (const char* leaf : {".weight", ".scales", ".biases"})
        OMX_REQUIRE(m->named.find(p + leaf) == m->named.end(), "omx_qwen3_set_quant_format: %s%s is already set: a matrix's format is fixed before its tensors arrive", prefix, leaf);
    OMX_REQUIRE(m->g_full == nullptr, "omx_qwen3_set_quant_format: weights are frozen once the decode step is built");
    m->quant_formats[p] = std::make_pair(bits, group_size);
    m->weights_resolved = false;
    return 0;
}

// ... and the format a matrix has: its own, or the base format where nothing was set
int omx_qwen3_quant_format(omx_qwen3 m, const char* prefix, int* bits, int* group_size) {
    OMX_REQUIRE(m && prefix && bits && group_size, "omx_qwen3_quant_format: null argument");
    OMX_REQUIRE(m->cfg.quant_bits != 0, "omx_qwen3_quant_format: %s: the model has no base quantization", prefix);
    OMX_REQUIRE(m->cfg.num_experts > 0 || packed_module_k(m, prefix) > 0, "omx_qwen3_quant_format: unknown prefix %s", prefix);
    const std::pair<int, int> fmt = quant_format_of(m, prefix);
    *bits = fmt.first; *group_size = fmt.second;
    return 0;
}

// device pointer of a registered (or synthesised) tensor by its checkpoint name: what a caller that ALSO drives the per-op mlx-c route on the
// same weights needs (omx_mlx_array_from_device wraps it; bench: per_op_route.hip)
int omx_qwen3_get_weight(omx_qwen3 m, const char* name, const void** ptr, size_t* nbytes) {
    OMX_REQUIRE(m && name && ptr, "omx_qwen3_get_weight: null argument");
    auto it = m->named.find(name);
    if (it == m->named.end()) return set_error("WeightNotFound: %s", name);
    *ptr = it->second;
    if (nbytes) *nbytes = expected_weight_bytes(m, name);
    return 0;
}

}  // extern "C"

static int synth_weights_impl(omx_qwen3 m, uint32_t base_seed, bool peaked) {
    OMX_REQUIRE(m, "omx_qwen3_synth_weights: null model");
    OMX_REQUIRE(!peaked || (m->cfg.quant_bits == 0 && !m->cfg.float16_weights && !m->cfg.tie_word_embeddings),
                "omx_qwen3_synth_weights_peaked: bf16 checkpoints with an untied lm_head only");
    OMX_REQUIRE(!m->cfg.quant_scales_f16, "omx_qwen3_synth_weights: the device generator quantises in bf16; a float16-scale model takes uploaded triplets");
    const EngineConfig& c = m->cfg;
    const int D = c.head_dim, hd = c.hidden_size, r = c.tp_rank;
    const float amp_w = (float)(0.02 * sqrt(3.0)), amp_n = (float)(0.01 * sqrt(3.0));   // == oracle/synth.py
    // logical tensor [rows_full, cols_full]; this rank holds rows [row0, row0+rows) x cols [col0, col0+cols)
    auto make = [&](const std::string& name, int64_t rows, int64_t cols, int64_t ld_full, int64_t row0, int64_t col0,
                    bool is_norm) -> int {
        bf16_t* p = nullptr;
        if (dev_alloc(m, &p, (size_t)rows * cols)) return 1;
        const uint32_t seed = base_seed ^ crc32_str(name.c_str());
        // (a dense float16 model: the same generator values rounded to float16 -- oracle/synth.py tensor(dt="f16"))
        if (omx_fill_uniform_2d(p, rows, cols, ld_full, row0, col0, seed, is_norm ? amp_n : amp_w, is_norm ? 1.0f : 0.0f,
                                c.float16_weights ? OMX_FLOAT16 : OMX_BFLOAT16, m->stream))
            return 1;
        m->named[name] = p;
        return 0;
    };
    const int Hq = m->H * D, Hk = m->Hkv * D;
    // first k / v row of this rank in the logical projection: its own KV heads, or the one head it shares with its neighbours
    const int kv_rep = c.num_key_value_heads >= c.tp_size ? 1 : c.tp_size / c.num_key_value_heads;
    const int64_t kv_row0 = (int64_t)(r / kv_rep) * Hk;
    if (c.quant_bits) {
        // the quantized model IS mlx quantize() of the synthetic bf16 model: generate each logical matrix into a scratch
        // buffer with the bf16 generator, quantise it on the device, keep only the (weight, scales, biases) triplet
        bf16_t* scratch = nullptr;
        size_t biggest = (size_t)std::max((int64_t)c.vocab_size, (int64_t)std::max(m->I, Hq)) * (size_t)std::max(hd, m->I);
        if (c.num_experts > 0) biggest = std::max(biggest, (size_t)c.num_experts * c.moe_intermediate_size * (size_t)hd);   // a whole expert stack
        OMX_HIP_CHECK(hipMalloc((void**)&scratch, biggest * 2));
        // (ld_full, row0, col0): this rank's window of the logical matrix -- quantisation is per group of one row, so the window's
        // triplet IS the slice of the whole matrix's triplet (K slices hold whole groups); seed_of: the logical tensor the values belong to
        auto makeq = [&](const std::string& prefix, int64_t rows, int64_t cols, int64_t ld_full = 0, int64_t row0 = 0, int64_t col0 = 0,
                         const char* seed_of = nullptr) -> int {
            const uint32_t seed = base_seed ^ crc32_str(seed_of ? seed_of : (prefix + ".weight").c_str());
            if (omx_fill_uniform_2d(scratch, rows, cols, ld_full ? ld_full : cols, row0, col0, seed, amp_w, 0.0f, OMX_BFLOAT16, m->stream)) return 1;
            uint32_t* pk = nullptr;
            bf16_t *sc = nullptr, *bi = nullptr;
            const std::pair<int, int> fmt = quant_format_of(m, prefix);   // quantised in the matrix's own format
            if (dev_alloc(m, &pk, (size_t)(rows * cols * fmt.first / 32)) || dev_alloc(m, &sc, (size_t)(rows * cols / fmt.second)) ||
                dev_alloc(m, &bi, (size_t)(rows * cols / fmt.second)))
                return 1;
            if (omx_quantize(pk, sc, bi, scratch, rows, (int)cols, fmt.second, fmt.first, OMX_BFLOAT16, m->stream)) return 1;
            m->named[prefix + ".weight"] = pk;
            m->named[prefix + ".scales"] = sc;
            m->named[prefix + ".biases"] = bi;
            return 0;
        };
        int rc = 0;
        for (int i = 0; i < c.num_hidden_layers && !rc; ++i) {
            const std::string p = "model.layers." + std::to_string(i) + ".";
            rc = makeq(p + "self_attn.q_proj", Hq, hd, hd, (int64_t)r * Hq) || makeq(p + "self_attn.k_proj", Hk, hd, hd, kv_row0) ||
                 makeq(p + "self_attn.v_proj", Hk, hd, hd, kv_row0) ||
                 makeq(p + "self_attn.o_proj", hd, Hq, (int64_t)c.num_attention_heads * D, 0, (int64_t)r * Hq) || make(p + "input_layernorm.weight", 1, hd, hd, 0, 0, true) ||
                 make(p + "post_attention_layernorm.weight", 1, hd, hd, 0, 0, true);
            if (!rc && !c.no_qk_norm) rc = make(p + "self_attn.q_norm.weight", 1, D, D, 0, 0, true) || make(p + "self_attn.k_norm.weight", 1, D, D, 0, 0, true);
            if (!rc && c.num_experts > 0) {
                const std::string mp = p + (c.moe_mode == 0 ? "block_sparse_moe." : "mlp.");
                const int64_t E = c.num_experts, Im = c.moe_intermediate_size;
                if (c.tp_size > 1) {
                    // expert tensor parallel: rows [r I_l, + I_l) of every expert's gate / up (E strided windows of the logical stack, gathered
                    // into the scratch before ONE quantise call), the same columns -- whole groups -- of its down projection
                    const int64_t Il = m->moe_I;
                    auto makeq_rows = [&](const std::string& prefix) -> int {
                        const uint32_t seed = base_seed ^ crc32_str((prefix + ".weight").c_str());
                        for (int64_t e = 0; e < E; ++e)
                            if (omx_fill_uniform_2d(scratch + e * Il * hd, Il, hd, hd, e * Im + (int64_t)r * Il, 0, seed, amp_w, 0.0f, OMX_BFLOAT16, m->stream)) return 1;
                        uint32_t* pk = nullptr;
                        bf16_t *sc = nullptr, *bi = nullptr;
                        const int64_t rows = E * Il;
                        const std::pair<int, int> fmt = quant_format_of(m, prefix);
                        if (dev_alloc(m, &pk, (size_t)(rows * hd * fmt.first / 32)) || dev_alloc(m, &sc, (size_t)(rows * hd / fmt.second)) ||
                            dev_alloc(m, &bi, (size_t)(rows * hd / fmt.second)))
                            return 1;
                        if (omx_quantize(pk, sc, bi, scratch, rows, hd, fmt.second, fmt.first, OMX_BFLOAT16, m->stream)) return 1;
                        m->named[prefix + ".weight"] = pk; m->named[prefix + ".scales"] = sc; m->named[prefix + ".biases"] = bi;
                        return 0;
                    };
                    rc = makeq(mp + "gate", E, hd) || makeq_rows(mp + "switch_mlp.gate_proj") || makeq_rows(mp + "switch_mlp.up_proj") ||
                         makeq(mp + "switch_mlp.down_proj", E * hd, Il, Im, 0, (int64_t)r * Il);
                } else {
                    const int64_t El = c.ep_size > 1 ? E / c.ep_size : E, e0 = c.ep_size > 1 ? c.ep_rank * El : 0;   // this rank's experts
                    rc = makeq(mp + "gate", E, hd) || makeq(mp + "switch_mlp.gate_proj", El * Im, hd, hd, e0 * Im) ||
                         makeq(mp + "switch_mlp.up_proj", El * Im, hd, hd, e0 * Im) || makeq(mp + "switch_mlp.down_proj", El * hd, Im, Im, e0 * hd);
                }
            } else if (!rc) {
                rc = makeq(p + "mlp.gate_proj", m->I, hd, hd, (int64_t)r * m->I) || makeq(p + "mlp.up_proj", m->I, hd, hd, (int64_t)r * m->I) ||
                     makeq(p + "mlp.down_proj", hd, m->I, c.intermediate_size, 0, (int64_t)r * m->I);
            }
        }
        rc = rc || makeq("model.embed_tokens", c.vocab_size, hd) || make("model.norm.weight", 1, hd, hd, 0, 0, true);
        if (!rc && !c.tie_word_embeddings) rc = makeq("lm_head", m->V, hd, hd, (int64_t)r * m->V);
        else if (!rc && c.tp_size > 1) rc = makeq("lm_head", m->V, hd, hd, (int64_t)r * m->V, 0, "model.embed_tokens.weight");   // tied: the table's shard
        (void)hipStreamSynchronize(m->stream);
        (void)hipFree(scratch);
        m->weights_resolved = false;
        return rc;
    }
    for (int i = 0; i < c.num_hidden_layers; ++i) {
        const std::string p = "model.layers." + std::to_string(i) + ".";
        if (make(p + "self_attn.q_proj.weight", Hq, hd, hd, (int64_t)r * Hq, 0, false) ||
            make(p + "self_attn.k_proj.weight", Hk, hd, hd, kv_row0, 0, false) ||
            make(p + "self_attn.v_proj.weight", Hk, hd, hd, kv_row0, 0, false) ||
            make(p + "self_attn.o_proj.weight", hd, Hq, (int64_t)c.num_attention_heads * D, 0, (int64_t)r * Hq, false) ||
            make(p + "input_layernorm.weight", 1, hd, hd, 0, 0, true) ||
            make(p + "post_attention_layernorm.weight", 1, hd, hd, 0, 0, true))
            return 1;
        if (!c.no_qk_norm && (make(p + "self_attn.q_norm.weight", 1, D, D, 0, 0, true) || make(p + "self_attn.k_norm.weight", 1, D, D, 0, 0, true)))
            return 1;
        // biases: this rank's columns of the logical [1, H_total * D] vector -- the same offsets as the rows of its projection
        const int64_t Hq_all = (int64_t)c.num_attention_heads * D, Hk_all = (int64_t)c.num_key_value_heads * D;
        if (c.attention_bias && (make(p + "self_attn.q_proj.bias", 1, Hq, Hq_all, 0, (int64_t)r * Hq, false) ||
                                 make(p + "self_attn.k_proj.bias", 1, Hk, Hk_all, 0, kv_row0, false) ||
                                 make(p + "self_attn.v_proj.bias", 1, Hk, Hk_all, 0, kv_row0, false)))
            return 1;
        if (layer_is_moe(c, i)) {
            const std::string mp = p + (c.moe_mode == 0 ? "block_sparse_moe." : "mlp.");
            const int64_t E = c.num_experts, Im = c.moe_intermediate_size;
            const int64_t El = c.ep_size > 1 ? E / c.ep_size : E, e0 = c.ep_size > 1 ? c.ep_rank * El : 0;   // this rank's experts
            const int64_t Ws = c.moe_mode == 2 ? (int64_t)c.n_shared_experts * Im : 0;                        // the shared MLP (mode 2)
            if (Ws > 0 && (make(mp + "shared_experts.gate_proj.weight", Ws, hd, hd, 0, 0, false) ||
                           make(mp + "shared_experts.up_proj.weight", Ws, hd, hd, 0, 0, false) ||
                           make(mp + "shared_experts.down_proj.weight", hd, Ws, Ws, 0, 0, false)))
                return 1;
            if (c.tp_size > 1) {
                // expert tensor parallel: rows [r I_l, +I_l) of every expert's gate / up, the same columns of its down projection
                const int64_t Il = m->moe_I;
                bf16_t *wg = nullptr, *wu = nullptr;
                if (dev_alloc(m, &wg, (size_t)(E * Il * hd)) || dev_alloc(m, &wu, (size_t)(E * Il * hd))) return 1;
                const uint32_t sg = base_seed ^ crc32_str((mp + "switch_mlp.gate_proj.weight").c_str());
                const uint32_t su = base_seed ^ crc32_str((mp + "switch_mlp.up_proj.weight").c_str());
                for (int64_t e = 0; e < E; ++e)
                    if (omx_fill_uniform_2d(wg + e * Il * hd, Il, hd, hd, e * Im + (int64_t)r * Il, 0, sg, amp_w, 0.f, OMX_BFLOAT16, m->stream) ||
                        omx_fill_uniform_2d(wu + e * Il * hd, Il, hd, hd, e * Im + (int64_t)r * Il, 0, su, amp_w, 0.f, OMX_BFLOAT16, m->stream))
                        return 1;
                m->named[mp + "switch_mlp.gate_proj.weight"] = wg;
                m->named[mp + "switch_mlp.up_proj.weight"] = wu;
                if (make(mp + "gate.weight", E, hd, hd, 0, 0, false) ||
                    make(mp + "switch_mlp.down_proj.weight", E * hd, Il, Im, 0, (int64_t)r * Il, false))
                    return 1;
            } else
            if (make(mp + "gate.weight", E, hd, hd, 0, 0, false) ||
                make(mp + "switch_mlp.gate_proj.weight", El * Im, hd, hd, e0 * Im, 0, false) ||
                make(mp + "switch_mlp.up_proj.weight", El * Im, hd, hd, e0 * Im, 0, false) ||
                make(mp + "switch_mlp.down_proj.weight", El * hd, Im, Im, e0 * hd, 0, false))
                return 1;
        } else if (make(p + "mlp.gate_proj.weight", m->I, hd, hd, (int64_t)r * m->I, 0, false) ||
                   make(p + "mlp.up_proj.weight", m->I, hd, hd, (int64_t)r * m->I, 0, false) ||
                   make(p + "mlp.down_proj.weight", hd, m->I, c.intermediate_size, 0, (int64_t)r * m->I, false)) {
            return 1;
        }
    }
    if (peaked) {
        const uint32_t seed = base_seed ^ crc32_str("model.embed_tokens.weight");
        bf16_t *e = nullptr, *hw = nullptr;
        if (dev_alloc(m, &e, (size_t)c.vocab_size * hd) || dev_alloc(m, &hw, (size_t)m->V * hd)) return 1;
        if (omx_fill_uniform_2d(e, c.vocab_size, hd, hd, 0, 0, seed, (float)(64.0 * sqrt(3.0)), 0.f, OMX_BFLOAT16, m->stream)) return 1;
        // this rank's head rows [r V_l, (r + 1) V_l) = table rows shifted by one, wrapping at the end of the vocabulary
        const int64_t first = (int64_t)r * m->V + 1, n_main = std::min<int64_t>(m->V, c.vocab_size - first);
        if (n_main > 0 && omx_fill_uniform_2d(hw, n_main, hd, hd, first, 0, seed, amp_w, 0.f, OMX_BFLOAT16, m->stream)) return 1;
        if (n_main < m->V && omx_fill_uniform_2d(hw + (size_t)std::max<int64_t>(n_main, 0) * hd, m->V - std::max<int64_t>(n_main, 0), hd, hd, 0, 0, seed,
                                                 amp_w, 0.f, OMX_BFLOAT16, m->stream))
            return 1;
        m->named["model.embed_tokens.weight"] = e;
        m->named["lm_head.weight"] = hw;
        if (make("model.norm.weight", 1, hd, hd, 0, 0, true)) return 1;
    } else {
    if (make("model.embed_tokens.weight", c.vocab_size, hd, hd, 0, 0, false) || make("model.norm.weight", 1, hd, hd, 0, 0, true))
        return 1;
    if (!c.tie_word_embeddings) {
        if (make("lm_head.weight", m->V, hd, hd, (int64_t)r * m->V, 0, false)) return 1;
    } else if (c.tp_size > 1) {
        // vocab shard of the tied table, same logical values as model.embed_tokens.weight
        bf16_t* p = nullptr;
        if (dev_alloc(m, &p, (size_t)m->V * hd)) return 1;
        const uint32_t seed = base_seed ^ crc32_str("model.embed_tokens.weight");
        if (omx_fill_uniform_2d(p, m->V, hd, hd, (int64_t)r * m->V, 0, seed, amp_w, 0.f, OMX_BFLOAT16, m->stream)) return 1;
        m->named["lm_head.weight"] = p;
    }
    }
    OMX_HIP_CHECK(hipStreamSynchronize(m->stream));
    m->weights_resolved = false;
    return 0;
}

extern "C" {

int omx_qwen3_synth_weights(omx_qwen3 m, uint32_t base_seed) { return synth_weights_impl(m, base_seed, false); }
/* The same synthetic checkpoint with PEAKED logits (parity at full size: i.i.d. weights give flat logits whose argmax flips on the last
 * bf16 bit, so token equality cannot be a hard assert): the embedding table is scaled to std 64 -- it dominates the ~10-rms sum of the
 * 36 layers' contributions -- and lm_head row v is row (v + 1) mod V of the SAME table at the usual std 0.02, so the greedy token after
 * token t is t - 1 with a top-1 margin of ~80 against a bf16 bound of ~0.5, while the other 151 935 logits still carry the layers'
 * arithmetic (std 0.2 of their 1.3).  oracle/ref_qwen3.py synth_weights(peaked=True) is the host twin. */
int omx_qwen3_synth_weights_peaked(omx_qwen3 m, uint32_t base_seed) { return synth_weights_impl(m, base_seed, true); }

}  // extern "C"
