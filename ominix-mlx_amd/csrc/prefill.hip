// Glue kernels of the batched (T > 1) prefill step of the decode engine; each fuses what the
// reference issues as several lazy ops.
#include "attn_row.hpp"
#include "engine_model.hpp"
#include "quant.hpp"

namespace omx {
namespace {

// A K/V slab as a scatter row policy names it (Slab), and the store of the 8 bf16 elements `o` that lane c holds of its row `row`.
// bf16 slabs [rows, D]: as they are
template <int D>
__device__ __forceinline__ void put_row(bf16_t* slab, size_t row, int c, const u32x4 o) {
    *reinterpret_cast<u32x4*>(slab + row * D + c * 8) = o;
}
// The 8-bit slabs of a kv_bits = 8 batch (KvAffine8's layout, attn_row.hpp): the row quantised as it is appended.  A 64-element group
// is 8 lanes: its extremes by DPP, affine_group / affine_code (quant.hpp: quantize_kernel's arithmetic, 8 bits), the lane's 8 codes in
// one 8-byte store, the pair rounded to bf16 by the group's first lane.  Returns the elements as every attention will read them,
// (float)code * scale + bias, rounded to bf16
struct Kv8Slab {
    uint8_t* q;
    uint32_t* sb;
};
template <int D>
__device__ __forceinline__ u32x4 put_row(const Kv8Slab slab, size_t row, int c, const u32x4 o) {
    float x[8];
    unpack8(o, x);
    float mx = x[0], mn = x[0];
#pragma unroll
    for (int e = 1; e < 8; ++e) {
        mx = fmaxf(mx, x[e]);
        mn = fminf(mn, x[e]);
    }
    mx = group_max<8>(mx);
    mn = -group_max<8>(-mn);
    float scale, bias;
    affine_group(mx, mn, 255.f, scale, bias);
    Kv8Raw r = {};
#pragma unroll
    for (int e = 0; e < 8; ++e) r.q[e >> 2] |= (uint32_t)affine_code(x[e], scale, bias, 255.f) << (8 * (e & 3));
    r.sb = pack_bf16(scale, bias);
    *reinterpret_cast<u32x2*>(slab.q + row * D + c * 8) = r.q;
    if ((c & 7) == 0) slab.sb[row * (D / 64) + c / 8] = r.sb;
    KvAffine8::unpack(r, x);
    u32x4 y;
#pragma unroll
    for (int e = 0; e < 4; ++e) y[e] = pack_bf16(x[2 * e], x[2 * e + 1]);
    return y;
}

// Where the rows of a qk_norm_rope_scatter_kernel launch live: row t's position and K/V slabs, and the q_out row of (t, head h).
// A prompt: token t at position offset + t of one pair of slabs; q_out[h][t][:] (the [B,H,T,D] operand of SDPA)
struct PromptRows {
    typedef bf16_t* Slab;
    bf16_t *kcache, *vcache;
    int offset;
    __device__ __forceinline__ void at(int t, int cap, int& pos, bf16_t*& k, bf16_t*& v) const { pos = offset + t; k = kcache; v = vcache; }
    static __device__ __forceinline__ size_t q_row(int t, int h, int T, int H) { return (size_t)h * T + t; }
};
// The ragged rows of a batched decode step (engine_batch.hip): row t is the pending token of slot row_slot[t], at that slot's position
// in that slot's slabs; q_out[t][h][:]
struct SlotRows {
    typedef bf16_t* Slab;
    bf16_t *kbase, *vbase;
    size_t slot_stride;
    const BatchSlot* slots;
    const int* row_slot;
    __device__ __forceinline__ void at(int t, int cap, int& pos, bf16_t*& k, bf16_t*& v) const {
        const int slot = row_slot[t];
        pos = min(slots[slot].pos, cap - 1);   // (the host refuses a step past the slab's end before it launches anything)
        k = kbase + (size_t)slot * slot_stride;
        v = vbase + (size_t)slot * slot_stride;
    }
    static __device__ __forceinline__ size_t q_row(int t, int h, int T, int H) { return (size_t)t * H + h; }
};
// ... of a kv_bits = 8 batch: the same rows, appended to the slot's 8-bit slabs
struct SlotRows8 {
    typedef Kv8Slab Slab;
    Kv8Layer base;
    size_t slot_stride, sb_stride;
    const BatchSlot* slots;
    const int* row_slot;
    __device__ __forceinline__ void at(int t, int cap, int& pos, Kv8Slab& k, Kv8Slab& v) const {
        const int slot = row_slot[t];
        pos = min(slots[slot].pos, cap - 1);
        k = {base.kq + (size_t)slot * slot_stride, base.ksb + (size_t)slot * sb_stride};
        v = {base.vq + (size_t)slot * slot_stride, base.vsb + (size_t)slot * sb_stride};
    }
    static __device__ __forceinline__ size_t q_row(int t, int h, int T, int H) { return (size_t)t * H + h; }
};

// One D/8-lane group per (token, head) row.  q rows: per-head RMSNorm -> RoPE -> q_out; k rows: same, written straight into the KV
// slab at the row's position (KVCache::update_and_fetch, cache.rs:183-188); v rows: copied into the slab.
//   reference: qwen3-mlx/src/model.rs:172-196 (reshape/transpose, q_norm/k_norm, rope, cache update).
// Rows: PromptRows / SlotRows / SlotRows8 (k and v rows go to the slab through put_row).  F16: a float16 model (float16 rows, norm weights, cache slabs and rounding points: act16.hpp)
template <int D, class Rows, bool F16 = false>
__global__ __launch_bounds__(256) void qk_norm_rope_scatter_kernel(
    const bf16_t* __restrict__ q_lin, const bf16_t* __restrict__ k_lin, const bf16_t* __restrict__ v_lin,
    const bf16_t* __restrict__ q_norm_w, const bf16_t* __restrict__ k_norm_w, const float* __restrict__ rope_cos,
    const float* __restrict__ rope_sin, bf16_t* __restrict__ q_out, const Rows rows, int T, int H, int Hkv, int cap, float eps) {
    typedef Act16<F16> A16;
    constexpr int LPR = D / 8;
    const int lane = threadIdx.x & 63;
    const int c = lane % LPR;
    const int rows_per_block = 256 / LPR;
    const int64_t row = (int64_t)blockIdx.x * rows_per_block + threadIdx.x / LPR;
    const int per_tok = H + 2 * Hkv;
    if (row >= (int64_t)T * per_tok) return;
    const int t = (int)(row / per_tok), hh = (int)(row % per_tok);
    int pos;
    typename Rows::Slab kcache, vcache;
    rows.at(t, cap, pos, kcache, vcache);
    if (hh >= H + Hkv) {   // v: plain copy into the slab
        const int kvh = hh - H - Hkv;
        put_row<D>(vcache, (size_t)kvh * cap + pos, c, *reinterpret_cast<const u32x4*>(v_lin + ((size_t)t * Hkv + kvh) * D + c * 8));
        return;
    }
    const bool is_q = hh < H;
    const bf16_t* src = is_q ? q_lin + ((size_t)t * H + hh) * D : k_lin + ((size_t)t * Hkv + (hh - H)) * D;
    const bf16_t* w = is_q ? q_norm_w : k_norm_w;
    const u32x4 r = *reinterpret_cast<const u32x4*>(src + c * 8);
    const u32x4 wr = w ? *reinterpret_cast<const u32x4*>(w + c * 8) : (F16 ? u32x4{0x3C003C00u, 0x3C003C00u, 0x3C003C00u, 0x3C003C00u} : u32x4{0x3F803F80u, 0x3F803F80u, 0x3F803F80u, 0x3F803F80u});   // no q/k norm (Mixtral): weight 1
    float x[8], wv[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        x[2 * e] = A16::lo(r[e]); x[2 * e + 1] = A16::hi(r[e]);
        wv[2 * e] = A16::lo(wr[e]); wv[2 * e + 1] = A16::hi(wr[e]);
    }
    float ss = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) ss = fmaf(x[e], x[e], ss);
    ss = group_sum<LPR>(ss);
    const float rstd = w ? 1.0f / sqrtf(ss / (float)D + eps) : 1.0f;   // without a norm the projection goes to RoPE as it is
    const int i0 = (c % (LPR / 2)) * 8;
    const bool first_half = c < LPR / 2;
    float y[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float xn = A16::rnd(x[e] * rstd * wv[e]);
        // partner element i +- D/2 lives in lane c ^ (LPR/2)
        const float other = (LPR == 16) ? dpp_f<0x128>(xn) : dpp_f<0x1B>(dpp_f<kDppHalfMirror>(xn));
        const float cs = rope_cos[(size_t)pos * (D / 2) + i0 + e], sn = rope_sin[(size_t)pos * (D / 2) + i0 + e];
        y[e] = first_half ? xn * cs - other * sn : other * sn + xn * cs;
    }
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = A16::pack(y[2 * e], y[2 * e + 1]);
    if (is_q) *reinterpret_cast<u32x4*>(q_out + Rows::q_row(t, hh, T, H) * D + c * 8) = o;
    else put_row<D>(kcache, (size_t)(hh - H) * cap + pos, c, o);
}

// The two hooks of a prompt pass on a kv_bits = 8 batch (prefill_prefix_batched, KvSlabs::packed), over rows [r0, r0 + n) of every KV
// head of one layer, K and V in one launch, one D/8-lane group per row.  PACK = false: the slot's packed rows expanded into the bf16
// staging pair the pass attends over.  PACK = true: the staging rows the scatter has just written packed into the slot's slabs
// (put_row) and overwritten with their dequantised values -- the prompt's attention reads what a decode step will read
template <int D, bool PACK>
__global__ __launch_bounds__(256) void kv8_rows_kernel(const Kv8Slab kq, const Kv8Slab vq, bf16_t* __restrict__ ks, bf16_t* __restrict__ vs,
                                                       int Hkv, int cap, int r0, int n) {
    constexpr int LPR = D / 8;
    const int64_t id = ((int64_t)blockIdx.x * 256 + threadIdx.x) / LPR;
    const int c = threadIdx.x % LPR;
    if (id >= (int64_t)2 * Hkv * n) return;
    const bool is_v = id >= (int64_t)Hkv * n;
    const int rr = (int)(id % ((int64_t)Hkv * n));
    const size_t row = (size_t)(rr / n) * cap + r0 + rr % n;
    const Kv8Slab slab = is_v ? vq : kq;
    u32x4* st = reinterpret_cast<u32x4*>((is_v ? vs : ks) + row * D + c * 8);
    if (PACK) {
        *st = put_row<D>(slab, row, c, *st);
    } else {
        Kv8Raw r;
        r.q = *reinterpret_cast<const u32x2*>(slab.q + row * D + c * 8);
        r.sb = slab.sb[row * (D / 64) + c / 8];
        float x[8];
        KvAffine8::unpack(r, x);
        u32x4 y;
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = pack_bf16(x[2 * e], x[2 * e + 1]);
        *st = y;
    }
}

// nn::silu(gate) * up with every primitive's result held in bf16 (qwen3-mlx/src/model.rs:264-265)
__global__ __launch_bounds__(256) void silu_mul_kernel(bf16_t* __restrict__ out, const bf16_t* __restrict__ gate,
                                                       const bf16_t* __restrict__ up, int64_t n_vec) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_vec; i += (int64_t)gridDim.x * 256) {
        const u32x4 g = reinterpret_cast<const u32x4*>(gate)[i];
        const u32x4 u = reinterpret_cast<const u32x4*>(up)[i];
        u32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float r[2];
#pragma unroll
            for (int hlf = 0; hlf < 2; ++hlf) {
                const float gv = hlf ? bf16hi(g[e]) : bf16lo(g[e]);
                const float uv = hlf ? bf16hi(u[e]) : bf16lo(u[e]);
                const float sg = round_bf16(1.0f / (1.0f + expf(-gv)));
                r[hlf] = round_bf16(gv * sg) * uv;
            }
            o[e] = pack_bf16(r[0], r[1]);
        }
        reinterpret_cast<u32x4*>(out)[i] = o;
    }
}

}  // namespace

int launch_qk_norm_rope_scatter(const bf16_t* q_lin, const bf16_t* k_lin, const bf16_t* v_lin, const bf16_t* q_norm_w,
                                const bf16_t* k_norm_w, const float* rope_cos, const float* rope_sin, bf16_t* q_out,
                                bf16_t* kcache, bf16_t* vcache, int T, int H, int Hkv, int D, int cap, int offset,
                                float eps, hipStream_t s, bool f16) {
    OMX_REQUIRE(D == 64 || D == 128, "qk_norm_rope: head_dim %d unsupported", D);
    const int64_t rows = (int64_t)T * (H + 2 * Hkv);
    const int rpb = 256 / (D / 8);
    const unsigned blocks = (unsigned)((rows + rpb - 1) / rpb);
    const PromptRows at = {kcache, vcache, offset};
    if (f16) {
        OMX_REQUIRE(D == 128, "qk_norm_rope: float16 models have head_dim 128");
        qk_norm_rope_scatter_kernel<128, PromptRows, true><<<blocks, 256, 0, s>>>(q_lin, k_lin, v_lin, q_norm_w, k_norm_w, rope_cos, rope_sin,
                                                                                  q_out, at, T, H, Hkv, cap, eps);
    } else
    if (D == 128)
        qk_norm_rope_scatter_kernel<128, PromptRows><<<blocks, 256, 0, s>>>(q_lin, k_lin, v_lin, q_norm_w, k_norm_w, rope_cos, rope_sin,
                                                                            q_out, at, T, H, Hkv, cap, eps);
    else
        qk_norm_rope_scatter_kernel<64, PromptRows><<<blocks, 256, 0, s>>>(q_lin, k_lin, v_lin, q_norm_w, k_norm_w, rope_cos, rope_sin,
                                                                           q_out, at, T, H, Hkv, cap, eps);
    OMX_LAUNCH_CHECK();
    return 0;
}

// the same launch over the ragged rows of a batched decode step: q rows -> pf_qt[r][h][:], k / v rows -> the slabs of the row's slot
int launch_batch_scatter(omx_qwen3 m, int layer, const RaggedRows& rag, int T, hipStream_t s) {
    const omx_qwen3_config& c = m->cfg;
    const LayerW& L = m->layers[layer];
    const int D = c.head_dim, H = m->H, Hkv = m->Hkv;
    const int64_t rows = (int64_t)T * (H + 2 * Hkv);
    const int rpb = 256 / (D / 8);
    const unsigned blocks = (unsigned)((rows + rpb - 1) / rpb);
    if (rag.kv8) {   // a kv_bits = 8 batch: the k / v rows quantised as they are appended
        const SlotRows8 at8 = {rag.kv8[layer], rag.slot_stride, rag.sb_stride, rag.slots, rag.row_slot};
        if (D == 128)
            qk_norm_rope_scatter_kernel<128, SlotRows8><<<blocks, 256, 0, s>>>(m->pf_q, m->pf_k, m->pf_v, L.q_norm, L.k_norm, m->rope_cos, m->rope_sin,
                                                                               m->pf_qt, at8, T, H, Hkv, rag.cap, c.rms_norm_eps);
        else
            qk_norm_rope_scatter_kernel<64, SlotRows8><<<blocks, 256, 0, s>>>(m->pf_q, m->pf_k, m->pf_v, L.q_norm, L.k_norm, m->rope_cos, m->rope_sin,
                                                                              m->pf_qt, at8, T, H, Hkv, rag.cap, c.rms_norm_eps);
        OMX_LAUNCH_CHECK();
        return 0;
    }
    const SlotRows at = {rag.kbase[layer], rag.vbase[layer], rag.slot_stride, rag.slots, rag.row_slot};
    if (D == 128)
        qk_norm_rope_scatter_kernel<128, SlotRows><<<blocks, 256, 0, s>>>(m->pf_q, m->pf_k, m->pf_v, L.q_norm, L.k_norm, m->rope_cos, m->rope_sin,
                                                                          m->pf_qt, at, T, H, Hkv, rag.cap, c.rms_norm_eps);
    else
        qk_norm_rope_scatter_kernel<64, SlotRows><<<blocks, 256, 0, s>>>(m->pf_q, m->pf_k, m->pf_v, L.q_norm, L.k_norm, m->rope_cos, m->rope_sin,
                                                                         m->pf_qt, at, T, H, Hkv, rag.cap, c.rms_norm_eps);
    OMX_LAUNCH_CHECK();
    return 0;
}

// rows [r0, r0 + n) of one layer of a slot's 8-bit slabs <-> the bf16 staging pair ks / vs [Hkv, cap, D] (kv8_rows_kernel)
int launch_kv8_rows(const Kv8Layer& L, bf16_t* ks, bf16_t* vs, int Hkv, int D, int cap, int r0, int n, bool pack, hipStream_t s) {
    OMX_REQUIRE(D == 64 || D == 128, "kv8 rows: head_dim %d unsupported", D);
    OMX_REQUIRE(r0 >= 0 && n >= 0 && r0 + n <= cap, "kv8 rows: rows [%d, %d) of %d", r0, r0 + n, cap);
    if (n == 0) return 0;
    const int64_t lanes = (int64_t)2 * Hkv * n * (D / 8);
    const unsigned blocks = (unsigned)((lanes + 255) / 256);
    const Kv8Slab kq = {L.kq, L.ksb}, vq = {L.vq, L.vsb};
    if (D == 128 && pack) kv8_rows_kernel<128, true><<<blocks, 256, 0, s>>>(kq, vq, ks, vs, Hkv, cap, r0, n);
    else if (D == 128) kv8_rows_kernel<128, false><<<blocks, 256, 0, s>>>(kq, vq, ks, vs, Hkv, cap, r0, n);
    else if (pack) kv8_rows_kernel<64, true><<<blocks, 256, 0, s>>>(kq, vq, ks, vs, Hkv, cap, r0, n);
    else kv8_rows_kernel<64, false><<<blocks, 256, 0, s>>>(kq, vq, ks, vs, Hkv, cap, r0, n);
    OMX_LAUNCH_CHECK();
    return 0;
}

int launch_silu_mul(bf16_t* out, const bf16_t* gate, const bf16_t* up, int64_t n, hipStream_t s) {
    OMX_REQUIRE(n % 8 == 0, "silu_mul: element count %lld must be a multiple of 8", (long long)n);
    const int64_t nv = n / 8;
    int64_t blocks = (nv + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    silu_mul_kernel<<<(unsigned)blocks, 256, 0, s>>>(out, gate, up, nv);
    OMX_LAUNCH_CHECK();
    return 0;
}

}  // namespace omx
