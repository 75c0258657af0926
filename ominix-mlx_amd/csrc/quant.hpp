// Packed-weight (MLX affine 2/3/4/5/6/8-bit) GEMV family: the decode-time Linear of a quantized checkpoint
// (nn::QuantizedLinear::forward, mlx-rs/src/nn/quantized.rs:361-385; quant.hip for the format).
#pragma once
#include "act16.hpp"
#include "common.hpp"
#include "gemv.hpp"   // PRO_* / EPI_* codes shared with the bf16 GEMV family

namespace omx {

struct QMat {               // one member of a row-stacked weight (q | k | v) -- or gate (0) / up (1) for SwiGLU
    const uint32_t* w;      // [n, K*bits/32]
    const bf16_t* scales;   // [n, K/group]
    const bf16_t* biases;   // [n, K/group] or null
    int n;
    // optional repack built by the engine at load time: word g = scale[g] | bias[g] << 16, so that a lane fetches both with ONE
    // 4-byte load (two 2-byte loads per 16 bytes of weights cost the 4-bit GEMV 15 % of its streaming rate)
    const uint32_t* sb = nullptr;
    // optional second repack (round 6, qgemv_mfma.hip): the matrix in 9 KB tiles of 16 rows x 1 024 columns (words in the order the
    // matrix-core kernel's lanes consume them, the tile's scale | bias words behind them) -- 4-bit, group 64, K = 4096 / 12288
    const uint32_t* tiles = nullptr;
    // the matrix's own MLX format where it travels with the matrix (a checkpoint whose matrices differ: the engine fills both in for
    // every matrix); 0 = the launch's (launch_qgemv's `bits`, QGemvArgs::group)
    int bits = 0, group = 0;
};
int launch_quant_interleave(uint32_t* sb, const bf16_t* scales, const bf16_t* biases, size_t n_groups, hipStream_t s);
// The raw-pointer C entry points (omx_moe_block_forward_q ...) receive the checkpoint's scales pointer; an engine that built the
// repack registers it under that pointer so those entry points find it (and removes it before freeing the repack).
void quant_register_sb(const bf16_t* scales, const uint32_t* sb);
void quant_unregister_sb(const bf16_t* scales);
const uint32_t* quant_find_sb(const bf16_t* scales);

struct QGemvArgs {
    QMat m[3];
    int N, K, group;
    const bf16_t* x;            // [n_x, K]
    const bf16_t* norm_w;       // PRO_RMSNORM
    float eps;
    const bf16_t* resid;        // EPI_RESIDUAL
    bf16_t* out;                // [n_batch, N]
    unsigned long long* argmax_slot;   // EPI_ARGMAX: one partial per block
    int rows_per_wave;
    int n_batch, x_div;         // batch entry j reads activation row j / x_div
    const uint32_t* w_sel;      // optional [n_batch] expert ids (gather_qmm)
    size_t w_estride, s_estride;    // words / groups between consecutive experts
    int swiglu_single_round;    // EPI_SWIGLU: fused_swiglu(up, gate) (one rounding, metal_kernels.rs:11-18) instead of nn::silu(g)*u
    int rolled_stage;           // A/B: stage the activation with the rolled loop (OMX_QGEMV_ROLLED_STAGE=1)
    int scales_f16;             // scales / biases (and QMat::sb's halves) hold float16 bit patterns: a float16 MLX checkpoint.  The
                                // activations, norm weights, residual and outputs are float16 too then (Act16<true>: x, norm_w, resid
                                // and out hold float16 bit patterns); every group's scale / bias enters the arithmetic as its exact
                                // float32 value
    // tensor parallel (round 4): EPI_F32 leaves the unrounded f32 row sums of this rank's K slice in out_f32 [N] (the all-reduce and the
    // fold into the residual follow as their own launches); EPI_ARGMAX numbers its rows from row_offset (this rank's vocabulary shard)
    float* out_f32;             // (batched: [n_batch, N])
    int row_offset;
    // expert parallel (round 5): only batch entries whose w_sel value lies in [w_sel_lo, w_sel_lo + w_sel_n) are computed, on expert
    // w_sel - w_sel_lo of this rank's stack; the others leave their output rows untouched (w_sel_n == 0: every entry, as before)
    int w_sel_lo, w_sel_n;
};
// packed [rows, cols*bits/32] -> bf16 [rows, cols]; scales_f16: scales / biases are float16 (engine-internal form of omx_dequantize)
int launch_dequantize_bf16(bf16_t* out, const uint32_t* packed, const void* scales, const void* biases, int64_t rows, int cols, int group_size,
                           int bits, bool scales_f16, hipStream_t s, bool out_f16 = false);   // out_f16: the result in float16 (a float16 model's prompt pass)

// bits / a.group: the format of every member that carries none of its own (QMat::bits / group == 0).  Members of one format: today's
// launches.  Members that differ (EPI_STORE stacks of bf16 triplets, one activation row): ONE launch of qgemv_stack_kernel.  Either way a
// member's rows are bit for bit what the VALU kernel gives for that member launched alone.
// route (optional): what the launch resolved to, filled in by the launcher that takes it -- untouched where the launch is refused
struct QGemvRoute {
    int dry_run;              // in: fill in the route and launch nothing (no device needed)
    int kernel;               // 1 qgemv_kernel (VALU, one format), 2 qgemv_stack_kernel (mixed formats), 3 qgemv4m_kernel (matrix cores)
    int bits, W, RB;          // the instantiation (stack: 0, 0 -- each member runs its own <BITS, W>; matrix cores: 4, 4, 0)
    int rows_per_wave;        // resolved (matrix cores: 0, a wave owns a 16-row tile)
    int SB, F16S;
    int blocks, lds_bytes;    // blocks along x, dynamic LDS bytes
    int KS, NU, NBUF;         // matrix cores only
};
int launch_qgemv(const QGemvArgs& a, int bits, int pro, int epi, hipStream_t s, QGemvRoute* route = nullptr);
// the format member i of a launch runs in
inline int qmat_bits(const QMat& m, int dflt) { return m.bits ? m.bits : dflt; }
inline int qmat_group(const QMat& m, int dflt) { return m.group ? m.group : dflt; }
// qgemv_mfma.hip (round 6): the dense 4-bit group-64 single-row forms on the matrix cores.  0 launched, -1 not its shape (take the VALU kernel), 1 error
int launch_qgemv4m(const QGemvArgs& a, int pro, int epi, hipStream_t s, QGemvRoute* route = nullptr);
bool qgemv4m_shape_ok(int K, int group, int bits);
size_t qgemv4m_tile_words(int n, int K);            // u32 words of the tile form of an [n, K] matrix
int launch_qgemv4m_repack(uint32_t* tiles, const uint32_t* wq, const bf16_t* scales, const bf16_t* biases, int n, int K, hipStream_t s);
int qgemv_grid(int N);          // blocks launch_qgemv's VALU kernel uses for an EPI_ARGMAX launch == argmax partials the engines reduce

// qgemv_rows.hip: M <= 8 activation rows against one packed matrix (or a q | k | v stack, a gate / up pair) with every packed word read
// once per launch -- the speculative verify pass of a quantized checkpoint.  g carries launch_qgemv's fields with their meaning for ONE
// row, except that x [M, K], resid [M, N] and out [M, N] hold M rows; bf16 triplets, forms PRO_NONE / PRO_RMSNORM x EPI_STORE,
// PRO_NONE x EPI_RESIDUAL, PRO_NONE / PRO_RMSNORM x EPI_SWIGLU.  Row t of the result is bit-identical to launch_qgemv on row t alone
// (no matrix-core tiles).
struct QRowsArgs {
    QGemvArgs g;
    int M;
    bf16_t* mout[3];     // optional (not SwiGLU): member i's rows go to mout[i] [M, m[i].n] instead of out
    int nb;              // (set by the launcher)
};
int launch_qgemv_rows(const QRowsArgs& a, int bits, int pro, int epi, hipStream_t s);

// The widths whose fields do not divide a word (3, 5, 6) and 2: a run of 32 elements is exactly BITS consecutive words, element j the
// BITS-wide field at bit j * BITS of that little-endian bit string (a field may straddle two words).  j must be a compile-time constant
// after unrolling: one v_bfe_u32, or v_alignbit + mask for a straddling field.
inline bool quant_bits_ok(int bits) { return bits == 2 || bits == 3 || bits == 4 || bits == 5 || bits == 6 || bits == 8; }   // MLX's affine widths
constexpr bool quant_chunked(int bits) { return bits == 2 || bits == 3 || bits == 5 || bits == 6; }
template <int B>
__device__ __forceinline__ uint32_t qfield(const uint32_t* w, int j) {
    const int p = j * B, k = p >> 5, o = p & 31;
    if (o + B <= 32) return (w[k] >> o) & ((1u << B) - 1u);
    return __builtin_amdgcn_alignbit(w[k + 1], w[k], o) & ((1u << B) - 1u);
}

// ---- the unpack and the activation staging of the packed GEMVs (quant.hip, qgemv_rows.hip, qgemv_mfma.hip), written once ----
// A = Act16<F16S>.  A field q becomes a 16-bit float by bit assembly: kMagicBytes' exponent byte over it, bf16 0x4300 | q = 128 + q,
// float16 0x6400 | q = 1024 + q, so each dot product accumulates x . (magic + q); the bf16 form's 128 * sum(x) excess is folded into
// the bias term (bias - 128 scale) * sum(x), the float16 form takes its 1024 off again before the product (A::unmagic).
// 4 bits: the eight nibbles of a word as four magic-biased pairs.  One v_perm per pair: the exponent byte comes from the second source,
// the two nibble bytes from the same masked word -- so the pairs are (q0, q2), (q4, q6) of the even nibbles and (q1, q3), (q5, q7) of
// the odd ones, and the activations are staged in that order (stage_octet4)
template <class A>
__device__ __forceinline__ void nibble_pairs(uint32_t wdw, uint32_t* out) {
    const uint32_t lo = wdw & 0x0F0F0F0Fu, hi = (wdw >> 4) & 0x0F0F0F0Fu;
    const uint32_t c43 = A::kMagicBytes;
    constexpr uint32_t kBytes02 = 0x04010400u, kBytes13 = 0x04030402u;   // (magic, byte 1, magic, byte 0), (magic, byte 3, magic, byte 2)
    out[0] = __builtin_amdgcn_perm(c43, lo, kBytes02);
    out[1] = __builtin_amdgcn_perm(c43, lo, kBytes13);
    out[2] = __builtin_amdgcn_perm(c43, hi, kBytes02);
    out[3] = __builtin_amdgcn_perm(c43, hi, kBytes13);
}
// eight consecutive activations (x0 .. x7, four packed pairs) as (x0,x2) (x4,x6) (x1,x3) (x5,x7): the pairing of nibble_pairs
__device__ __forceinline__ u32x4 stage_octet4(const u32x4 o) {
    u32x4 t;
    t[0] = __builtin_amdgcn_perm(o[1], o[0], 0x05040100u); t[1] = __builtin_amdgcn_perm(o[3], o[2], 0x05040100u);
    t[2] = __builtin_amdgcn_perm(o[1], o[0], 0x07060302u); t[3] = __builtin_amdgcn_perm(o[3], o[2], 0x07060302u);
    return t;
}
// 2 / 3 / 5 / 6 bits: elements 2 i and 2 i + 1 of a run of 32 as one magic-biased pair, natural order -- each field one v_bfe_u32
// (v_alignbit for a straddling one), the pair one v_lshl_or_b32 + one v_or_b32 of the magic
template <int BITS, class A>
__device__ __forceinline__ uint32_t field_pair(const uint32_t* wd, int i) {
    const uint32_t q0 = qfield<BITS>(wd, 2 * i), q1 = qfield<BITS>(wd, 2 * i + 1);
    return ((q1 << 16) | q0) | (A::kMagicBytes & 0xFF00FF00u);
}
// Stage the eight activations o = x[i, i + 8) of a row: into xs (OCTET4: in the 4-bit kernels' order) and into the sum over each lane
// chunk of EPL elements that every row's bias term shares, xsum[i / EPL] -- EPL / 8 consecutive threads hold a chunk and reduce it
// by DPP, so thread t of the block must stage vector t (+ a multiple of 64) of the row
template <class A, int EPL, bool OCTET4>
__device__ __forceinline__ void stage_chunk(bf16_t* xs, float* xsum, int i, const u32x4 o) {
    static_assert(EPL == 8 || EPL == 16 || EPL == 32 || EPL == 64, "a lane chunk is 1, 2, 4 or 8 activation vectors");
    *reinterpret_cast<u32x4*>(xs + i) = OCTET4 ? stage_octet4(o) : o;
    float sv = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) sv += A::lo(o[q]) + A::hi(o[q]);
    if (EPL >= 16) sv += dpp_f<kDppXor1>(sv);
    if (EPL >= 32) sv += dpp_f<kDppXor2>(sv);
    if (EPL >= 64) sv += dpp_f<kDppHalfMirror>(sv);
    if (((i >> 3) & (EPL / 8 - 1)) == 0) xsum[i / EPL] = sv;
}

// MLX affine_quantize of one group, given its extremes: the f32 scale and bias the codes are computed with (the stored pair is their
// rounding to the scales' dtype).  The text of quantize_kernel (quant.hip) and of the 8-bit K/V cache's append (prefill.hip)
__device__ __forceinline__ void affine_group(float mx, float mn, float n_bins, float& scale, float& bias) {
    scale = fmaxf((mx - mn) / n_bins, 1e-7f);
    const bool side = fabsf(mn) > fabsf(mx);
    scale = side ? scale : -scale;
    const float edge = side ? mn : mx;
    const float q0 = rintf(edge / scale);
    const bool at_zero = q0 == 0.f;
    scale = at_zero ? scale : edge / q0;
    bias = at_zero ? 0.f : edge;
}
// ... and the code of element v under that pair
__device__ __forceinline__ float affine_code(float v, float scale, float bias, float n_bins) {
    return fminf(fmaxf(rintf((v - bias) / scale), 0.f), n_bins);
}

// One row of QuantizedEmbedding::forward straight from the packed table, by one block: element j of row `id` as (float)q * scale + bias
// with one rounding, the expression of dequantize_kernel / dequantize_chunk_kernel (quant.hip).  The text of qembed_rows_kernel
// (engine_prefill.hip) and of the packed batch_embed_kernel (engine_batch.hip)
template <int BITS>
__device__ __forceinline__ void qembed_row(bf16_t* __restrict__ out, const uint32_t* __restrict__ table, const bf16_t* __restrict__ scales,
                                           const bf16_t* __restrict__ biases, size_t id, int hidden, int group) {
    const uint32_t* wrow = table + id * (size_t)(hidden / 32 * BITS);
    const bf16_t* srow = scales + id * (size_t)(hidden / group);
    const bf16_t* brow = biases ? biases + id * (size_t)(hidden / group) : nullptr;
    for (int j = threadIdx.x; j < hidden; j += blockDim.x) {
        const int p = j * BITS, k = p >> 5, o = p & 31;
        const uint32_t q = (o + BITS <= 32 ? wrow[k] >> o : __builtin_amdgcn_alignbit(wrow[k + 1], wrow[k], o)) & ((1u << BITS) - 1u);
        const float sc = bf16_to_f32(srow[j / group]), b = brow ? bf16_to_f32(brow[j / group]) : 0.f;
        out[j] = f32_to_bf16((float)q * sc + b);
    }
}

}  // namespace omx
