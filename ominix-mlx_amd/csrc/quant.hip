// MLX affine group quantisation on gfx950 (the reference's flagship checkpoint format).
//   reference: mlx_rs::ops::{quantize, dequantize, quantized_matmul, gather_qmm}
//              (mlx-rs/src/ops/quantization.rs:41-153, 226-279) -> mlx_quantize / mlx_dequantize /
//              mlx_quantized_matmul / mlx_gather_qmm (mlx-c ops.h:356-365, 471-484, 793-810);
//              nn::QuantizedLinear::forward (mlx-rs/src/nn/quantized.rs:361-385).
// Format: w [N, K] -> packed u32 [N, K*bits/32] (element j of a row = the `bits`-wide field at bit
// (j*bits) mod 32 of word floor(j*bits/32), LSB first), scales / biases [N, K/group] in the activation
// dtype; w ~= q * scale + bias.  bits 2, 3, 4, 5, 6 or 8, group 32 / 64 / 128.  At 3 / 5 / 6 bits a field may straddle two words; a
// run of 32 elements always fills exactly `bits` words (quant_chunked, quant.hpp), the unit every kernel of those widths (and of 2 bits)
// works in.
//
// quantized_matmul (transpose = true: x . dequant(W)^T):
//   * M <= 16 (decode): weight-streaming GEMV that reads the PACKED weights -- a quarter (4-bit) of the
//     bf16 bytes.  One wave per row, each lane owns W words per step; per lane  acc += scale * sum(x_i q_i)
//     + bias * sum(x_i), the per-chunk sum(x_i) being shared by all rows (computed once per block into LDS).
//     grid.y walks the activation rows / expert-selected batch entries (gather_qmm).
//   * M > 16 (prefill): dequantise W once into the workspace, then the bf16 MFMA GEMM (gemm.hip).
#include <hip/hip_fp16.h>
#include "common.hpp"
#include "gemm.hpp"
#include <climits>
#include <mutex>
#include <unordered_map>

#include "quant.hpp"
#include "act16.hpp"
#include "gemv_parts.hpp"
#include "launch_timing.hpp"
#include "vec.hpp"
#include "workspace.hpp"

namespace omx {

namespace {

// ---- quantize: one wave per group of 32/64/128 elements (MLX affine_quantize) ----
template <int BITS, int DT = OMX_BFLOAT16>
__global__ __launch_bounds__(256) void quantize_kernel(uint32_t* __restrict__ packed, typename Elem<DT>::T* __restrict__ scales,
                                                       typename Elem<DT>::T* __restrict__ biases, const typename Elem<DT>::T* __restrict__ w,
                                                       int64_t n_groups, int group) {
    constexpr int EPW = 32 / BITS;
    constexpr float n_bins = (float)((1 << BITS) - 1);
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= n_groups) return;
    const typename Elem<DT>::T* src = w + g * group;
    const int per_lane = group / 64 > 0 ? group / 64 : 1;   // 128 -> 2, 64 -> 1, 32 -> 1 (upper half idle)
    float v[2] = {0.f, 0.f};
    float mx = -INFINITY, mn = INFINITY;
    for (int i = 0; i < per_lane; ++i) {
        const int e = lane * per_lane + i;
        if (e < group) {
            v[i] = Elem<DT>::ld(src + e);
            mx = fmaxf(mx, v[i]);
            mn = fminf(mn, v[i]);
        }
    }
    mx = wave_max(mx);
    mn = -wave_max(-mn);
    float scale, bias;
    affine_group(mx, mn, n_bins, scale, bias);
    if (lane == 0) {
        Elem<DT>::st(scales + g, scale);
        Elem<DT>::st(biases + g, bias);
    }
    if constexpr (32 % BITS != 0) {
        // 3 / 5 / 6 bits: lane L < group * BITS / 32 assembles word L of the group from the (at most 32 / BITS + 2) elements whose
        // fields touch its bits [32 L, 32 L + 32): element e sits at lane e / per_lane, slot e % per_lane
        uint32_t qv[2] = {0u, 0u};
        for (int i = 0; i < per_lane; ++i) {
            const int e = lane * per_lane + i;
            if (e < group) qv[i] = (uint32_t)affine_code(v[i], scale, bias, n_bins);
        }
        const int n_words = group * BITS / 32;
        const int e_first = (32 * lane) / BITS;
        uint64_t word = 0;
#pragma unroll
        for (int k = 0; k < 32 / BITS + 2; ++k) {
            const int e = e_first + k;                              // (every lane shuffles: the bpermute reads all lanes' values)
            const int src = min(e / per_lane, 63);
            const uint32_t a0 = __shfl(qv[0], src, 64), a1 = __shfl(qv[1], src, 64);
            const uint32_t q = (e % per_lane) ? a1 : a0;
            const int bit = e * BITS - 32 * lane;
            if (e < group && bit < 32) word |= bit >= 0 ? (uint64_t)q << bit : (uint64_t)(q >> -bit);
        }
        if (lane < n_words) packed[g * n_words + lane] = (uint32_t)word;
        return;
    }
    // pack: element e goes to word e / EPW at bit (e % EPW) * BITS; the EPW elements of a word sit in
    // EPW / per_lane consecutive lanes
    uint32_t word = 0;
    for (int i = 0; i < per_lane; ++i) {
        const int e = lane * per_lane + i;
        if (e < group) {
            const float q = affine_code(v[i], scale, bias, n_bins);
            word |= (uint32_t)q << ((e % EPW) * BITS);
        }
    }
    constexpr int kLanesPerWordMax = EPW;   // per_lane == 1
    const int lanes_per_word = EPW / per_lane;
    for (int o = 1; o < kLanesPerWordMax; o <<= 1)
        if (o < lanes_per_word) word |= __shfl_xor(word, o, 64);
    const int e0 = lane * per_lane;
    if (e0 < group && (lane % lanes_per_word) == 0) packed[(g * group + e0) / EPW] = word;
}

// a 16-bit scale / bias pattern as float32: bfloat16, or float16 for a float16 checkpoint
template <bool F16>
__device__ __forceinline__ float scale_to_f32(uint16_t bits) {
    if (F16) return __half2float(__ushort_as_half(bits));
    return bf16_to_f32((bf16_t)bits);
}

template <int BITS>
__global__ __launch_bounds__(256) void dequantize_kernel(bf16_t* __restrict__ out, const uint32_t* __restrict__ packed,
                                                         const bf16_t* __restrict__ scales, const bf16_t* __restrict__ biases,
                                                         int64_t n_words, int group, bool scales_f16 = false, bool out_f16 = false) {
    constexpr int EPW = 32 / BITS;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t wd = packed[i];
        const int64_t g = i * EPW / group;
        const float s = scales_f16 ? scale_to_f32<true>(scales[g]) : bf16_to_f32(scales[g]);
        const float b = biases ? (scales_f16 ? scale_to_f32<true>(biases[g]) : bf16_to_f32(biases[g])) : 0.f;
        bf16_t o[EPW];
#pragma unroll
        for (int e = 0; e < EPW; ++e) {
            const float v = (float)((wd >> (e * BITS)) & ((1u << BITS) - 1u)) * s + b;
            o[e] = out_f16 ? (bf16_t)__half_as_ushort(__float2half(v)) : f32_to_bf16(v);
        }
        if (EPW == 8) *reinterpret_cast<u32x4*>(out + i * 8) = *reinterpret_cast<const u32x4*>(o);
        else *reinterpret_cast<u32x2*>(out + i * 4) = *reinterpret_cast<const u32x2*>(o);
    }
}

// any width that divides 32 and any float dtype (the result has the scales' dtype: ops/quantization.rs:118-153); one element per store
template <int BITS, int DT>
__global__ __launch_bounds__(256) void dequantize_any_kernel(typename Elem<DT>::T* __restrict__ out, const uint32_t* __restrict__ packed,
                                                             const typename Elem<DT>::T* __restrict__ scales,
                                                             const typename Elem<DT>::T* __restrict__ biases, int64_t n_words, int group) {
    constexpr int EPW = 32 / BITS;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t wd = packed[i];
        const int64_t g = i * EPW / group;
        const float sc = Elem<DT>::ld(scales + g), b = biases ? Elem<DT>::ld(biases + g) : 0.f;
#pragma unroll
        for (int e = 0; e < EPW; ++e) Elem<DT>::st(out + i * EPW + e, (float)((wd >> (e * BITS)) & ((1u << BITS) - 1u)) * sc + b);
    }
}

// 2 / 3 / 5 / 6 bits (quant_chunked): one thread per run of 32 elements = BITS words.  Each element is the expression of the 4 / 8-bit
// kernels above ((float)q * s + b, one rounding), so a q gives the same bits at every width.  bf16 / f16 out: four 16-byte stores.
template <int BITS>
__global__ __launch_bounds__(256) void dequantize_chunk_kernel(bf16_t* __restrict__ out, const uint32_t* __restrict__ packed,
                                                               const bf16_t* __restrict__ scales, const bf16_t* __restrict__ biases,
                                                               int64_t n_chunks, int group, bool scales_f16, bool out_f16) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_chunks; i += (int64_t)gridDim.x * blockDim.x) {
        uint32_t wd[BITS];
#pragma unroll
        for (int k = 0; k < BITS; ++k) wd[k] = packed[i * BITS + k];
        const int64_t g = i * 32 / group;
        const float s = scales_f16 ? scale_to_f32<true>(scales[g]) : bf16_to_f32(scales[g]);
        const float b = biases ? (scales_f16 ? scale_to_f32<true>(biases[g]) : bf16_to_f32(biases[g])) : 0.f;
        bf16_t o[32];
#pragma unroll
        for (int e = 0; e < 32; ++e) {
            const float v = (float)qfield<BITS>(wd, e) * s + b;
            o[e] = out_f16 ? (bf16_t)__half_as_ushort(__float2half(v)) : f32_to_bf16(v);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) reinterpret_cast<u32x4*>(out + i * 32)[k] = reinterpret_cast<const u32x4*>(o)[k];
    }
}

// ... any float dtype (omx_dequantize's float32 form)
template <int BITS, int DT>
__global__ __launch_bounds__(256) void dequantize_any_chunk_kernel(typename Elem<DT>::T* __restrict__ out, const uint32_t* __restrict__ packed,
                                                                   const typename Elem<DT>::T* __restrict__ scales,
                                                                   const typename Elem<DT>::T* __restrict__ biases, int64_t n_chunks, int group) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_chunks; i += (int64_t)gridDim.x * blockDim.x) {
        uint32_t wd[BITS];
#pragma unroll
        for (int k = 0; k < BITS; ++k) wd[k] = packed[i * BITS + k];
        const int64_t g = i * 32 / group;
        const float sc = Elem<DT>::ld(scales + g), b = biases ? Elem<DT>::ld(biases + g) : 0.f;
#pragma unroll
        for (int e = 0; e < 32; ++e) Elem<DT>::st(out + i * 32 + e, (float)qfield<BITS>(wd, e) * sc + b);
    }
}

// W = u32 words per lane per step; a lane's W*EPW elements lie inside one group.
// 2 / 3 / 5 / 6 bits (quant_chunked): W == BITS, a lane's chunk is 32 elements (one run of BITS words, streamed with dwordx2 / x3 / x4 + x1 /
// x4 + x2 non-temporal loads), the activations stay in natural order, and a K that is not a multiple of 64 x 32 masks the tail lanes of the
// last step.  Element pairs (q0, q1) become the bf16 pair (128 + q0, 128 + q1) by bit assembly (field_pair, quant.hpp) for the same
// v_dot2 as the 4-bit branch (nibble_pairs).
// PRO / EPI as in gemv.hip, from the same text (gemv_parts.hpp): RMSNorm prologue; store, residual add, SwiGLU
// over (gate, up) row pairs, logits + greedy-argmax partial.
// SB: scales and biases come interleaved from QMat::sb (one load per row and step instead of two)
// The kernel's text is qgemv_body.inc, which one member of a mixed-format stack (qgemv_member below) includes too.
// What each macro must expand to at an include site (a wrong expansion compiles and addresses the wrong rows):
//   QGB_BX          int expression: this block's index among the blocks that cover the QGB_N rows (4 waves x a.rows_per_wave rows each)
//   QGB_N           int expression: rows of the matrix / stack this block works on; every row index is clamped to QGB_N - 1 for loads
//                   and stores are guarded by row < QGB_N
//   QGB_GROUP       int expression: elements per scale / bias of those rows (divides a.K)
//   QGB_COL0        EMPTY, or `+ <int expression>`: spliced behind `(size_t)by * a.N` in the address of output element 0 of the rows
//                   -- the first output column of the matrix inside the launch's output row
//   QGB_FIND_MEMBER EMPTY, or one statement that turns the stack row `row` into (member index `mi`, row inside that member)
//   QGB_MEMBER      an lvalue of type const QMat: the matrix row `row` belongs to (it may use `mi`)
template <int BITS, int W, int PRO, int EPI, int RB, bool SB = false, bool F16S = false>
__global__ __launch_bounds__(256) void qgemv_kernel(const QGemvArgs a) {
    // the rows of the stack a.m[0 .. 2], written from column 0: block blockIdx.x of a.N rows in groups of a.group
#define QGB_BX blockIdx.x
#define QGB_N a.N
#define QGB_GROUP a.group
#define QGB_COL0
#define QGB_FIND_MEMBER if (row >= a.m[0].n) { row -= a.m[0].n; mi = 1; if (row >= a.m[1].n) { row -= a.m[1].n; mi = 2; } }
#define QGB_MEMBER a.m[mi]
#include "qgemv_body.inc"
#undef QGB_BX
#undef QGB_N
#undef QGB_GROUP
#undef QGB_COL0
#undef QGB_FIND_MEMBER
#undef QGB_MEMBER
}

// ... for block bx of ONE matrix M1 (n_rows rows in ITS <BITS, W> and group) whose rows start at column col0 of the launch's output row
template <int BITS, int W, int PRO, int RB, bool SB>
__device__ __forceinline__ void qgemv_member(const QGemvArgs& a, const int bx, const int n_rows, const int group, const QMat& M1, const int col0) {
    constexpr int EPI = EPI_STORE;
    constexpr bool F16S = false;
    // (macros as listed above qgemv_kernel) the n_rows rows of M1 alone, written from column col0: no member walk, `mi` unused
#define QGB_BX bx
#define QGB_N n_rows
#define QGB_GROUP group
#define QGB_COL0 +col0
#define QGB_FIND_MEMBER
#define QGB_MEMBER ((void)mi, M1)
#include "qgemv_body.inc"
#undef QGB_BX
#undef QGB_N
#undef QGB_GROUP
#undef QGB_COL0
#undef QGB_FIND_MEMBER
#undef QGB_MEMBER
}

// A q | k | v stack whose members differ in format, as ONE launch: the members' grids laid end to end, every member starting on a block
// boundary.  A block finds its member from blockIdx.x (block-uniform compares on the plan) and runs that member's <BITS, W> text on the
// member's rows in the member's group: the activation is staged per block for ONE width (stage_octet4 order at 4 bits, EPL by width),
// which is why a block serves one format.  EPI_STORE on bf16 triplets, one activation row.
struct QStackPlan {
    int first[3];     // first block of member i (INT_MAX: absent)
    int fmt[3];       // bits | W << 8
    int group[3];
    int col0[3];      // first output column of member i
};
template <int PRO, int RB, bool SB>
__global__ __launch_bounds__(256) void qgemv_stack_kernel(const QGemvArgs a, const QStackPlan p) {
    const int b = blockIdx.x;
    const int mi = b >= p.first[2] ? 2 : b >= p.first[1] ? 1 : 0;
    QMat M;
    M.w = mi == 2 ? a.m[2].w : mi == 1 ? a.m[1].w : a.m[0].w;
    M.scales = mi == 2 ? a.m[2].scales : mi == 1 ? a.m[1].scales : a.m[0].scales;
    M.biases = mi == 2 ? a.m[2].biases : mi == 1 ? a.m[1].biases : a.m[0].biases;
    M.sb = mi == 2 ? a.m[2].sb : mi == 1 ? a.m[1].sb : a.m[0].sb;
    M.n = mi == 2 ? a.m[2].n : mi == 1 ? a.m[1].n : a.m[0].n;
    const int bx = b - (mi == 2 ? p.first[2] : mi == 1 ? p.first[1] : 0);
    const int fmt = mi == 2 ? p.fmt[2] : mi == 1 ? p.fmt[1] : p.fmt[0];
    const int group = mi == 2 ? p.group[2] : mi == 1 ? p.group[1] : p.group[0];
    const int col0 = mi == 2 ? p.col0[2] : mi == 1 ? p.col0[1] : 0;
#define OMX_QSTACK_CASE(B, WW) \
    case (B | (WW << 8)): qgemv_member<B, WW, PRO, RB, SB>(a, bx, M.n, group, M, col0); break;
    switch (fmt) {
        OMX_QSTACK_CASE(2, 2) OMX_QSTACK_CASE(3, 3) OMX_QSTACK_CASE(5, 5) OMX_QSTACK_CASE(6, 6)
        OMX_QSTACK_CASE(4, 4) OMX_QSTACK_CASE(4, 2) OMX_QSTACK_CASE(4, 1) OMX_QSTACK_CASE(8, 4) OMX_QSTACK_CASE(8, 2)
    }
#undef OMX_QSTACK_CASE
}

// the (prologue, epilogue) pairs qgemv_kernel is instantiated for
static bool qgemv_form_built(int pro, int epi) {
    return (pro == PRO_NONE && (epi == EPI_STORE || epi == EPI_RESIDUAL || epi == EPI_SWIGLU || epi == EPI_F32)) ||
           (pro == PRO_RMSNORM && (epi == EPI_STORE || epi == EPI_SWIGLU || epi == EPI_ARGMAX));
}

template <int BITS, int W>
int launch_qgemv_w(const QGemvArgs& a, int pro, int epi, hipStream_t s, QGemvRoute* route) {
    constexpr int EPW = 32 / BITS;
    const int groups = (a.N + a.rows_per_wave - 1) / a.rows_per_wave;
    const dim3 grid((groups + 3) / 4, a.n_batch > 1 ? a.n_batch : 1), block(256);
    constexpr int EPL = quant_chunked(BITS) ? 32 : W * EPW;
    const size_t shmem = (size_t)a.K * 2 + (size_t)(a.K / EPL) * 4 + 64;
    // RB = logical rows per unit: 4 for long matrices, 2 when the matrix is small enough that wave count matters more
    // (rows_per_wave == RB there: one batch per wave, twice the waves) and for SwiGLU row pairs
    // interleaved scale/bias words: the engine's K % 2048 == 0 matrices (every member of the stack must carry them)
    bool sb = W == 4 || quant_chunked(BITS);
    for (int i = 0; i < 3 && sb; ++i)
        if (a.m[i].w && !a.m[i].sb) sb = false;
    if (route && qgemv_form_built(pro, epi)) {
        route->kernel = 1; route->bits = BITS; route->W = W; route->RB = (epi == EPI_SWIGLU || a.rows_per_wave == 2) ? 2 : 4;
        route->rows_per_wave = a.rows_per_wave; route->SB = sb; route->F16S = a.scales_f16 != 0;
        route->blocks = (int)grid.x; route->lds_bytes = (int)shmem; route->KS = route->NU = route->NBUF = 0;
        if (route->dry_run) return 0;
    }
#define OMX_QGEMV_LAUNCH(P, E, SBF, F16)                                                       \
    {                                                                                         \
        if (E == EPI_SWIGLU || a.rows_per_wave == 2) OMX_LAUNCH((qgemv_kernel<BITS, W, P, E, 2, SBF, F16>), grid, block, shmem, s, a); \
        else OMX_LAUNCH((qgemv_kernel<BITS, W, P, E, 4, SBF, F16>), grid, block, shmem, s, a);          \
        OMX_LAUNCH_CHECK();                                                                   \
        return 0;                                                                             \
    }
#define OMX_QGEMV_CASE(P, E)                                                                  \
    if (pro == P && epi == E) {                                                               \
        if constexpr (W == 4 || quant_chunked(BITS)) {                                        \
            if (sb) {                                                                         \
                if (a.scales_f16) OMX_QGEMV_LAUNCH(P, E, true, true)                          \
                OMX_QGEMV_LAUNCH(P, E, true, false)                                           \
            }                                                                                 \
        }                                                                                     \
        if (a.scales_f16) OMX_QGEMV_LAUNCH(P, E, false, true)                                 \
        OMX_QGEMV_LAUNCH(P, E, false, false)                                                  \
    }
    OMX_QGEMV_CASE(PRO_NONE, EPI_STORE)
    OMX_QGEMV_CASE(PRO_RMSNORM, EPI_STORE)
    OMX_QGEMV_CASE(PRO_NONE, EPI_RESIDUAL)
    OMX_QGEMV_CASE(PRO_RMSNORM, EPI_SWIGLU)
    OMX_QGEMV_CASE(PRO_NONE, EPI_SWIGLU)
    OMX_QGEMV_CASE(PRO_RMSNORM, EPI_ARGMAX)
    OMX_QGEMV_CASE(PRO_NONE, EPI_F32)
#undef OMX_QGEMV_CASE
#undef OMX_QGEMV_LAUNCH
    return set_error("quantized gemv: unsupported prologue/epilogue combination %d/%d", pro, epi);
}

// words per lane and step of the non-chunked widths (4 / 8 bits) for a row of K elements in groups of `group`: the widest of 4, 2, 1 whose
// lane chunk divides K / 64 and lies inside one group; 0: none (a chunked width streams BITS words).  With it the lane's chunk -- and so
// the order of every row's sums -- is a function of the matrix's own (bits, group, K) alone.
int qgemv_words(int bits, int K, int group) {
    if (quant_chunked(bits)) return (K > 0 && K % 32 == 0 && group >= 32) ? bits : 0;
    const int EPW = 32 / bits;
    int W = 4;
    while (W * EPW > 8 && (K % (64 * W * EPW) != 0 || W * EPW > group)) W >>= 1;
    return (K % (64 * W * EPW) == 0 && W * EPW <= group && W * EPW >= 8) ? W : 0;
}

// rows per wave of a launch over N logical rows: long streams for the vocabulary matrix, one batch per wave otherwise; small matrices:
// two rows per wave -- and the tuning knobs that override it.  An EPI_ARGMAX launch takes no knob: its block count is the number of
// partial keys the engines sized their slots for and reduce (qgemv_grid, which sees neither K nor the environment) -- with
// OMX_QGEMV_RPW_SMALL=4 a vocabulary of N <= 8192 wrote half of them and the reduction read the rest as they were left
int qgemv_default_rpw(int N, int epi) { return N >= 65536 ? 16 : (N <= 8192 && epi != EPI_SWIGLU) ? 2 : 4; }
int qgemv_rows_per_wave(int N, int K, int epi) {
    int rpw = qgemv_default_rpw(N, epi);
    if (epi == EPI_ARGMAX) return rpw;
    if (const char* e = getenv("OMX_QGEMV_RPW_SMALL"))   // tuning knob: rows per wave of the small matrices (2 or 4)
        if (N <= 8192 && epi != EPI_SWIGLU && (atoi(e) == 2 || atoi(e) == 4)) rpw = atoi(e);
    if (const char* e = getenv("OMX_QGEMV_RPW_LONGK"))   // ... of the small matrices with a long row (K > 8192: the down projection)
        if (N <= 8192 && K > 8192 && epi != EPI_SWIGLU && (atoi(e) == 2 || atoi(e) == 4 || atoi(e) == 8)) rpw = atoi(e);
    if (const char* e = getenv("OMX_QGEMV_RPW_GU"))      // ... of the gate/up pair launch (logical rows: 2, 4, 8)
        if (epi == EPI_SWIGLU && N < 65536 && (atoi(e) == 2 || atoi(e) == 4 || atoi(e) == 8)) rpw = atoi(e);
    return rpw;
}

template <int BITS>
int launch_qgemv_bits(const QGemvArgs& a_in, int pro, int epi, hipStream_t s, QGemvRoute* route) {
    QGemvArgs a = a_in;
    const int W = qgemv_words(BITS, a.K, a.group);
    if constexpr (quant_chunked(BITS)) {
        OMX_REQUIRE(W != 0, "quantized_matmul: K=%d unsupported for %d-bit group %d", a.K, BITS, a.group);
    } else {
        // (the narrowest lane chunk is 8 elements -- one 16-byte activation vector -- at either width: 64 lanes x 8)
        OMX_REQUIRE(W != 0, "quantized_matmul: K=%d unsupported for %d-bit group %d (K must be a multiple of %d)",
                    a.K, BITS, a.group, 64 * 8);
    }
    if (a.n_batch < 1) a.n_batch = 1;
    if (a.x_div < 1) a.x_div = 1;
    a.rows_per_wave = qgemv_rows_per_wave(a.N, a.K, epi);
    if (const char* e = getenv("OMX_QGEMV_ROLLED_STAGE")) a.rolled_stage = e[0] == '1';
    if constexpr (quant_chunked(BITS)) {
        return launch_qgemv_w<BITS, BITS>(a, pro, epi, s, route);
    } else {
        if (W == 4) return launch_qgemv_w<BITS, 4>(a, pro, epi, s, route);
        if (W == 2) return launch_qgemv_w<BITS, 2>(a, pro, epi, s, route);
        if constexpr (BITS == 4) return launch_qgemv_w<BITS, 1>(a, pro, epi, s, route);
        return set_error("quantized gemv: K=%d too small for %d-bit weights", a.K, BITS);
    }
}

// quantize / dequantize alone take what mlx_rs::ops::quantize takes: MLX's affine widths 2, 3, 4, 5, 6 and 8 on bfloat16 / float16 /
// float32 (the reference's own value test loops [2, 4, 8] on float32: ops/quantization.rs:289-305)
int check_format_qdq(const char* who, int K, int group, int bits, int dtype) {
    OMX_REQUIRE(dtype == OMX_BFLOAT16 || dtype == OMX_FLOAT16 || dtype == OMX_FLOAT32, "%s: bf16 / f16 / f32 only (got dtype %d)", who, dtype);
    OMX_REQUIRE(quant_bits_ok(bits), "%s: bits must be 2, 3, 4, 5, 6 or 8 (got %d)", who, bits);
    OMX_REQUIRE(group == 32 || group == 64 || group == 128, "%s: group_size must be 32, 64 or 128 (got %d)", who, group);
    OMX_REQUIRE(K > 0 && K % group == 0, "%s: the last dimension (%d) must be divisible by the group size (%d)", who, K, group);
    return 0;
}

// dtype: OMX_BFLOAT16, or OMX_FLOAT16 where `f16_scales_ok` -- scales / biases of a float16 checkpoint (activations stay bf16)
int check_format(const char* who, int K, int group, int bits, int dtype, bool f16_scales_ok = false) {
    OMX_REQUIRE(dtype == OMX_BFLOAT16 || (f16_scales_ok && dtype == OMX_FLOAT16), "%s: bf16 activations / scales only (got dtype %d)", who, dtype);
    OMX_REQUIRE(quant_bits_ok(bits), "%s: bits must be 2, 3, 4, 5, 6 or 8 (got %d)", who, bits);
    OMX_REQUIRE(group == 32 || group == 64 || group == 128, "%s: group_size must be 32, 64 or 128 (got %d)", who, group);
    OMX_REQUIRE(K > 0 && K % group == 0, "%s: the last dimension (%d) must be divisible by the group size (%d)", who, K, group);
    return 0;
}

}  // namespace

namespace {
__global__ __launch_bounds__(256) void quant_interleave_kernel(uint32_t* __restrict__ sb, const bf16_t* __restrict__ scales,
                                                               const bf16_t* __restrict__ biases, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        sb[i] = (uint32_t)scales[i] | ((uint32_t)(biases ? biases[i] : (bf16_t)0) << 16);
}
}  // namespace

int launch_quant_interleave(uint32_t* sb, const bf16_t* scales, const bf16_t* biases, size_t n_groups, hipStream_t s) {
    OMX_REQUIRE(sb && scales, "quant interleave: null tensor");
    if (n_groups == 0) return 0;
    quant_interleave_kernel<<<(unsigned)std::min<size_t>((n_groups + 255) / 256, 4096), 256, 0, s>>>(sb, scales, biases, n_groups);
    OMX_LAUNCH_CHECK();
    return 0;
}

namespace {
std::mutex g_sb_mu;
std::unordered_map<const void*, const uint32_t*> g_sb_of_scales;
}  // namespace
void quant_register_sb(const bf16_t* scales, const uint32_t* sb) {
    std::lock_guard<std::mutex> lk(g_sb_mu);
    g_sb_of_scales[scales] = sb;
}
void quant_unregister_sb(const bf16_t* scales) {
    std::lock_guard<std::mutex> lk(g_sb_mu);
    g_sb_of_scales.erase(scales);
}
const uint32_t* quant_find_sb(const bf16_t* scales) {
    std::lock_guard<std::mutex> lk(g_sb_mu);
    auto it = g_sb_of_scales.find(scales);
    return it == g_sb_of_scales.end() ? nullptr : it->second;
}

int qgemv_grid(int N) {
    const int rpw = qgemv_default_rpw(N, EPI_ARGMAX);
    return ((N + rpw - 1) / rpw + 3) / 4;
}

// the q | k | v stack with members of different formats as ONE launch (qgemv_stack_kernel); fb / fg: the members' bits / groups
static int launch_qgemv_stack(const QGemvArgs& a_in, const int* fb, const int* fg, int pro, hipStream_t s, QGemvRoute* route) {
    QGemvArgs a = a_in;
    a.rows_per_wave = qgemv_rows_per_wave(a.N, a.K, EPI_STORE);
    if (const char* e = getenv("OMX_QGEMV_ROLLED_STAGE")) a.rolled_stage = e[0] == '1';
    a.n_batch = 1; a.x_div = 1;
    QStackPlan p = {};
    int blocks = 0, col = 0, min_epl = 64;
    bool sb = true;
    for (int i = 0; i < 3; ++i) {
        p.first[i] = INT_MAX;
        if (!a.m[i].w) continue;
        OMX_REQUIRE(i == 0 || a.m[i - 1].w, "quantized gemv: the members of a stack are m[0], m[1], m[2] in order");
        const int W = qgemv_words(fb[i], a.K, fg[i]);
        OMX_REQUIRE(W != 0, "quantized gemv: K=%d unsupported for %d-bit group %d (member %d of a mixed stack)", a.K, fb[i], fg[i], i);
        p.first[i] = blocks; p.fmt[i] = fb[i] | (W << 8); p.group[i] = fg[i]; p.col0[i] = col;
        blocks += ((a.m[i].n + a.rows_per_wave - 1) / a.rows_per_wave + 3) / 4;
        col += a.m[i].n;
        min_epl = std::min(min_epl, quant_chunked(fb[i]) ? 32 : W * (32 / fb[i]));
        if (!a.m[i].sb) sb = false;
    }
    OMX_REQUIRE(col == a.N && blocks > 0, "quantized gemv: the stack's members hold %d rows, N = %d", col, a.N);
    const size_t shmem = (size_t)a.K * 2 + (size_t)(a.K / min_epl) * 4 + 64;
    const dim3 grid(blocks), block(256);
    if (route && (pro == PRO_NONE || pro == PRO_RMSNORM)) {
        route->kernel = 2; route->bits = 0; route->W = 0; route->RB = a.rows_per_wave == 2 ? 2 : 4; route->rows_per_wave = a.rows_per_wave;
        route->SB = sb; route->F16S = 0; route->blocks = blocks; route->lds_bytes = (int)shmem; route->KS = route->NU = route->NBUF = 0;
        if (route->dry_run) return 0;
    }
#define OMX_QSTACK_LAUNCH(P)                                                                                        \
    if (pro == P) {                                                                                                 \
        if (a.rows_per_wave == 2) {                                                                                 \
            if (sb) OMX_LAUNCH((qgemv_stack_kernel<P, 2, true>), grid, block, shmem, s, a, p);                      \
            else OMX_LAUNCH((qgemv_stack_kernel<P, 2, false>), grid, block, shmem, s, a, p);                        \
        } else {                                                                                                    \
            if (sb) OMX_LAUNCH((qgemv_stack_kernel<P, 4, true>), grid, block, shmem, s, a, p);                      \
            else OMX_LAUNCH((qgemv_stack_kernel<P, 4, false>), grid, block, shmem, s, a, p);                        \
        }                                                                                                           \
        OMX_LAUNCH_CHECK();                                                                                         \
        return 0;                                                                                                   \
    }
    OMX_QSTACK_LAUNCH(PRO_NONE)
    OMX_QSTACK_LAUNCH(PRO_RMSNORM)
#undef OMX_QSTACK_LAUNCH
    return set_error("quantized gemv: unsupported prologue %d for a stack of mixed formats", pro);
}

int launch_qgemv(const QGemvArgs& a_in, int bits, int pro, int epi, hipStream_t s, QGemvRoute* route) {
    // the format each member runs in: its own where it carries one, else the launch's
    int fb[3] = {0, 0, 0}, fg[3] = {0, 0, 0}, first = -1;
    bool mixed = false;
    for (int i = 0; i < 3; ++i) {
        if (!a_in.m[i].w) continue;
        fb[i] = qmat_bits(a_in.m[i], bits); fg[i] = qmat_group(a_in.m[i], a_in.group);
        if (first < 0) first = i;
        else if (fb[i] != fb[first] || fg[i] != fg[first]) mixed = true;
    }
    if (mixed) {
        OMX_REQUIRE(epi != EPI_SWIGLU, "quantized gemv: gate (%d-bit group %d) and up (%d-bit group %d) must share a format", fb[0], fg[0], fb[1], fg[1]);
        OMX_REQUIRE(epi == EPI_STORE && !a_in.scales_f16 && a_in.n_batch <= 1 && !a_in.w_sel && a_in.w_sel_n == 0,
                    "quantized gemv: a stack of mixed formats is a plain store of one activation row on bf16 triplets");
        for (int i = 0; i < 3; ++i)
            if (a_in.m[i].w) {
                OMX_REQUIRE(quant_bits_ok(fb[i]), "quantized gemv: bits must be 2, 3, 4, 5, 6 or 8 (got %d)", fb[i]);
                OMX_REQUIRE(fg[i] == 32 || fg[i] == 64 || fg[i] == 128, "quantized gemv: group_size must be 32, 64 or 128 (got %d)", fg[i]);
                OMX_REQUIRE(a_in.K > 0 && a_in.K % fg[i] == 0, "quantized gemv: the row width (%d) must be divisible by the group size (%d)", a_in.K, fg[i]);
            }
        return launch_qgemv_stack(a_in, fb, fg, pro, s, route);
    }
    QGemvArgs a = a_in;
    if (first >= 0) { bits = fb[first]; a.group = fg[first]; }
    OMX_REQUIRE(quant_bits_ok(bits), "quantized gemv: bits must be 2, 3, 4, 5, 6 or 8 (got %d)", bits);
    if (bits == 4) {
        const int r = launch_qgemv4m(a, pro, epi, s, route);
        if (r >= 0) return r;
    }
    switch (bits) {
    case 2: return launch_qgemv_bits<2>(a, pro, epi, s, route);
    case 3: return launch_qgemv_bits<3>(a, pro, epi, s, route);
    case 5: return launch_qgemv_bits<5>(a, pro, epi, s, route);
    case 6: return launch_qgemv_bits<6>(a, pro, epi, s, route);
    default: return bits == 4 ? launch_qgemv_bits<4>(a, pro, epi, s, route) : launch_qgemv_bits<8>(a, pro, epi, s, route);
    }
}

}  // namespace omx

using namespace omx;

extern "C" int omx_quantize(void* packed, void* scales, void* biases, const void* w, int64_t rows, int cols, int group_size,
                            int bits, omx_dtype dtype, omx_stream stream) {
    OMX_REQUIRE(packed && scales && biases && w, "omx_quantize: null tensor");
    if (check_format_qdq("omx_quantize", cols, group_size, bits, dtype)) return 1;
    const int64_t n_groups = rows * (cols / group_size);
    if (n_groups == 0) return 0;
    const unsigned blocks = (unsigned)((n_groups + 3) / 4);
#define OMX_Q_CASE(B, D)                                                                                                     \
    if (bits == B && dtype == D) {                                                                                           \
        typedef Elem<D>::T T;                                                                                                \
        quantize_kernel<B, D><<<blocks, 256, 0, (hipStream_t)stream>>>((uint32_t*)packed, (T*)scales, (T*)biases, (const T*)w, n_groups, group_size); \
    }
    OMX_Q_CASE(2, OMX_BFLOAT16) OMX_Q_CASE(4, OMX_BFLOAT16) OMX_Q_CASE(8, OMX_BFLOAT16)
    OMX_Q_CASE(2, OMX_FLOAT16) OMX_Q_CASE(4, OMX_FLOAT16) OMX_Q_CASE(8, OMX_FLOAT16)
    OMX_Q_CASE(2, OMX_FLOAT32) OMX_Q_CASE(4, OMX_FLOAT32) OMX_Q_CASE(8, OMX_FLOAT32)
    OMX_Q_CASE(3, OMX_BFLOAT16) OMX_Q_CASE(5, OMX_BFLOAT16) OMX_Q_CASE(6, OMX_BFLOAT16)
    OMX_Q_CASE(3, OMX_FLOAT16) OMX_Q_CASE(5, OMX_FLOAT16) OMX_Q_CASE(6, OMX_FLOAT16)
    OMX_Q_CASE(3, OMX_FLOAT32) OMX_Q_CASE(5, OMX_FLOAT32) OMX_Q_CASE(6, OMX_FLOAT32)
#undef OMX_Q_CASE
    OMX_LAUNCH_CHECK();
    return 0;
}

static int launch_dequantize_any(void* out, const uint32_t* packed, const void* scales, const void* biases, int64_t rows, int cols,
                                 int group_size, int bits, bool scales_f16, bool out_f16, hipStream_t s) {
    OMX_REQUIRE(out && packed && scales, "omx_dequantize: null tensor");
    if (quant_chunked(bits)) {
        const int64_t n_chunks = rows * cols / 32;
        if (n_chunks == 0) return 0;
        const unsigned blocks = (unsigned)((n_chunks + 255) / 256 < 16384 ? (n_chunks + 255) / 256 : 16384);
#define OMX_DQC_CASE(B)                                                                                                         \
        if (bits == B) dequantize_chunk_kernel<B><<<blocks, 256, 0, s>>>((bf16_t*)out, packed, (const bf16_t*)scales, (const bf16_t*)biases, \
                                                                          n_chunks, group_size, scales_f16, out_f16);
        OMX_DQC_CASE(2) OMX_DQC_CASE(3) OMX_DQC_CASE(5) OMX_DQC_CASE(6)
#undef OMX_DQC_CASE
        OMX_LAUNCH_CHECK();
        return 0;
    }
    OMX_REQUIRE(bits == 4 || bits == 8, "dequantize: bits must be 2, 3, 4, 5, 6 or 8 (got %d)", bits);
    const int64_t n_words = rows * cols * bits / 32;
    if (n_words == 0) return 0;
    const unsigned blocks = (unsigned)((n_words + 255) / 256 < 16384 ? (n_words + 255) / 256 : 16384);
    if (bits == 4) dequantize_kernel<4><<<blocks, 256, 0, s>>>((bf16_t*)out, packed, (const bf16_t*)scales, (const bf16_t*)biases, n_words, group_size, scales_f16, out_f16);
    else dequantize_kernel<8><<<blocks, 256, 0, s>>>((bf16_t*)out, packed, (const bf16_t*)scales, (const bf16_t*)biases, n_words, group_size, scales_f16, out_f16);
    OMX_LAUNCH_CHECK();
    return 0;
}
int omx::launch_dequantize_bf16(bf16_t* out, const uint32_t* packed, const void* scales, const void* biases, int64_t rows, int cols,
                                int group_size, int bits, bool scales_f16, hipStream_t s, bool out_f16) {
    return launch_dequantize_any(out, packed, scales, biases, rows, cols, group_size, bits, scales_f16, out_f16, s);
}

/* mlx_rs::ops::dequantize (ops/quantization.rs:118-153): the result has the dtype of scales / biases -- OMX_BFLOAT16, or OMX_FLOAT16 for
 * a float16 checkpoint's triplets (each element one fma in float32 from the exact scale / bias, one rounding) */
extern "C" int omx_dequantize(void* out, const void* packed, const void* scales, const void* biases, int64_t rows, int cols,
                              int group_size, int bits, omx_dtype dtype, omx_stream stream) {
    OMX_REQUIRE(out && packed && scales, "omx_dequantize: null tensor");
    if (check_format_qdq("omx_dequantize", cols, group_size, bits, dtype)) return 1;
    if (bits != 2 && dtype != OMX_FLOAT32) {   // the 16-bit forms the matmul paths share (vector stores)
        const bool f16 = dtype == OMX_FLOAT16;
        return launch_dequantize_any(out, (const uint32_t*)packed, scales, biases, rows, cols, group_size, bits, f16, f16, (hipStream_t)stream);
    }
    if (bits != 2 && quant_chunked(bits)) {   // 3 / 5 / 6 bits, float32 out
        const int64_t n_chunks = rows * cols / 32;
        if (n_chunks == 0) return 0;
        const unsigned blocks = (unsigned)((n_chunks + 255) / 256 < 16384 ? (n_chunks + 255) / 256 : 16384);
        if (bits == 3) dequantize_any_chunk_kernel<3, OMX_FLOAT32><<<blocks, 256, 0, (hipStream_t)stream>>>((float*)out, (const uint32_t*)packed, (const float*)scales, (const float*)biases, n_chunks, group_size);
        if (bits == 5) dequantize_any_chunk_kernel<5, OMX_FLOAT32><<<blocks, 256, 0, (hipStream_t)stream>>>((float*)out, (const uint32_t*)packed, (const float*)scales, (const float*)biases, n_chunks, group_size);
        if (bits == 6) dequantize_any_chunk_kernel<6, OMX_FLOAT32><<<blocks, 256, 0, (hipStream_t)stream>>>((float*)out, (const uint32_t*)packed, (const float*)scales, (const float*)biases, n_chunks, group_size);
        OMX_LAUNCH_CHECK();
        return 0;
    }
    const int64_t n_words = rows * cols * bits / 32;
    if (n_words == 0) return 0;
    const unsigned blocks = (unsigned)((n_words + 255) / 256 < 16384 ? (n_words + 255) / 256 : 16384);
#define OMX_DQ_CASE(B, D)                                                                                                    \
    if (bits == B && dtype == D) {                                                                                           \
        typedef Elem<D>::T T;                                                                                                \
        dequantize_any_kernel<B, D><<<blocks, 256, 0, (hipStream_t)stream>>>((T*)out, (const uint32_t*)packed, (const T*)scales, (const T*)biases, n_words, group_size); \
    }
    OMX_DQ_CASE(2, OMX_BFLOAT16) OMX_DQ_CASE(2, OMX_FLOAT16) OMX_DQ_CASE(2, OMX_FLOAT32) OMX_DQ_CASE(4, OMX_FLOAT32) OMX_DQ_CASE(8, OMX_FLOAT32)
#undef OMX_DQ_CASE
    OMX_LAUNCH_CHECK();
    return 0;
}

/* out [M, N] = x [M, K] . dequant(W [N, K])^T   (nn::QuantizedLinear::forward, quantized.rs:366-375) */
extern "C" int omx_quantized_matmul(void* out, const void* x, const void* packed, const void* scales, const void* biases, int M,
                                    int N, int K, int group_size, int bits, omx_dtype dtype, omx_stream stream) {
    OMX_REQUIRE(out && x && packed && scales, "omx_quantized_matmul: null tensor");
    // dtype = the dtype of x, out, scales and biases alike: bfloat16, or float16 (a float16 MLX checkpoint runs in float16 end to end)
    if (check_format("omx_quantized_matmul", K, group_size, bits, dtype, true)) return 1;
    OMX_REQUIRE(M >= 0 && N > 0, "omx_quantized_matmul: bad shape");
    if (M == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == OMX_FLOAT16 && !(M <= 16 && K % 512 == 0)) {
        // many float16 rows: weights dequantised to float16 (one fma + one rounding per element, like MLX's qmm tile), both operands widened
        // to float32 and multiplied on the f32 matrix cores (exact products of float16 values, f32 accumulation), one rounding to float16
        void* ws = nullptr;
        const size_t nw = (size_t)N * K, nx = (size_t)M * K, no = (size_t)M * N;
        if (get_workspace(&ws, nw * 2 + (nw + nx + no) * 4 + 1024)) return 1;
        char* p = (char*)ws;
        f16_t* w16 = (f16_t*)p; p += (nw * 2 + 255) & ~(size_t)255;
        float* w32 = (float*)p; p += nw * 4;
        float* x32 = (float*)p; p += nx * 4;
        float* o32 = (float*)p;
        if (launch_dequantize_any(w16, (const uint32_t*)packed, scales, biases, N, K, group_size, bits, true, true, s)) return 1;
        if (omx_cast(w32, OMX_FLOAT32, w16, OMX_FLOAT16, (int64_t)nw, stream) || omx_cast(x32, OMX_FLOAT32, x, OMX_FLOAT16, (int64_t)nx, stream)) return 1;
        GemmF32 g = {};
        g.a = x32; g.b = w32; g.out = o32; g.M = M; g.N = N; g.K = K; g.lda = K; g.ldb = K; g.ldc = N; g.batch = 1; g.alpha = 1.0f;
        if (launch_gemm_f32(g, s)) return 1;
        return omx_cast(out, OMX_FLOAT16, o32, OMX_FLOAT32, (int64_t)no, stream);
    }
    if (M <= 16 && K % 512 == 0) {
        QGemvArgs a = {};
        a.m[0] = QMat{(const uint32_t*)packed, (const bf16_t*)scales, (const bf16_t*)biases, N};
        a.x = (const bf16_t*)x; a.out = (bf16_t*)out; a.N = N; a.K = K; a.group = group_size;
        a.n_batch = M; a.x_div = 1; a.scales_f16 = dtype == OMX_FLOAT16;
        return launch_qgemv(a, bits, PRO_NONE, EPI_STORE, s);
    }
    void* ws = nullptr;
    if (get_workspace(&ws, (size_t)N * K * 2)) return 1;
    if (launch_dequantize_bf16((bf16_t*)ws, (const uint32_t*)packed, scales, biases, N, K, group_size, bits, dtype == OMX_FLOAT16, s)) return 1;
    return launch_gemm_bf16((bf16_t*)out, (const bf16_t*)x, (const bf16_t*)ws, nullptr, M, N, K, s);
}

/* out [n, N] = x [n / x_div, K] . dequant(W[rhs_indices[i]])^T : SwitchLinear on expert-stacked quantized weights
 * (mixtral-mlx/src/model.rs:195-201 -> gather_qmm, ops/quantization.rs:226-279); packed [E, N, K*bits/32] */
extern "C" int omx_gather_qmm(void* out, const void* x, const void* packed, const void* scales, const void* biases,
                              const uint32_t* rhs_indices, int n_rows, int x_div, int N, int K, int n_experts, int group_size,
                              int bits, omx_dtype dtype, omx_stream stream) {
    OMX_REQUIRE(out && x && packed && scales && rhs_indices, "omx_gather_qmm: null tensor");
    if (check_format("omx_gather_qmm", K, group_size, bits, dtype, true)) return 1;
    OMX_REQUIRE(n_rows >= 0 && x_div >= 1 && N > 0 && n_experts >= 1, "omx_gather_qmm: bad shape");
    OMX_REQUIRE(K % 512 == 0, "omx_gather_qmm: K=%d must be a multiple of 512", K);
    if (n_rows == 0) return 0;
    QGemvArgs a = {};
    a.m[0] = QMat{(const uint32_t*)packed, (const bf16_t*)scales, (const bf16_t*)biases, N};
    a.x = (const bf16_t*)x; a.out = (bf16_t*)out; a.N = N; a.K = K; a.group = group_size;
    a.n_batch = n_rows; a.x_div = x_div; a.w_sel = rhs_indices; a.scales_f16 = dtype == OMX_FLOAT16;
    a.w_estride = (size_t)N * K * bits / 32; a.s_estride = (size_t)N * (K / group_size);
    return launch_qgemv(a, bits, PRO_NONE, EPI_STORE, (hipStream_t)stream);
}
