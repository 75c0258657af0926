// bf16 activations x MLX-packed weights (4 / 8-bit affine, quant.hip for the format) on the gfx950 matrix cores:
//   out[M, N] = x[M, K] . dequant(W)^T      (nn::QuantizedLinear::forward, mlx-rs/src/nn/quantized.rs:361-385)
// for the quantized FLUX.2-klein DiT (flux-klein-mlx/src/klein_quantized.rs) at M > 16, where the packed GEMV (quant.hip) is
// the wrong shape class and the older route -- dequantise the whole matrix into a bf16 workspace, then the bf16 GEMM -- writes and
// re-reads a bf16 copy of every matrix per step.  Here W never exists in HBM as bf16:
//
//   * 256 (or 128) x 256 x 64 tile, 512 threads = 8 waves as 2 (M) x 4 (N), a wave owns (TMR / 2) x 64 of the output as 16 x 16
//     tiles of v_mfma_f32_16x16x32_bf16, one f32 accumulator per output element, k ascending from 0, no split-K: every output
//     element is the same MFMA chain as in the bf16 kernels of the 16x16x32 family (gemm.hip: the eight-wave 256^2 kernel with
//     MF = 16, the four-wave tile, the 64^2 ring kernel), so  qgemm(x, W) == gemm_bf16(x, omx_dequantize(W))  bit for bit;
//   * A (activations): global_load_lds straight into LDS, two buffers, the source-side 16-byte-chunk swizzle kc ^ (row & 7)
//     that lds_frag undoes -- as the bf16 kernels stage it;
//   * B (weights): thread t owns tile column t >> 1 and 32 k of the 64-k step: BITS packed words (32 B at 8-bit, 16 B at 4-bit)
//     and ONE scale and ONE bias load (a 32-aligned run of 32 k lies inside one group).  The words of tile t+2 are loaded into
//     VGPRs before the MFMAs of tile t; between the two 32-k halves of those MFMAs every thread dequantises tile t+1's 32 elements with
//     dequantize_kernel's expression (f32 q * s + b, one RNE rounding to bf16) and writes them into the other B buffer in the
//     same swizzled layout, so the VALU work issues while the matrix core runs the first half;
//   * two tiles in flight (three A buffers, two B buffers, two register sets of packed words: 160 KiB of LDS at 256 rows), one barrier
//     per 64-k step (A of tile t+1 landed, B of tile t+1 written, the buffers of tile t free);
//   * epilogues: plain store; the DiT's gated residual bf16(resid + acc * gate[col]); the segmented SwiGLU form of
//     launch_gemm_bf16_swiglu (n_plain plain columns, then column tiles of 128 gate + the matching 128 up rows, fused_swiglu);
//   * XCD-aware block order and 8-row-tile grouping of gemm_bf16_nt_256_kernel; TMR = 128 under gemm_tile_hint(128) (a GEMM that
//     shares the chip with another stream's grid) and for grids whose 256-row tiles would cover less than the chip.
// No workspace: two launches on two streams share nothing.
#include <mutex>

#include "gemm.hpp"
#include "qgemm.hpp"

namespace omx {
namespace {

typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef const __attribute__((address_space(1))) void* glb_ptr_t;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;

constexpr int NT = 512, TK = 64, TN = 256;
constexpr int B_BYTES = TN * TK * 2;                                   // 32 KiB per B buffer
constexpr int smem_bytes(int tmr) { return 3 * (tmr * TK * 2) + 2 * B_BYTES; }   // three A buffers, two B buffers (160 KiB at 256 rows)

struct QArgs {
    const bf16_t* x;          // [M, K]
    const uint32_t* w;        // [rows, K * BITS / 32]
    const bf16_t* scales;     // [rows, K / group]
    const bf16_t* biases;     // [rows, K / group] or null
    bf16_t* out;              // plain columns, row stride ld_out
    const bf16_t* resid;      // gated form: [M, n_plain]
    const bf16_t* gate;       // gated form: [n_plain]
    bf16_t* out_act;          // SwiGLU outputs, row stride ld_act
    int M, K, group;
    int n_plain, ld_out;      // plain columns (the plain form: N)
    int half, ld_act;         // SwiGLU pairs (0: none)
    int act_tile0;            // first SwiGLU column tile
    int grid_m, grid_n;
};

__device__ __forceinline__ bf16x8 lds_frag(const unsigned char* lds_tile, int row, int kc) {
    return *reinterpret_cast<const bf16x8*>(lds_tile + ((row << 3) + (kc ^ (row & 7))) * 16);
}

template <int BITS, int TMR>
__global__ __launch_bounds__(NT) void qgemm_kernel(const QArgs a) {
    static_assert(BITS == 4 || BITS == 8, "4- or 8-bit packings");
    static_assert(TMR == 256 || TMR == 128, "256- or 128-row tiles");
    constexpr int WM = TMR / 2;            // rows per wave
    constexpr int RT = WM / 16, CT = 4;    // 16 x 16 accumulator tiles per wave
    constexpr int A_BYTES = TMR * TK * 2;
    constexpr int NA = TMR * 8 / NT;       // 16-byte A chunks per thread and tile
    constexpr int EPW = 32 / BITS;         // elements per packed word
    constexpr int WPT = 32 / EPW;          // packed words per thread and tile (32 elements)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // [A0 | A1 | A2 | B0 | B1]
    auto bufA = [&](int i) { return smem + i * A_BYTES; };
    auto bufB = [&](int i) { return smem + 3 * A_BYTES + i * B_BYTES; };
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 2, wc = wave & 3;

    // XCD-aware remap (bijective), then 8 row tiles x all column tiles per group (gemm_bf16_nt_256_kernel)
    const int nblk = a.grid_m * a.grid_n;
    int bid = blockIdx.x;
    {
        const int q = nblk / 8, r = nblk % 8, xcd = bid % 8, idx = bid / 8;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    int tm, tn;
    {
        constexpr int GM = 8;
        const int per_group = GM * a.grid_n;
        const int group = bid / per_group, in_group = bid % per_group;
        const int first_m = group * GM;
        const int gm = min(a.grid_m - first_m, GM);
        tm = first_m + in_group % gm;
        tn = in_group / gm;
    }
    const int m0 = tm * TMR;
    const bool act = tn >= a.act_tile0;
    const int n0 = act ? (tn - a.act_tile0) * 128 : tn * TN;   // first output column of the tile (act: first SwiGLU output)

    // A sources: chunk c = i * 512 + tid lands at LDS chunk c; it carries logical chunk (c & 7) ^ (row & 7) of row c >> 3
    const bf16_t* srcA[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int c = i * NT + tid, row = c >> 3, kc = (c & 7) ^ (row & 7);
        srcA[i] = a.x + (size_t)min(m0 + row, a.M - 1) * a.K + kc * 8;
    }
    auto stage_a = [&](int t, unsigned char* buf) {
#pragma unroll
        for (int i = 0; i < NA; ++i)
            __builtin_amdgcn_global_load_lds((glb_ptr_t)(srcA[i] + t * TK), (lds_ptr_t)(buf + (i * NT + wave * 64) * 16), 16, 0, 0);
    };

    // B: tile column bn, k half hk.  SwiGLU tiles: columns wc * 64 + [0, 32) are gate rows, wc * 64 + [32, 64) the up rows of the
    // same 32 outputs (the layout of the bf16 segmented kernel), so a lane's accumulators j and j + 2 are one output's pair.
    const int bn = tid >> 1, hk = tid & 1;
    int wrow;
    if (act) {
        const int w = bn & 63, oc = min(n0 + (bn >> 6) * 32 + (w & 31), a.half - 1);
        wrow = a.n_plain + oc + (w >= 32 ? a.half : 0);
    } else {
        wrow = min(n0 + bn, a.n_plain - 1);
    }
    const int ng = a.K / a.group;
    const uint32_t* srcW = a.w + (size_t)wrow * (a.K / EPW) + hk * WPT;
    const bf16_t* srcS = a.scales + (size_t)wrow * ng;
    const bf16_t* srcB = a.biases ? a.biases + (size_t)wrow * ng : nullptr;
    struct PReg { uint32_t w[WPT]; bf16_t s, b; };   // one tile's packed words, scale and bias of this thread
    auto load_b = [&](int t, PReg& p) {
#pragma unroll
        for (int v = 0; v < WPT / 4; ++v) {
            const u32x4 q = *reinterpret_cast<const u32x4*>(srcW + t * (2 * WPT) + 4 * v);
#pragma unroll
            for (int e = 0; e < 4; ++e) p.w[4 * v + e] = q[e];
        }
        const int g = (t * TK + hk * 32) / a.group;
        p.s = srcS[g];
        p.b = srcB ? srcB[g] : (bf16_t)0;
    };
    // dequantize_kernel's arithmetic: f32 q * s + b, rounded once to bf16 (RNE); four 16-byte chunks of 8 k into the swizzled layout
    auto dequant_b = [&](const PReg& p, unsigned char* buf) {
        const float s = bf16_to_f32(p.s), b = bf16_to_f32(p.b);
        const uint32_t* pw = p.w;
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
            u32x4 o;
#pragma unroll
            for (int e2 = 0; e2 < 4; ++e2) {
                const int e = ch * 8 + 2 * e2;
                const float v0 = (float)((pw[e / EPW] >> ((e % EPW) * BITS)) & ((1u << BITS) - 1u)) * s + b;
                const float v1 = (float)((pw[(e + 1) / EPW] >> (((e + 1) % EPW) * BITS)) & ((1u << BITS) - 1u)) * s + b;
                o[e2] = pack_bf16(v0, v1);
            }
            const int kc = hk * 4 + ch;
            *reinterpret_cast<u32x4*>(buf + ((bn << 3) + (kc ^ (bn & 7))) * 16) = o;
        }
    };

    f32x4 acc[RT][CT];
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int j = 0; j < CT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int arow = lane & 15, kh = lane >> 4;
    auto mma_half = [&](const unsigned char* A, const unsigned char* B, int ks) {
        bf16x8 fa[RT], fb[CT];
#pragma unroll
        for (int i = 0; i < RT; ++i) fa[i] = lds_frag(A, wr * WM + i * 16 + arow, ks * 4 + kh);
#pragma unroll
        for (int j = 0; j < CT; ++j) fb[j] = lds_frag(B, wc * 64 + j * 16 + arow, ks * 4 + kh);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
        // operands swapped (W fragment first) as in the bf16 kernels: a lane holds four consecutive columns of one row
#pragma unroll
        for (int i = 0; i < RT; ++i)
#pragma unroll
            for (int j = 0; j < CT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[j], fa[i], acc[i][j], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
    };

    // Two tiles in flight: step t issues A(t+2) into the A buffer step t-1 read and the words of tile t+2 into the register set tile t
    // used; between its two MFMA halves it dequantises tile t+1 (whose words arrived during step t-1) into the B buffer step t-1 read.
    // The counted wait at the end of a step leaves the NA newest loads -- part of tile t+2 -- in flight, so A(t+1) has landed (loads
    // retire in order).  Two register sets, so the loop body is written for an even / odd pair of steps.
    const int nt = a.K / TK;
    PReg p0, p1;
    stage_a(0, bufA(0));
    load_b(0, p0);
    if (nt > 1) {
        stage_a(1, bufA(1));
        load_b(1, p1);
    }
    dequant_b(p0, bufB(0));
    if (nt > 1) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(NA) : "memory");
    else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    auto step = [&](int t, PReg& pnext, PReg& pfree) {   // pnext: words of tile t+1; pfree: receives tile t+2
        const bool more = t + 1 < nt, more2 = t + 2 < nt;
        const int ia = t % 3;
        if (more2) {
            stage_a(t + 2, bufA((ia + 2) % 3));
            load_b(t + 2, pfree);
        }
        mma_half(bufA(ia), bufB(t & 1), 0);
        if (more) dequant_b(pnext, bufB((t + 1) & 1));
        __builtin_amdgcn_sched_barrier(0);
        mma_half(bufA(ia), bufB(t & 1), 1);
        if (more2) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(NA) : "memory");
        else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    };
    for (int t = 0; t < nt; t += 2) {
        step(t, p1, p0);
        if (t + 1 < nt) step(t + 1, p0, p1);
    }

    // epilogue: 16x16 accumulator layout with swapped operands -> row = lane & 15, columns 4 * (lane >> 4) + [0, 4)
    if (act) {
        const int c0 = n0 + wc * 32 + 4 * kh;
#pragma unroll
        for (int i = 0; i < RT; ++i) {
            const int row = m0 + wr * WM + i * 16 + arow;
            if (row >= a.M) continue;
#pragma unroll
            for (int j = 0; j < CT / 2; ++j) {
                const int col = c0 + j * 16;
                if (col >= a.half) continue;   // half % 4 == 0: a run is inside or outside
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {   // fused_swiglu: one rounding (launch_gemm_bf16_swiglu, act_mode 0)
                    const float gt = round_bf16(acc[i][j][e]), up = round_bf16(acc[i][j + CT / 2][e]);
                    v[e] = gt / (1.0f + expf(-gt)) * up;
                }
                *reinterpret_cast<u32x2*>(a.out_act + (size_t)row * a.ld_act + col) = u32x2{pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3])};
            }
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < RT; ++i) {
        const int row = m0 + wr * WM + i * 16 + arow;
        if (row >= a.M) continue;
#pragma unroll
        for (int j = 0; j < CT; ++j) {
            const int col = n0 + wc * 64 + j * 16 + 4 * kh;
            if (col >= a.n_plain) continue;
            const size_t o = (size_t)row * a.ld_out + col;
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = acc[i][j][e];
            if (col + 3 < a.n_plain && (a.ld_out & 3) == 0) {
                if (a.gate) {
                    const u32x2 r = *reinterpret_cast<const u32x2*>(a.resid + o);
                    const u32x2 gt = *reinterpret_cast<const u32x2*>(a.gate + col);
                    v[0] = bf16lo(r[0]) + v[0] * bf16lo(gt[0]); v[1] = bf16hi(r[0]) + v[1] * bf16hi(gt[0]);
                    v[2] = bf16lo(r[1]) + v[2] * bf16lo(gt[1]); v[3] = bf16hi(r[1]) + v[3] * bf16hi(gt[1]);
                }
                *reinterpret_cast<u32x2*>(a.out + o) = u32x2{pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3])};
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (col + e >= a.n_plain) break;
                    float x = v[e];
                    if (a.gate) x = bf16_to_f32(a.resid[o + e]) + x * bf16_to_f32(a.gate[col + e]);
                    a.out[o + e] = f32_to_bf16(x);
                }
            }
        }
    }
}

template <int BITS, int TMR>
int set_smem_attr() {
    OMX_HIP_CHECK(hipFuncSetAttribute((const void*)qgemm_kernel<BITS, TMR>, hipFuncAttributeMaxDynamicSharedMemorySize, smem_bytes(TMR)));
    return 0;
}

int ensure_qgemm_attr() {
    static std::once_flag once;
    static int rc = 0;
    std::call_once(once, [] { rc = set_smem_attr<4, 256>() || set_smem_attr<4, 128>() || set_smem_attr<8, 256>() || set_smem_attr<8, 128>(); });
    return rc;
}

// 128-row tiles under the caller's hint (a GEMM beside another stream's grid) and where 256-row tiles would not cover the chip
int pick_rows(int M, int col_tiles) {
    if (gemm_tile_hint_get() == 128) return 128;
    return ((M + 255) / 256) * col_tiles < 160 ? 128 : 256;
}

int launch(QArgs& a, int bits, hipStream_t s) {
    if (ensure_qgemm_attr()) return 1;
    const int tmr = pick_rows(a.M, a.grid_n);
    a.grid_m = (a.M + tmr - 1) / tmr;
    const unsigned blocks = (unsigned)(a.grid_m * a.grid_n);
    if (bits == 4) {
        if (tmr == 256) qgemm_kernel<4, 256><<<blocks, NT, smem_bytes(256), s>>>(a);
        else qgemm_kernel<4, 128><<<blocks, NT, smem_bytes(128), s>>>(a);
    } else {
        if (tmr == 256) qgemm_kernel<8, 256><<<blocks, NT, smem_bytes(256), s>>>(a);
        else qgemm_kernel<8, 128><<<blocks, NT, smem_bytes(128), s>>>(a);
    }
    OMX_LAUNCH_CHECK();
    return 0;
}

int check_operands(const char* who, const bf16_t* x, const QWeight& w, int M, int K) {
    OMX_REQUIRE(x && w.w && w.scales, "%s: null tensor", who);
    OMX_REQUIRE(M > 0 && K > 0, "%s: bad shape M=%d K=%d", who, M, K);
    if (qgemm_check_format(who, K, w.group, w.bits)) return 1;
    OMX_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(w.w)) & 15u) == 0, "%s: x and the packed weight must be 16-byte aligned", who);
    return 0;
}

}  // namespace

int qgemm_check_format(const char* who, int K, int group, int bits) {
    OMX_REQUIRE(bits == 4 || bits == 8, "%s: bits must be 4 or 8 (got %d)", who, bits);
    OMX_REQUIRE(group == 32 || group == 64 || group == 128, "%s: group_size must be 32, 64 or 128 (got %d)", who, group);
    OMX_REQUIRE(K % group == 0, "%s: K=%d is not a multiple of group_size %d", who, K, group);
    OMX_REQUIRE(K % 64 == 0, "%s: K=%d must be a multiple of 64", who, K);
    return 0;
}

int launch_qgemm(bf16_t* out, const bf16_t* x, const QWeight& w, const bf16_t* resid, const bf16_t* gate, int M, int N, int K,
                 hipStream_t s) {
    if (check_operands("quantized linear", x, w, M, K)) return 1;
    OMX_REQUIRE(out && N > 0, "quantized linear: null output or N=%d", N);
    OMX_REQUIRE((resid == nullptr) == (gate == nullptr), "quantized linear: the gated form takes both resid and gate");
    QArgs a = {};
    a.x = x; a.w = w.w; a.scales = w.scales; a.biases = w.biases;
    a.out = out; a.resid = resid; a.gate = gate;
    a.M = M; a.K = K; a.group = w.group;
    a.n_plain = N; a.ld_out = N;
    a.act_tile0 = 0x7FFFFFFF;
    a.grid_n = (N + TN - 1) / TN;
    return launch(a, w.bits, s);
}

int launch_qgemm_swiglu(bf16_t* out_plain, int ld_plain, bf16_t* out_act, int ld_act, const bf16_t* x, const QWeight& w, int M,
                        int n_plain, int half, int K, hipStream_t s) {
    if (check_operands("quantized linear_swiglu", x, w, M, K)) return 1;
    OMX_REQUIRE(out_act && (n_plain == 0 || out_plain), "quantized linear_swiglu: null output");
    OMX_REQUIRE(n_plain >= 0 && n_plain % 4 == 0 && half > 0 && half % 4 == 0 && ld_act % 4 == 0 && (n_plain == 0 || ld_plain % 4 == 0),
                "quantized linear_swiglu: widths plain=%d half=%d (row strides %d / %d) must be multiples of 4", n_plain, half, ld_plain, ld_act);
    QArgs a = {};
    a.x = x; a.w = w.w; a.scales = w.scales; a.biases = w.biases;
    a.out = out_plain; a.out_act = out_act;
    a.M = M; a.K = K; a.group = w.group;
    a.n_plain = n_plain; a.ld_out = ld_plain;
    a.half = half; a.ld_act = ld_act;
    a.act_tile0 = (n_plain + TN - 1) / TN;
    a.grid_n = a.act_tile0 + (half + 127) / 128;
    return launch(a, w.bits, s);
}

}  // namespace omx

using namespace omx;

extern "C" {

int omx_quantized_linear_mfma(void* out, const void* x, const void* packed, const void* scales, const void* biases, const void* resid,
                              const void* gate, int M, int N, int K, int group_size, int bits, omx_stream stream) {
    OMX_REQUIRE(M >= 0, "omx_quantized_linear_mfma: bad shape M=%d", M);
    if (M == 0) return 0;
    const QWeight w = {(const uint32_t*)packed, (const bf16_t*)scales, (const bf16_t*)biases, group_size, bits};
    return launch_qgemm((bf16_t*)out, (const bf16_t*)x, w, (const bf16_t*)resid, (const bf16_t*)gate, M, N, K, (hipStream_t)stream);
}

int omx_quantized_linear_swiglu(void* out_plain, void* out_act, const void* x, const void* packed, const void* scales, const void* biases,
                                int M, int n_plain, int half, int K, int group_size, int bits, omx_stream stream) {
    OMX_REQUIRE(M >= 0, "omx_quantized_linear_swiglu: bad shape M=%d", M);
    if (M == 0) return 0;
    const QWeight w = {(const uint32_t*)packed, (const bf16_t*)scales, (const bf16_t*)biases, group_size, bits};
    return launch_qgemm_swiglu((bf16_t*)out_plain, n_plain, (bf16_t*)out_act, half, (const bf16_t*)x, w, M, n_plain, half, K,
                               (hipStream_t)stream);
}

}  // extern "C"
