// down GEMV + residual of layer l and [RMSNorm + q/k/v GEMV] of layer l + 1 in ONE launch (declarations and the argument block: gemv.hpp).
//
// Why: the streaming GEMVs of the decode step run at their model, 3.4 us + bytes / 6.5 TB/s -- what a launch costs beyond its bytes is the
// gap to the next one, the ramp until the first byte is usable and the tail.  The q/k/v weights of the next layer depend on nothing and are
// exactly as many registers per wave (3 rows x 8 vectors = 96 VGPRs) as the two register sets the down loop has just finished with, so a
// wave that is done with phase A asks for its q/k/v rows AT ONCE: HBM keeps streaming while the 8 KB residual row crosses the launch as
// tagged granules (granule.hpp, the scheme of the O projection inside the attention launch, attn_step.hip), and when the row has been
// swept the products wait in registers.  One boundary and one ramp less per layer.  One wave of four brings the row in BEFORE it asks for
// its rows (loads return in order: a sweep behind the weights would start when they have landed, two round trips too late).
//
// Bit-identity with the two launches it replaces:
//   phase A = gemv_kernel<NVA, 4, 2, PRO_NONE, EPI_RESIDUAL> (gemv.hip): the same lane-to-element map, fma chain, K-quarter partials summed
//             in wave order from 0.f, bf16(resid + bf16(sum)).  A thread finishes a PAIR of rows (one dword store, one granule).
//   phase B = gemv_kernel<NVB, 1, 2, PRO_RMSNORM, EPI_STORE>: thread t owns vectors t and t + 256 of the row for the sum of squares, the
//             same block_sum order, x * rstd * w rounded into LDS, the dot8 chain over j = 0..NVB-1, wave_sum, optional bias, one rounding.
//             Rows are independent: three per wave instead of four changes no bit.
// Every workgroup waits on all others: the grid must be resident as a whole (gemv_chain_grid() <= 2 per CU, the caller checks); waits are
// bounded and a wait that gives up raises abort_flag (the engine then replays the steps with two launches) instead of hanging the GPU.
#include "gemv.hpp"
#include "act16.hpp"
#include "gemv_parts.hpp"
#include "granule.hpp"
#include "launch_timing.hpp"

namespace omx {

namespace {

constexpr int kBlock = 256;   // 4 waves
constexpr int kWaves = 4;
constexpr int kSplit = 4;     // phase A: waves sharing one row
constexpr int kRowsA = 8;     // phase A: rows per workgroup (resolve_rpw of a K-split kernel)
constexpr int kRB = 2;        // phase A: rows per register batch

// NVA = 16-byte vectors per lane per row per wave of phase A (K = NVA * 4 * 512); NVB = vectors per lane per row of phase B
// (N = NVB * 512); RQ = q/k/v rows a wave holds
template <int NVA, int NVB, int RQ>
__global__ __launch_bounds__(kBlock, 2) void down_qkv_kernel(const GemvChainArgs a) {
    typedef Act16<false> A;
    constexpr int NVT = NVA * kSplit;                 // phase A: vectors per lane for the whole row
    constexpr int N = NVB * 512, K = NVT * 512;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u32x4* xs = reinterpret_cast<u32x4*>(smem);                            // A: [NVT*64] the activation; B: [NVB*64] the normalised row
    float* red = reinterpret_cast<float*>(smem + (size_t)NVT * 64 * 16);   // [4] block-reduce scratch (phase B)
    float* part = red + 8;                                                 // [kRowsA][kSplit]

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int row_begin = blockIdx.x * kRowsA;        // (N is a multiple of kRowsA and the grid N / kRowsA: every row is live)
    const int koff = wave * NVA * 64;                 // first vector of this wave's K quarter

    u32x4 wA[kRB][NVA], wB[kRB][NVA];
#define OMX_ISSUE(WB, R0)                                                                          \
    {                                                                                              \
        _Pragma("unroll") for (int r = 0; r < kRB; ++r) {                                          \
            const u32x4* p = reinterpret_cast<const u32x4*>(a.w_down + (size_t)((R0) + r) * K) + koff; \
            _Pragma("unroll") for (int j = 0; j < NVA; ++j) WB[r][j] = ld_nt(p + j * 64 + lane);   \
        }                                                                                          \
    }
#define OMX_COMPUTE(WB, R0)                                                                        \
    {                                                                                              \
        float acc[kRB];                                                                            \
        rows_dot<false, kRB, NVA>(WB, xs + koff, lane, acc);                                       \
        if (lane == 0) {                                                                           \
            _Pragma("unroll") for (int r = 0; r < kRB; ++r) part[((R0) + r - row_begin) * kSplit + wave] = acc[r]; \
        }                                                                                          \
    }

    // ---- phase A.  The first weight batch goes out before the activation is even loaded (gemv.hip) ----
    OMX_ISSUE(wA, row_begin);
    __builtin_amdgcn_sched_barrier(0);   // (hipcc would hoist the activation loads in front of them)
    const unsigned tag = *a.seq_ptr * a.tag_mul + a.tag_add;
    // the residual pair this thread will finish (threads 0..3), asked for now: nothing below waits behind the q/k/v rows for it
    const uint32_t res2 = reinterpret_cast<const uint32_t*>(a.resid)[row_begin / 2 + (threadIdx.x & 3)];
    {
        constexpr int PV = NVT * 64 / kBlock;         // vectors per thread
        static_assert(NVT * 64 % kBlock == 0, "whole vectors per thread");
        u32x4 xv[PV];
#pragma unroll
        for (int i = 0; i < PV; ++i) xv[i] = *(reinterpret_cast<const u32x4*>(a.x) + threadIdx.x + i * kBlock);
#pragma unroll
        for (int i = 0; i < PV; ++i) xs[threadIdx.x + i * kBlock] = xv[i];
        __syncthreads();
    }
    // batch b is reduced from one register set while batch b + 1 is in flight
    static_assert(kRowsA % (2 * kRB) == 0, "whole double-buffer rounds");
#pragma unroll
    for (int r0 = 0; r0 < kRowsA; r0 += 2 * kRB) {
        OMX_ISSUE(wB, row_begin + r0 + kRB);
        OMX_COMPUTE(wA, row_begin + r0);
        if (r0 + 2 * kRB < kRowsA) OMX_ISSUE(wA, row_begin + r0 + 2 * kRB);
        OMX_COMPUTE(wB, row_begin + r0 + kRB);
    }
#undef OMX_ISSUE
#undef OMX_COMPUTE
    __syncthreads();
    if (threadIdx.x < kRowsA / 2) {
        // rows 2t and 2t + 1 of the workgroup: K-quarter partials in wave order, bf16(resid + bf16(sum)) -- then the pair leaves twice:
        // to the ping-pong buffer (the attention launch reads it as its residual) and as a tagged granule for phase B of every workgroup
        const uint32_t o2 = residual_pair<A, kSplit>(part + 2 * threadIdx.x * kSplit, res2);
        reinterpret_cast<uint32_t*>(a.out)[row_begin / 2 + threadIdx.x] = o2;
        st_granule_u32(a.xg + row_begin / 2 + threadIdx.x, tag, o2);
    }

    // ---- the norm weight and the bias of phase B: asked for before anything is awaited ----
    const int q_row0 = (blockIdx.x * kWaves + wave) * RQ;
    constexpr int PVB = NVB * 64 / kBlock;            // vectors of the row per thread: thread t owns t, t + 256, ...
    static_assert(NVB * 64 % kBlock == 0, "whole vectors per thread");
    u32x4 nwv[PVB];
#pragma unroll
    for (int i = 0; i < PVB; ++i) nwv[i] = *(reinterpret_cast<const u32x4*>(a.norm_w) + threadIdx.x + i * kBlock);
    bf16_t ob[RQ];
#pragma unroll
    for (int r = 0; r < RQ; ++r) ob[r] = *(a.out_bias ? a.out_bias + min(q_row0 + r, a.qkv.rows - 1) : a.norm_w);   // (one load either way: no branch)
    u32x4 qw[RQ][NVB];
#define OMX_ISSUE_QKV()                                                                                                   \
    {                                                                                                                     \
        _Pragma("unroll") for (int r = 0; r < RQ; ++r) {                                                                  \
            const u32x4* p = reinterpret_cast<const u32x4*>(a.qkv.row_ptr(min(q_row0 + r, a.qkv.rows - 1), N)); /* clamp: surplus waves re-read the last row */ \
            _Pragma("unroll") for (int j = 0; j < NVB; ++j) qw[r][j] = ld_nt(p + j * 64 + lane);                          \
        }                                                                                                                 \
        __builtin_amdgcn_sched_barrier(0); /* keep the loads HERE: the scheduler would sink them to their use */          \
    }
    // ---- waves 1..3 ask for their q/k/v rows NOW: HBM keeps streaming through the hop.  Wave 0 -- whose loads return in order, so that
    //      a granule asked for behind 24 KB of weights would only arrive after them -- first brings the row in: it watches one granule of
    //      every eighth producer politely (a sleep between looks), sweeps all N / 2 granules into LDS, and only then asks for ITS rows,
    //      which queue behind the other waves' 3/4 of the matrix: the hop costs the launch nothing while it is shorter than that stream.
    //      (Measured, EXPERIMENTS C-3: wave 0 asking for its rows right BEHIND a peeled first pass of the sweep, tags read behind
    //      s_waitcnt vmcnt(24) -- 344.26 / 344.44 tok/s against 344.29 / 344.44, 230 VGPRs instead of 138: nothing, not in the tree.) ----
    if (wave != 0) {
        OMX_ISSUE_QKV();
    } else {
        sweep_granules<N / 2, 1>(a.xg, reinterpret_cast<unsigned*>(xs), 0, tag, lane, a.abort_flag);   // the raw row, natural element order
        OMX_ISSUE_QKV();
    }
#undef OMX_ISSUE_QKV
    // (barriers of this phase wait for LDS only: the q/k/v rows stay in flight across them)
    lds_barrier();
    // RMS-normalise in LDS (gemv.hip, PRO_RMSNORM): thread t owns vectors t, t + 256
    rmsnorm_in_lds<A, PVB>(xs, red, nwv, N, a.eps, true);
    float acc[RQ];
    rows_dot<false, RQ, NVB>(qw, xs, lane, acc);
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < RQ; ++r)
            if (q_row0 + r < a.qkv.rows) a.qkv_out[q_row0 + r] = A::bits(a.out_bias ? acc[r] + A::val(ob[r]) : acc[r]);
    }
}

constexpr int kHidden = 4096, kInter = 12288, kRQ = 3;

}  // namespace

bool gemv_chain_ok(int hidden, int inter, int n_qkv) {
    const int waves = hidden / kRowsA * kWaves;
    return hidden == kHidden && inter == kInter && n_qkv > (kRQ - 1) * waves && n_qkv <= kRQ * waves;
}

int gemv_chain_grid(int hidden) { return hidden / kRowsA; }

int launch_gemv_chain(const GemvChainArgs& a, hipStream_t s) {
    OMX_REQUIRE(gemv_chain_ok(a.N, a.K, a.qkv.rows) && a.qkv.n0 >= 0 && a.qkv.n1 >= 0 && a.qkv.rows >= a.qkv.n0 + a.qkv.n1,
                "down + q/k/v: no register layout for hidden %d, intermediate %d, %d q/k/v rows", a.N, a.K, a.qkv.rows);
    OMX_REQUIRE(a.w_down && a.x && a.resid && a.out && a.xg && a.seq_ptr && a.abort_flag && a.qkv.w0 && a.norm_w && a.qkv_out && a.tag_add >= 1u,
                "down + q/k/v: missing argument");
    const size_t shmem = (size_t)(kInter / 8) * 16 + 32 + (size_t)kRowsA * 2 * kSplit * 4;
    OMX_LAUNCH_TIMED((down_qkv_kernel<kInter / 512 / kSplit, kHidden / 512, kRQ>), dim3(gemv_chain_grid(a.N)), dim3(kBlock), shmem, s, a);
    OMX_LAUNCH_CHECK();
    return 0;
}

}  // namespace omx
