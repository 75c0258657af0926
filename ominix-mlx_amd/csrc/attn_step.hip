// Attention of ONE decode step inside the engine's step graph (Tq == 1, batch 1): q/k RMSNorm + RoPE + KV-cache append +
// split-KV SDPA + split merge in a single launch whose dependent chain is as short as the hardware allows.
//   reference: Attention::forward of qwen3-mlx/src/model.rs:161-215 (q_norm/k_norm :172-181, rope at cache.offset() :186-194,
//   cache.update_and_fetch :196, scaled_dot_product_attention :198-210 -> mlx-rs-core/src/utils.rs:191-209);
//   Mixtral / Qwen2 wiring without q/k norm (mixtral-mlx/src/model.rs:96-160, qwen3-mlx/src/qwen2.rs:100-160).
//
// Why a second decode-attention kernel next to attn_decode.hip (which stays the per-op SDPA of the mlx-c route): at batch 1 and
// a 2 k context a layer's KV is 9 MB -- 1.5 us of HBM time -- yet the round-1 kernel took 14.5 us, because it was a chain of
// eight dependent memory round trips (position -> K/V -> ... -> partial store -> ack -> counter atomic -> (m,l) -> partials ->
// output).  This kernel removes five of them:
//   * NOTHING it loads at the start depends on the position: the split a block owns is a FIXED token range
//     [split*chunk, +chunk) chosen when the step graph is captured (the engine re-captures when the context outgrows the
//     bucket), and the RoPE row of the current position sits in a small `rope_cur` buffer that the step's first kernel
//     refreshes.  Position, raw q/k/v, norm weights, RoPE row and the first K/V rows are therefore ONE round of loads;
//   * the split partials travel as data-tagged 8-byte granules {f32 value, tag} written with write-through (sc1) stores
//     (cdna_hip_programming.md Guideline 16, form R2): no store-ack wait, no arrival counter, no flag.  The tag is the step
//     sequence number x layer, so nothing has to be reset between launches;
//   * the blocks with split < G are also the consumers: after their own chunk, waves 0..D/64-1 of block (kvh, j) gather the
//     granules of head kvh*G + j with coherent loads -- all splits in flight at once, re-read until every tag matches --
//     merge them (max, rescale, sum, one division, one rounding) and store the bf16 head output.
// Every block of the launch is co-resident (one block per CU by construction, __launch_bounds__(512, 1), grid <= 256), spins are
// bounded and a wait that gives up raises `abort_flag` (the host reports it) instead of hanging the GPU.
//
// O projection in the same launch (NVW > 0; model.rs:214, 325).  The attention phase is a chain of latencies during which the HBM
// idles, and the O-projection weights (33 MB at Qwen3-8B shapes) depend on nothing: every wave issues the loads of ITS two weight
// rows right after its first K/V loads (in-order return: nothing the attention waits for is queued behind them) and keeps the rows
// in registers.  The consumers publish the merged head outputs a second time as granules {two packed bf16, tag}; every block
// sweeps those K/2 granules into LDS (all 512 threads, one coherent round per pass) and finishes with the exact arithmetic of the
// separate O GEMV (gemv_kernel<NVW, 1, 2, PRO_NONE, EPI_RESIDUAL>: same lane-to-element map, same fma order, same wave
// reduction, same roundings) -- bit-identical hidden state, one launch boundary and one weight-stream ramp less per layer.
#include <algorithm>

#include "attn.hpp"
#include "act16.hpp"
#include "gemv_parts.hpp"
#include "granule.hpp"
#include "launch_timing.hpp"

namespace omx {

namespace {

constexpr int kBlock = 512;
constexpr int kWaves = 8;

template <int N>
__device__ __forceinline__ float swap_halves(float v) {     // value of lane (l ^ N/2) of the aligned N-lane group
    if (N == 16) return dpp_f<0x128>(v);                       // row_ror:8
    return dpp_f<0x1B>(dpp_f<kDppHalfMirror>(v));              // (7 - i) then quad reverse == i ^ 4
}

template <bool F16 = false>
__device__ __forceinline__ void unpack8(const u32x4 r, float (&x)[8]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        x[2 * e] = Act16<F16>::lo(r[e]);
        x[2 * e + 1] = Act16<F16>::hi(r[e]);
    }
}

// merge the granules of one head: `NB` batches of 16 splits, every load of every live batch in flight before the first wait
template <int D, int NB, bool F16 = false>
__device__ __forceinline__ void gather_head(const AttnStepArgs& a, const uint64_t* base, int n_active, unsigned tag, int lane,
                                            int dim, bf16_t* out, uint64_t* xg_head) {
    constexpr int STRIDE = D + 2;
    unsigned long long ml0 = 0, ml1 = 0, og[NB][16];
    bool ok_ml = false, ok_b[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) ok_b[b] = b * 16 >= n_active;   // batches past the live splits are never read
    const int sl = min(lane, n_active - 1);
    for (unsigned spins = 0;; ++spins) {
        if (!ok_ml) {
            ml0 = ld_granule(base + (size_t)sl * STRIDE + D);
            ml1 = ld_granule(base + (size_t)sl * STRIDE + D + 1);
        }
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            if (ok_b[b]) continue;
#pragma unroll
            for (int j = 0; j < 16; ++j) og[b][j] = ld_granule(base + (size_t)min(b * 16 + j, n_active - 1) * STRIDE + dim);
        }
        bool all = true;
        if (!ok_ml) ok_ml = __all((unsigned)(ml0 >> 32) == tag && (unsigned)(ml1 >> 32) == tag);
        all = ok_ml;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            if (!ok_b[b]) {
                bool ok = true;
#pragma unroll
                for (int j = 0; j < 16; ++j) ok &= (unsigned)(og[b][j] >> 32) == tag;
                ok_b[b] = __all(ok);
            }
            all = all && ok_b[b];
        }
        if (all) break;
        if (spins >= kGranuleSpinLimit) {   // a producer never showed up: void result, loud flag, no hang
            if (lane == 0) __hip_atomic_store(a.abort_flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            break;
        }
        __builtin_amdgcn_s_sleep(1);
    }
    const float m = lane < n_active ? __uint_as_float((unsigned)ml0) : -INFINITY;
    const float l = lane < n_active ? __uint_as_float((unsigned)ml1) : 0.f;
    const float M = wave_max(m);
    const float f = (m == -INFINITY) ? 0.f : __expf(m - M);
    const float L = wave_sum(f * l);
    float acc = 0.f;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        if (b * 16 >= n_active) break;
#pragma unroll
        for (int j = 0; j < 16; ++j)   // splits past n_active re-read the last live one and carry f == 0
            acc = fmaf(readlane_f(f, b * 16 + j), __uint_as_float((unsigned)og[b][j]), acc);
    }
    const bf16_t r = Act16<F16>::bits(acc / L);     // (16-bit pattern: bfloat16, or float16 in a float16 model)
    out[dim] = r;
    if (xg_head) {   // the same value once more, for the O-projection phase of every block: one granule per dim pair
        const float nb = dpp_f<kDppXor1>(bf16_to_f32(r));
        if (!(lane & 1)) st_granule_u32(xg_head + dim / 2, tag, (unsigned)r | ((unsigned)f32_to_bf16(nb) << 16));
    }
}

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
typedef __attribute__((ext_vector_type(2))) float f32x2;

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
// sum of 8 exact bf16 products, f32 accumulation (v_dot2c_f32_bf16).  The pairs are taken with shufflevector from the whole
// 8-element vector: bit-casting the dwords of a u32x4 one by one made hipcc (ROCm 7.2) feed all four dot2 instructions the
// SAME register pair -- 4x the first product, silently wrong scores.
__device__ __forceinline__ float dot8_bf16(const u32x4 a, const u32x4 b) {
    const bf16x8_t A = __builtin_bit_cast(bf16x8_t, a), B = __builtin_bit_cast(bf16x8_t, b);
    float d = 0.f;
    d = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(A, A, 0, 1), __builtin_shufflevector(B, B, 0, 1), d, false);
    d = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(A, A, 2, 3), __builtin_shufflevector(B, B, 2, 3), d, false);
    d = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(A, A, 4, 5), __builtin_shufflevector(B, B, 4, 5), d, false);
    d = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(A, A, 6, 7), __builtin_shufflevector(B, B, 6, 7), d, false);
    return d;
}

// One block per CU: 8 waves share a split's token range in units of one wave-instruction (TPW token rows), so the serial
// instruction chain of a wave is a quarter of what four waves with four rows each had, two waves per SIMD cover each other's
// latencies, and the q/k RMSNorm + RoPE is done ONCE per block (wave g: query head g, wave GT % 8: the new key row) and shared
// through LDS instead of five times per wave.  attn_step_plan keeps the grid <= 256 blocks.
constexpr int kKU = 3;   // units in flight per wave

// ... and of float16 rows (a float16 checkpoint's K cache): v_dot2_f32_f16, same order
template <bool F16>
__device__ __forceinline__ float dot8_16(const u32x4 a, const u32x4 b) {
    if constexpr (!F16) return dot8_bf16(a, b);
    float d = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) d = Act16<true>::dot2(a[e], b[e], d);
    return d;
}

constexpr int kORows = 4;   // most O-projection rows a wave holds (attn_step_oproj_ok)

// ---- [RMSNorm + gate/up + SwiGLU] of the layer behind the O projection (attn_step_kernel, GU > 0) ----
// The launch's 256 blocks share the 12 288 (gate, up) row pairs: block b owns pairs [b * kGuBlockPairs, + kGuBlockPairs) and its eight waves
// draw them from a ticket counter in LDS (gateup_claim), one ticket per gateup_issue, drawn one reduce ahead -- a wave that starts late (wave 0, which brings the
// hidden row in) simply draws fewer.  The hidden row the O projection leaves crosses the launch a third time as granules {two packed bf16,
// tag}: the scheme of gemv_chain.hip's phase B, whose texts (gemv_parts.hpp) this phase calls -- the arithmetic is
// gemv_kernel<8, 1, 1, PRO_RMSNORM, EPI_SWIGLU>'s, bit for bit (a pair's value depends on its rows and the row in LDS, not on who reduces it).
constexpr int kGuBlockPairs = 48, kGuHidden = 4096, kGuNV = kGuHidden / 512;
// the phase's words in LDS (behind the attention vector; zeroed ahead of the launch's first barrier, so nothing outlives a
// launch): the ticket counter, the pairs reduced (TRACE)
enum { kGuTicket = 0, kGuReduced = 1, kGuWords = 4 };

// the next ticket of the block, wave-uniform.  Tickets >= kGuBlockPairs: nothing left (every wave draws exactly one of those)
__device__ __forceinline__ int gateup_claim(int* sm_gu, int lane) {
    int t = 0;
    if (lane == 0) t = __hip_atomic_fetch_add(sm_gu + kGuTicket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    return __builtin_amdgcn_readfirstlane(t);
}

// one (gate, up) pair into a register set: w[0] the gate row, w[1] the up row
__device__ __forceinline__ void gateup_issue(const AttnStepArgs& a, u32x4 (*w)[kGuNV], int pair, int lane) {
    const u32x4* g = reinterpret_cast<const u32x4*>(a.gu_gate + (size_t)pair * kGuHidden);
    const u32x4* u = reinterpret_cast<const u32x4*>(a.gu_up + (size_t)pair * kGuHidden);
#pragma unroll
    for (int j = 0; j < kGuNV; ++j) {
        w[0][j] = ld_nt(g + j * 64 + lane);
        w[1][j] = ld_nt(u + j * 64 + lane);
    }
    __builtin_amdgcn_sched_barrier(0);   // keep the loads HERE: the scheduler would sink them to their use
}

// the merged attention vector: awaited, then swept from its granules into LDS (natural element order); a block-wide step.
// (Written out, not sweep_granules: all 512 threads share the sweep and meet in __syncthreads_and between passes.)
// (With gate/up in the launch, the first pair of waves 1..7 asked for right behind a peeled first pass of this sweep, tags read behind a
//  counted wait: measured SLOWER than asking once the O rows are consumed -- EXPERIMENTS C-3 -- and not in the tree.)
template <int NVW>
__device__ __forceinline__ void oproj_await_vector(const AttnStepArgs& a, u32x4* sm_x, unsigned tag, int lane, int wave) {
    // wait politely: ONE wave watches one granule per consumer wave (the last of its 32) with a sleep between looks; only then does
    // the block read the whole vector -- normally once (measured: sweep done at 11.3 us with the watch, 11.9 us without)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (wave == 0) {
        constexpr int SEGS = NVW * 8;                                  // consumer waves: H * D / 64
        const uint64_t* probe = a.xg + (size_t)min(lane, SEGS - 1) * 32 + 31;
        for (unsigned spins = 0; spins < kGranuleSpinLimit; ++spins) {
            const unsigned long long g = ld_granule(probe);
            if (__all((unsigned)(g >> 32) == tag)) break;
            __builtin_amdgcn_s_sleep(4);
        }
    }
    __syncthreads();
    // sweep the granules into LDS: thread t owns granules [t * GP, + GP) of NVW * 256
    constexpr int GP = (NVW + 1) / 2;      // NVW * 256 granules over 512 threads: 1, 1, 2, 4 (NVW = 7: 448 threads), 4
    static_assert((NVW * 256) % GP == 0, "a thread takes all of its granules or none");
    bool done = (int)threadIdx.x * GP >= NVW * 256;
    unsigned* sx = reinterpret_cast<unsigned*>(sm_x);
    for (unsigned spins = 0;; ++spins) {
        if (!done) {
            unsigned long long g[GP];
#pragma unroll
            for (int i = 0; i < GP; ++i) g[i] = ld_granule(a.xg + (size_t)threadIdx.x * GP + i);
            bool ok = true;
#pragma unroll
            for (int i = 0; i < GP; ++i) ok &= (unsigned)(g[i] >> 32) == tag;
            if (ok) {
#pragma unroll
                for (int i = 0; i < GP; ++i) sx[threadIdx.x * GP + i] = (unsigned)g[i];
                done = true;
            }
        }
        if (__syncthreads_and(done)) break;                          // also orders the LDS writes before the reads below
        if (spins >= kGranuleSpinLimit) {
            if (threadIdx.x == 0) __hip_atomic_store(a.abort_flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            break;
        }
        __builtin_amdgcn_s_sleep(2);
    }
}

// a pair in a register set reduced against the normalised row in LDS: rows_dot with NR = 2, then gemv.hip's SwiGLU epilogue
// (DN: the value is parked in LDS at its ticket's slot as well, for the activation hop of down_qkv_phase)
template <bool DN = false>
__device__ __forceinline__ void gateup_reduce(const AttnStepArgs& a, const u32x4 (*w)[kGuNV], const u32x4* xs, int pair, int lane,
                                              uint16_t* park = nullptr) {
    typedef Act16<false> A;
    float acc[2];
    rows_dot<false, 2, kGuNV>(w, xs, lane, acc);
    if constexpr (DN) {
        if (lane == 0) {
            const uint16_t v = epi_bits<EPI_SWIGLU, A>(acc[0], acc[1], (bf16_t)0, 0);
            a.gu_out[pair] = v;
            *park = v;
        }
    } else
    if (lane == 0) a.gu_out[pair] = epi_bits<EPI_SWIGLU, A>(acc[0], acc[1], (bf16_t)0, 0);
}

// ---- [down + residual] of the layer and [RMSNorm + q/k/v] of the NEXT layer behind gate/up (attn_step_kernel, DN) ----
// The launch that ends a layer: gemv_chain.hip's down_qkv_kernel on the 256 blocks of this launch, bit for bit.  Two more hops: the
// block's 48 activations leave as 24 granules {two packed bf16, tag} and every block sweeps all 6 144 into LDS; the 16 residual rows a
// block finishes leave as 8 granules and every block sweeps the 2 048.  Block b owns down rows [b * kDnBlockRows, + kDnBlockRows): 32 units
// of (row pair, K quarter), 12 KB each, drawn from a ticket counter in LDS into two register sets per wave.  The arithmetic is
// gemv_kernel<6, 4, 2, PRO_NONE, EPI_RESIDUAL>'s -- a quarter is a dot8 chain over its six vectors per lane + wave_sum, the four partials are
// added in quarter order from 0.f, bf16(resid + bf16(sum)) -- and gemv_kernel<8, 1, 2, PRO_RMSNORM, EPI_STORE>'s on three q/k/v rows per
// wave.  What is asked for where:
//   * hop four (activation vector): the block's 24 activation granules are stored FIRST, behind the barrier that follows the block's last
//     pair; only then does a non-sweeper wave ask for its first two down units -- they depend on nothing -- and NOTHING else: 24 KB per
//     wave stream through the hop.  Waves 0 and 4 bring the activation vector in, half each, in one straight-line pass (nothing of their
//     own in flight in front of the granules; one down unit behind them, the tags read behind a counted wait);
//   * hop five (residual row): behind the block's last unit wave 0 finishes the 16 rows and stores their 8 granules, asks for the whole
//     residual row at once -- no watch: an optimistic straight-line pass right behind the publish -- and the block meets at an LDS-only
//     barrier; behind it every wave asks for all three of its q/k/v rows (192 KB per block), which stream while the row crosses and is
//     normalised.  Wave 0 reads the tags behind a counted wait (its rows stay in flight); a tag that is not there yet sends it into the
//     draining retry loop, behind the rows.  Until C-6 two of the three rows were asked for around hop four, which did not want them,
//     and hop five idled HBM.  Forms measured at Qwen3-8B shapes, ctx 2 k (EXPERIMENTS C-4; parent 347.6 tok/s):
//   * wave 0 alone sweeping the activation vector in three passes of 32 granules per lane, all q/k/v rows asked for behind the last unit
//     (wave 0's behind the row's sweep): 344.1; with two q/k/v rows up front: 343.7 -- more requests queued, longer round trips;
//   * waves 0 and 4 sweeping half each in one pass: 351.9; without the watch in front of the residual row's sweep: 350.6.
// Issue order around the hop (EXPERIMENTS C-5, mean tok/s against the parent's of the same interleaved set):
//   * both rows behind the sweepers' pass, two units in front: 354.07 against 353.96; one unit in front, the second behind the pass with the
//     rows: 351.85; two units + one row in front, one row behind the pass: 354.42 (set 1), 352.90 against 351.25 (set 2) -- no gain alone;
//   * the first down unit into the register set that gate/up's loop leaves free: 353.73; the third q/k/v row ahead of the last unit's
//     reduce: 352.68; all three together: 353.49 against 353.96 -- not in the tree;
//   * the activation granules stored before the block's own requests (they used to queue behind the other waves' 240 KB): 355.37 against
//     351.25; with two units + one row in front and one row behind the pass (the tree until C-6): 355.98 (set 2), 356.64 against 351.67 (set 3).
// The rows moved to hop five (EXPERIMENTS C-6, mean tok/s of four runs; parent 358.41 in set 1, 355.62 in set 2):
//   * A, publish -> watch -> pass -> barrier -> three rows: 361.60; B, the same without the watch, as here: 368.33 (set 1), 365.89 (set 2);
//   * C, the rows of waves 1..7 right behind a barrier that follows the publish, wave 0 watch -> pass -> its rows: 366.56, 364.17; C without
//     the watch: 361.22 (set 2) -- the rows in front of the optimistic pass delay it, and a miss costs a second pass;
//   * E, row 0 left in front of hop four, on A / B / C: 362.51 / 367.09 / 365.62 (set 1), on B 364.35 (set 2) -- row 0 carries 1.2-1.5 of B's 10;
//   * D, a third named down set through hop four: 256 VGPRs and 332 bytes of scratch -- not run.
// The residual row's norm (EXPERIMENTS C-7): hipcc holds s_waitcnt vmcnt(4) / (3) / (3) between its barriers -- the norm weight was asked for
// ahead of the rows, but across the join of the two arms the count is lost -- so the row is normalised when 21 of a wave's 24 row loads have
// landed.  With the weight read from LDS (parked there by the launch's first round of loads) no wait is left in the norm: 368.55 against the
// parent's 367.79 in one set, 366.43 against 366.71 in the other, +0.1 on top of hop three's publish-first form -- the rows land while the
// norm runs either way.  Not in the tree.
constexpr int kDnInter = 12288, kDnBlockRows = 16, kDnNV = kDnInter / 512 / 4, kDnUnits = kDnBlockRows / 2 * 4, kDnQRows = 3;
// LDS of the phase, in the (dead) split-merge area at the front: the activation vector, the K-quarter partials, the parked activations
constexpr int kDnPartOff = kDnInter * 2, kDnParkOff = kDnPartOff + kDnBlockRows * 4 * 4, kDnLdsBytes = kDnParkOff + kGuBlockPairs * 2;
// the phase's words behind gate/up's in LDS: the unit ticket counter; units reduced and q/k/v rows stored (TRACE)
enum { kDnTicket = 4, kDnReduced = 5, kDnStored = 6, kDnWords = 8 };

__device__ __forceinline__ int down_claim(int* sm_gu, int lane) {
    int t = 0;
    if (lane == 0) t = __hip_atomic_fetch_add(sm_gu + kDnTicket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    return __builtin_amdgcn_readfirstlane(t);
}

// unit `u` of the block = rows row_begin + 2 * (u / 4) + {0, 1}, K quarter u % 4, into a register set
__device__ __forceinline__ void down_issue(const AttnStepArgs& a, u32x4 (*w)[kDnNV], int row_begin, int u, int lane) {
    const u32x4* p = reinterpret_cast<const u32x4*>(a.dn_w) + (size_t)(row_begin + 2 * (u >> 2)) * (kDnInter / 8) + (u & 3) * (kDnNV * 64) + lane;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
#pragma unroll
        for (int j = 0; j < kDnNV; ++j) w[r][j] = ld_nt(p + (size_t)r * (kDnInter / 8) + j * 64);
    }
    __builtin_amdgcn_sched_barrier(0);   // keep the loads HERE: the scheduler would sink them to their use
}

// a unit in a register set reduced against its quarter of the activation vector in LDS: gemv_chain.hip's OMX_COMPUTE
__device__ __forceinline__ void down_reduce(const u32x4 (*w)[kDnNV], const u32x4* xa, float* part, int u, int lane) {
    float acc[2];
    rows_dot<false, 2, kDnNV>(w, xa + (u & 3) * (kDnNV * 64), lane, acc);
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < 2; ++r) part[(2 * (u >> 2) + r) * 4 + (u & 3)] = acc[r];
    }
}

// Every wave of every block of a DN launch ends here, behind its last (gate, up) pair; `res2`: the residual pair of rows
// 2 * (lane & 7) + {0, 1} of the block.  Every wave passes the same barriers on every path, the give-up included; they wait for LDS only.
template <bool TRACE>
__device__ __forceinline__ void down_qkv_phase(const AttnStepArgs& a, unsigned char* sm_dn, u32x4* xs, float* red, int* sm_gu, unsigned res2,
                                               unsigned tag, int lane, int wave, unsigned long long* tr) {
    typedef Act16<false> A;
    u32x4* xa = reinterpret_cast<u32x4*>(sm_dn);
    float* part = reinterpret_cast<float*>(sm_dn + kDnPartOff);
    const int blk = (int)blockIdx.y * (int)gridDim.x + (int)blockIdx.x;
    const int row_begin = blk * kDnBlockRows;
    const int q_row0 = (blk * kWaves + __builtin_amdgcn_readfirstlane(wave)) * kDnQRows;   // (in scalar registers: so are the row pointers)
    // the next layer's norm weight and bias: asked for before any weight row
    constexpr int PV = kGuNV * 64 / 256;
    u32x4 nwv[PV];
#pragma unroll
    for (int i = 0; i < PV; ++i) nwv[i] = *(reinterpret_cast<const u32x4*>(a.nq_norm_w) + (threadIdx.x & 255) + i * 256);
    bf16_t ob[kDnQRows];
#pragma unroll
    for (int r = 0; r < kDnQRows; ++r) ob[r] = *(a.nq_bias ? a.nq_bias + min(q_row0 + r, a.nq.rows - 1) : a.nq_norm_w);   // (one load either way: no branch)
    u32x4 dA[2][kDnNV], dB[2][kDnNV];
    int tA = 0, tB = 0;
    u32x4 qw[kDnQRows][kGuNV];
    auto issue_qkv = [&]() {
#pragma unroll
        for (int r = 0; r < kDnQRows; ++r) {
            const u32x4* p = reinterpret_cast<const u32x4*>(a.nq.row_ptr(min(q_row0 + r, a.nq.rows - 1), kGuHidden));   // clamp: surplus waves re-read the last row
#pragma unroll
            for (int j = 0; j < kGuNV; ++j) qw[r][j] = ld_nt(p + j * 64 + lane);
        }
        __builtin_amdgcn_sched_barrier(0);   // keep the loads HERE: the scheduler would sink them to their use
    };
    // (the two tickets a wave draws ahead of the loop are below kDnUnits, no check: sixteen of the 32)
    // Measured (EXPERIMENTS C-4): the more weight requests are queued when the sweep starts, the longer each of its round trips -- the hop is
    // kept short by its number of round trips, not by what is parked in front of it
    const bool sweeper = (wave & (kWaves / 2 - 1)) == 0;   // waves 0 and 4 bring the activation vector in, half each
    lds_barrier();   // the block's 48 activations are parked
    // publish FIRST: every block's sweep waits for the slowest block's granules, and stored behind the block's own 240 KB of fresh weight
    // requests they became visible late (the sweep was done at 55.9 us; with this order at 48.8, EXPERIMENTS C-5)
    if (wave == 0 && lane < kGuBlockPairs / 2)
        st_granule_u32(a.ag + (size_t)blk * (kGuBlockPairs / 2) + lane, tag, reinterpret_cast<const unsigned*>(sm_dn + kDnParkOff)[lane]);
    lds_barrier();   // the block's granules are in the CU's queue: what the block asks for now is behind them
    if (sweeper) {
        // (written out, not sweep_granules: the first pass is straight-line, its tags read behind a counted wait -- gateup_phase's pattern)
        constexpr int HALF = kDnInter / 2 / 2, GPL = HALF / 64;   // the granules of a sweeper's half, per lane
        const int half = __builtin_amdgcn_readfirstlane(wave) / (kWaves / 2);
        const uint64_t* gr = a.ag + (size_t)half * HALF;
        for (unsigned spins = 0; spins < kGranuleSpinLimit; ++spins) {   // politely: one granule per lane, a sleep between looks
            const unsigned long long g = ld_granule(gr + (size_t)lane * GPL + (GPL - 1));
            if (__all((unsigned)(g >> 32) == tag)) break;
            __builtin_amdgcn_s_sleep(4);
        }
        unsigned long long g[GPL];
#pragma unroll
        for (int i = 0; i < GPL; ++i) g[i] = ld_granule(gr + (size_t)i * 64 + lane);
        __builtin_amdgcn_sched_barrier(0);
        lds_barrier();   // the sweep is in the CU's queue: what the block asks for now is behind it
        tA = down_claim(sm_gu, lane);
        down_issue(a, dA, row_begin, tA, lane);   // (one unit: with two, or with the rows, behind 96 registers of granules the kernel spills)
        unsigned bad = 0;
#pragma unroll
        for (int i = 0; i < GPL; ++i) bad |= (unsigned)(g[i] >> 32) ^ tag;
        asm volatile("; activation vector: tags read behind the first down unit" : "+v"(bad));
        if (!__all(bad == 0)) {
            for (unsigned spins = 0;; ++spins) {
#pragma unroll
                for (int i = 0; i < GPL; ++i) g[i] = ld_granule(gr + (size_t)i * 64 + lane);
                bool ok = true;
#pragma unroll
                for (int i = 0; i < GPL; ++i) ok &= (unsigned)(g[i] >> 32) == tag;
                if (__all(ok)) break;
                if (spins >= kGranuleSpinLimit) {   // a producer never showed up: void result, loud flag, no hang
                    if (lane == 0) __hip_atomic_store(a.abort_flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    break;
                }
                __builtin_amdgcn_s_sleep(4);
            }
        }
        unsigned* sx = reinterpret_cast<unsigned*>(xa) + half * HALF;   // natural element order
#pragma unroll
        for (int i = 0; i < GPL; ++i) sx[i * 64 + lane] = (unsigned)g[i];
        if (TRACE && threadIdx.x == 0) tr[11] = wall_clock64();
        tB = down_claim(sm_gu, lane);   // into the registers the granules have left
        down_issue(a, dB, row_begin, tB, lane);
    } else {
        tA = down_claim(sm_gu, lane);
        down_issue(a, dA, row_begin, tA, lane);
        tB = down_claim(sm_gu, lane);
        down_issue(a, dB, row_begin, tB, lane);
        lds_barrier();   // (the sweepers' barrier behind their pass)
    }
    lds_barrier();   // the activation vector is in LDS
    down_reduce(dA, xa, part, tA, lane);
    if (TRACE && threadIdx.x == 0) tr[12] = wall_clock64();
    // the loop of gateup_phase: wave-uniform branches over two named sets, the ticket of a refill drawn one reduce ahead
    // (written out at both places: hipcc's counted waits depend on the two named register sets, EXPERIMENTS C-3)
    int n_reduced = 1;
    int nA = down_claim(sm_gu, lane), nB;
    for (;;) {
        if (nA >= kDnUnits) {
            down_reduce(dB, xa, part, tB, lane);
            ++n_reduced;
            break;
        }
        tA = nA;
        down_issue(a, dA, row_begin, tA, lane);
        nB = down_claim(sm_gu, lane);
        down_reduce(dB, xa, part, tB, lane);
        if (nB >= kDnUnits) {
            down_reduce(dA, xa, part, tA, lane);
            n_reduced += 2;
            break;
        }
        tB = nB;
        down_issue(a, dB, row_begin, tB, lane);
        nA = down_claim(sm_gu, lane);
        down_reduce(dA, xa, part, tA, lane);
        n_reduced += 2;
    }
    if (TRACE && lane == 0) __hip_atomic_fetch_add(sm_gu + kDnReduced, n_reduced, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    lds_barrier();   // every K-quarter partial of the block's 16 rows is in LDS
    // publish FIRST, as at the head of the phase: every block's sweep waits for the slowest block's granules
    if (wave == 0 && lane < kDnBlockRows / 2) {
        // rows 2 * lane and 2 * lane + 1 of the block: the pair leaves twice, to the ping-pong buffer (the next attention launch reads it
        // as its residual) and as a tagged granule for the q/k/v rows of every block
        const uint32_t o2 = residual_pair<A, 4>(part + 2 * lane * 4, res2);
        reinterpret_cast<uint32_t*>(a.dn_out)[row_begin / 2 + lane] = o2;
        st_granule_u32(a.rg + row_begin / 2 + lane, tag, o2);
    }
    if (wave == 0) {
        // (written out, not sweep_granules: the first pass is straight-line, its tags read behind a counted wait -- gateup_phase's pattern)
        // No watch: the optimistic pass goes out right behind the publish, so the block's 192 KB of q/k/v rows are asked for at once and
        // stream while the row crosses; a pass that came too early is repeated behind them (measured against the watched forms, C-6)
        constexpr int GPL = kGuHidden / 2 / 64;   // granules per lane
        unsigned long long g[GPL];
#pragma unroll
        for (int i = 0; i < GPL; ++i) g[i] = ld_granule(a.rg + (size_t)i * 64 + lane);
        __builtin_amdgcn_sched_barrier(0);
        lds_barrier();   // the publish and the sweep are in the CU's queue: what the block asks for now is behind them
        issue_qkv();
        unsigned bad = 0;
#pragma unroll
        for (int i = 0; i < GPL; ++i) bad |= (unsigned)(g[i] >> 32) ^ tag;
        asm volatile("; residual row: tags read behind wave 0's q/k/v rows" : "+v"(bad));
        if (!__all(bad == 0)) {
            for (unsigned spins = 0;; ++spins) {
#pragma unroll
                for (int i = 0; i < GPL; ++i) g[i] = ld_granule(a.rg + (size_t)i * 64 + lane);
                bool ok = true;
#pragma unroll
                for (int i = 0; i < GPL; ++i) ok &= (unsigned)(g[i] >> 32) == tag;
                if (__all(ok)) break;
                if (spins >= kGranuleSpinLimit) {   // a producer never showed up: void result, loud flag, no hang
                    if (lane == 0) __hip_atomic_store(a.abort_flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    break;
                }
                __builtin_amdgcn_s_sleep(4);
            }
        }
        unsigned* sx = reinterpret_cast<unsigned*>(xs);   // the raw row, natural element order
#pragma unroll
        for (int i = 0; i < GPL; ++i) sx[i * 64 + lane] = (unsigned)g[i];
        if (TRACE && lane == 0) tr[13] = wall_clock64();
    } else {
        lds_barrier();
        issue_qkv();   // all three rows, into the registers the wave's down sets have left
    }
    lds_barrier();   // the residual row is in LDS
    rmsnorm_in_lds<A, PV>(xs, red, nwv, kGuHidden, a.eps, threadIdx.x < 256);
    float acc[kDnQRows];
    rows_dot<false, kDnQRows, kGuNV>(qw, xs, lane, acc);
    if (lane == 0) {
        int stored = 0;
#pragma unroll
        for (int r = 0; r < kDnQRows; ++r)
            if (q_row0 + r < a.nq.rows) {
                a.nq_out[q_row0 + r] = A::bits(a.nq_bias ? acc[r] + A::val(ob[r]) : acc[r]);
                ++stored;
            }
        if (TRACE) __hip_atomic_fetch_add(sm_gu + kDnStored, stored, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    if constexpr (TRACE) {   // when the block's rows were stored; the units it reduced | the q/k/v rows it stored << 32
        lds_barrier();
        if (threadIdx.x == 0) {
            tr[14] = wall_clock64();
            tr[15] = (unsigned long long)sm_gu[kDnReduced] | (unsigned long long)sm_gu[kDnStored] << 32;
        }
    }
}

// Every wave of every block ends here.  `pub_rows` > 0: the block's O rows [pub_row0, + pub_rows) are parked in sm_pub (a block of O
// waves holds an even number of rows from an even row on: whole granules).  Waves 1..7 ask for their first pair at once (in the layer
// launch's O blocks: behind the publish, see below).  Wave 0 -- no weight load in flight: a granule asked for behind 32 KB of weights would
// only arrive after them -- publishes the rows, watches (not in the layer launch), and asks for the whole hidden row ONCE in straight-line
// code; right behind those 32 granule loads the block meets at an LDS-only barrier,
// wave 0 asks for its first pair and the others for their SECOND: all of it is queued behind the sweep -- it cannot delay it -- and
// streams while the row makes its round trip and is normalised.  Wave 0 reads the tags behind a counted wait (hipcc counts loads exactly
// in straight-line code only; the pair stays in flight); a tag that is not there yet (rare) sends it into the draining retry loop.
// Every wave passes the same three barriers (four in a block that publishes first) on every path, the give-up included.
// Issue points measured at Qwen3-8B shapes, ctx 2 k:
//   * (EXPERIMENTS C-2) first pair of waves 1..7 HERE, once their O rows are consumed: 343.4 tok/s against the parent's 337.7; right
//     behind the O rows' own loads -- 57 MB more parked in front of the split merge and the attention vector's sweep -- 338.1: no gain;
//   * (EXPERIMENTS C-3) pairs drawn from the block's ticket counter instead of six per wave: 346.4 against the parent's 344.4; with wave
//     0's first and the others' second pair behind the hidden row's sweep as well: 347.5; the first pair of waves 1..7 moved up behind
//     the ATTENTION VECTOR's sweep on top of that: 343.9, slower than the parent -- that sweep feeds the O rows every block waits for;
//   * wave 0's second pair asked for as soon as the row is in LDS instead of behind the norm: 342.7 against 346.4.
// Hop three of the layer launch (DN; EXPERIMENTS C-7, mean tok/s of four runs; parent 367.79 in set 1, 366.71 in set 2).  An O block (PUB)
// publishes FIRST, as down_qkv_phase does at hops four and five: wave 0 stores the block's O rows behind the barrier that follows their
// parking, the block meets at a second LDS-only barrier, and only then do waves 1..7 ask for their first pair -- stored behind the 112 KB
// they used to ask for ahead of the first barrier, the granules became visible late, and every block's sweep waits for the slowest block's.
// And wave 0 does not watch: its optimistic pass goes out right behind the publish, a miss goes to the draining retry loop (hop five's form).
//   * P, publish first, with the watch: 373.87 (set 1); P', without it, as here: 375.84 (set 1), 374.90 (set 2);
//   * N, the hidden row's norm reading its weight from LDS (parked there by the launch's first round of loads), one arm per wave class from
//     a pair's issue to its reduce -- no s_waitcnt vmcnt between the row's LDS write and the first reduce, which then waits for vmcnt(31)
//     .. (16) with the second pair in flight: 364.72 against the parent's 367.79 (set 1), 363.04 against 366.71 with the weights parked
//     behind the block's own chunk (set 2) -- SLOWER; with wave 0's second pair asked for as soon as the row is in LDS: 364.54 (set 1);
//   * N5, the same norm in hop five: 368.55 (set 1), 366.43 (set 2, parked late) -- inside the parent's spread; P' + N5: 375.00 (set 2),
//     P' + N + N5: 373.64, with the early second pair 372.66 -- neither N nor N5 is in the tree.
// A consumer block (PUB false) publishes nothing here and keeps its early first pair.
template <bool TRACE, bool DN = false, bool PUB = false>
__device__ __forceinline__ void gateup_phase(const AttnStepArgs& a, u32x4* xs, float* red, int* sm_gu, const uint16_t* sm_pub, unsigned tag,
                                             int lane, int wave, int pub_row0, int pub_rows, unsigned long long* tr,
                                             unsigned char* sm_dn = nullptr) {
    typedef Act16<false> A;
    constexpr bool PFIRST = DN && PUB;   // the layer launch's O blocks: the O rows leave before the block asks for anything
    const int pair0 = ((int)blockIdx.y * (int)gridDim.x + (int)blockIdx.x) * kGuBlockPairs;
    uint16_t* park = DN ? reinterpret_cast<uint16_t*>(sm_dn + kDnParkOff) : nullptr;   // DN: the block's values by ticket
    constexpr int PV = kGuNV * 64 / 256;              // vectors of the row per thread of the first four waves
    u32x4 nwv[PV];
#pragma unroll
    for (int i = 0; i < PV; ++i) nwv[i] = *(reinterpret_cast<const u32x4*>(a.gu_norm_w) + (threadIdx.x & 255) + i * 256);
    u32x4 wA[2][kGuNV], wB[2][kGuNV];
    int tA = 0, tB;
    // (the two tickets a wave draws ahead of the norm are below kGuBlockPairs, no check: all sixteen are drawn before the barrier in front
    //  of it, and the tickets that are compared with kGuBlockPairs are drawn behind it)
    if (!PFIRST && wave != 0) {
        tA = gateup_claim(sm_gu, lane);
        gateup_issue(a, wA, pair0 + tA, lane);
    }
    lds_barrier();   // every wave is done with the attention vector in `xs` and has parked its O rows
    if constexpr (PFIRST) {
        if (wave == 0 && lane < pub_rows / 2) st_granule_u32(a.hg + pub_row0 / 2 + lane, tag, reinterpret_cast<const unsigned*>(sm_pub)[lane]);
        lds_barrier();   // the block's granules are in the CU's queue: what the block asks for now is behind them
        if (wave != 0) {
            tA = gateup_claim(sm_gu, lane);
            gateup_issue(a, wA, pair0 + tA, lane);
        }
    }
    if (wave == 0) {
        if constexpr (!PFIRST) {
            if (lane < pub_rows / 2) st_granule_u32(a.hg + pub_row0 / 2 + lane, tag, reinterpret_cast<const unsigned*>(sm_pub)[lane]);
        }
        // (written out, not sweep_granules: the first pass is straight-line, its tags read behind a counted wait)
        constexpr int GPL = kGuHidden / 2 / 64;       // granules per lane
        if constexpr (!DN) {   // (the layer launch does not watch: see above)
            for (unsigned spins = 0; spins < kGranuleSpinLimit; ++spins) {   // politely: one granule of every eighth producer, a sleep between looks
                const unsigned long long g = ld_granule(a.hg + (size_t)lane * GPL + (GPL - 1));
                if (__all((unsigned)(g >> 32) == tag)) break;
                __builtin_amdgcn_s_sleep(4);
            }
        }
        unsigned long long g[GPL];
#pragma unroll
        for (int i = 0; i < GPL; ++i) g[i] = ld_granule(a.hg + (size_t)i * 64 + lane);
        __builtin_amdgcn_sched_barrier(0);
        lds_barrier();   // the sweep is in the CU's queue: what the block asks for now is behind it
        tA = gateup_claim(sm_gu, lane);
        gateup_issue(a, wA, pair0 + tA, lane);
        unsigned bad = 0;
#pragma unroll
        for (int i = 0; i < GPL; ++i) bad |= (unsigned)(g[i] >> 32) ^ tag;
        asm volatile("; hidden row: tags read behind the first (gate, up) pair" : "+v"(bad));
        if (!__all(bad == 0)) {
            for (unsigned spins = 0;; ++spins) {
#pragma unroll
                for (int i = 0; i < GPL; ++i) g[i] = ld_granule(a.hg + (size_t)i * 64 + lane);
                bool ok = true;
#pragma unroll
                for (int i = 0; i < GPL; ++i) ok &= (unsigned)(g[i] >> 32) == tag;
                if (__all(ok)) break;
                if (spins >= kGranuleSpinLimit) {   // a producer never showed up: void result, loud flag, no hang
                    if (lane == 0) __hip_atomic_store(a.abort_flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    break;
                }
                __builtin_amdgcn_s_sleep(4);
            }
        }
        unsigned* sx = reinterpret_cast<unsigned*>(xs);   // the raw row, natural element order
#pragma unroll
        for (int i = 0; i < GPL; ++i) sx[i * 64 + lane] = (unsigned)g[i];
        if (TRACE && lane == 0 && pub_rows > 0) tr[4] = wall_clock64();
        tB = gateup_claim(sm_gu, lane);   // drawn on this side of the barrier (see above), asked for behind the norm
    } else {
        lds_barrier();
        tB = gateup_claim(sm_gu, lane);
        gateup_issue(a, wB, pair0 + tB, lane);
    }
    lds_barrier();
    // DN: the raw hidden row is the down rows' residual.  The pair a finishing thread of down_qkv_phase needs is read now, before the norm
    // overwrites the row (its first barrier waits for this read); the plain `o_out` another block stored is not visible inside the launch
    unsigned res2 = 0;
    if constexpr (DN) res2 = reinterpret_cast<const unsigned*>(xs)[(pair0 / kGuBlockPairs) * (kDnBlockRows / 2) + (lane & (kDnBlockRows / 2 - 1))];
    rmsnorm_in_lds<A, PV>(xs, red, nwv, kGuHidden, a.eps, threadIdx.x < 256);
    // Wave 0 asks for its second pair only now: the norm's last barrier waits for every load of the first four waves (hipcc drains in
    // front of it), and a pair asked for when the row was in LDS would hold the whole block for its round trip.  (Two arms with an asm
    // text of their own: merged, the wait in front of the first reduce would drain wave 0's second pair.)
    if (wave == 0) {
        gateup_issue(a, wB, pair0 + tB, lane);
        gateup_reduce<DN>(a, wA, xs, pair0 + tA, lane, park + tA);
        if (TRACE && threadIdx.x == 0) tr[7] = wall_clock64();
        asm volatile("; first pair reduced: wave 0, its second pair just asked for" ::: "memory");
    } else {
        gateup_reduce<DN>(a, wA, xs, pair0 + tA, lane, park + tA);
        asm volatile("; first pair reduced: the second pair came in through the hop" ::: "memory");
    }
    // Both sets are in flight.  A set is reduced and refilled with the pair of the wave's next ticket -- or, with no pair left, the other
    // set is reduced and the wave is done.  Wave-uniform branches over two named sets, each arm with a load count of its own: hipcc's waits
    // stay counted (a refill skipped under a condition makes the wait that follows drain the set in flight).  The ticket of a refill is
    // drawn one reduce AHEAD (nA, nB): the LDS round trip hides behind the reduce, and with the draw at the loop's head hipcc drained the
    // set in flight there (s_waitcnt vmcnt(0) in front of the draw's first VALU write): 346.4 against 347.5 tok/s, EXPERIMENTS C-3
    // (written out here and in down_qkv_phase, not a template over the sets: the counted waits depend on the two NAMED sets)
    int n_reduced = 1;
    int nA = gateup_claim(sm_gu, lane), nB;
    for (;;) {
        if (nA >= kGuBlockPairs) {
            gateup_reduce<DN>(a, wB, xs, pair0 + tB, lane, park + tB);
            ++n_reduced;
            break;
        }
        tA = nA;
        gateup_issue(a, wA, pair0 + tA, lane);
        nB = gateup_claim(sm_gu, lane);
        gateup_reduce<DN>(a, wB, xs, pair0 + tB, lane, park + tB);
        if (nB >= kGuBlockPairs) {
            gateup_reduce<DN>(a, wA, xs, pair0 + tA, lane, park + tA);
            n_reduced += 2;
            break;
        }
        tB = nB;
        gateup_issue(a, wB, pair0 + tB, lane);
        nA = gateup_claim(sm_gu, lane);
        gateup_reduce<DN>(a, wA, xs, pair0 + tA, lane, park + tA);
        n_reduced += 2;
    }
    if constexpr (TRACE) {   // when wave 0 and wave 7 reduced their last pair, and how many pairs the block reduced
        if (lane == 0) {
            __hip_atomic_fetch_add(sm_gu + kGuReduced, n_reduced, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (wave == 0) tr[8] = wall_clock64();
            if (wave == kWaves - 1) tr[9] = wall_clock64();
        }
        lds_barrier();
        if (threadIdx.x == 0) tr[10] = (unsigned long long)sm_gu[kGuReduced];
    }
    if constexpr (DN) down_qkv_phase<TRACE>(a, sm_dn, xs, red, sm_gu, res2, tag, lane, wave, tr);
}

// The O-projection phase of a non-consumer block (attn_step_kernel, NVW > 0): R weight rows per wave go out NOW -- the block's
// latency-critical work is over and its attention registers are free -- then the merged attention vector is awaited and swept into
// LDS, then the separate O GEMV's arithmetic (gemv.hip gemv_kernel<NVW, 1, 2, PRO_NONE, EPI_RESIDUAL>) runs on the held rows.
// Measured alternatives at Qwen3-8B shapes, ctx 2 k: weight loads issued with the first K/V round -> 33 MB of requests fill the HBM
// queues ahead of the q / K / V rows (they land at 6.7 us instead of 2.1); issued after that round landed, in every block -> a wave's
// memory instructions queue in order behind its own prefetch, the partial stores left 1.5 us and the gather 0.5 us later (kernel
// 13.8 us, still 2.4 us/layer better than two launches).
// GU (the gate/up rows follow in this launch, gateup_phase): the rounded rows are parked in `sm_pub` for the block's publishing wave
template <int NVW, int R, bool GU = false>
__device__ __forceinline__ void oproj_phase(const AttnStepArgs& a, u32x4* sm_x, unsigned tag, int lane, int wave, int o_row0,
                                            unsigned long long* tr, uint16_t* sm_pub = nullptr, int pub_row0 = 0) {
    u32x4 ow[R][NVW];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int row = min(o_row0 + r, a.o_rows - 1);                           // clamp: surplus waves re-read a valid row
        const u32x4* p = reinterpret_cast<const u32x4*>(a.o_w + (size_t)row * (NVW * 512));
#pragma unroll
        for (int j = 0; j < NVW; ++j) ow[r][j] = __builtin_nontemporal_load(p + j * 64 + lane);
    }
    bf16_t o_res[R];
#pragma unroll
    for (int r = 0; r < R; ++r) o_res[r] = a.o_resid[min(o_row0 + r, a.o_rows - 1)];
    __builtin_amdgcn_sched_barrier(0);   // keep the loads HERE: the scheduler would sink them to their use
    oproj_await_vector<NVW>(a, sm_x, tag, lane, wave);
    if (tr && threadIdx.x == 0) tr[5] = wall_clock64();
    float acc[R];
    rows_dot<false, R, NVW>(ow, sm_x, lane, acc);
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (o_row0 + r < a.o_rows) {
                if (a.o_out_f32) a.o_out_f32[o_row0 + r] = acc[r];   // the O GEMV's EPI_F32: this rank's partial, un-rounded
                else {
                    const bf16_t hb = f32_to_bf16(bf16_to_f32(o_res[r]) + round_bf16(acc[r]));
                    a.o_out[o_row0 + r] = hb;
                    if (GU) sm_pub[o_row0 + r - pub_row0] = hb;
                }
            }
    }
    if (tr && threadIdx.x == 0) tr[6] = wall_clock64();
}


// The same phase on a 4-bit packed O matrix (quant.hip qgemv_kernel<4, 4, PRO_NONE, EPI_RESIDUAL, 2, true>: 32 elements per lane and
// step, interleaved scale | bias words): a row is NVW / 4 steps of one 16-byte weight load + one 4-byte scale/bias load per lane.
// The attention vector is re-paired in LDS the way that kernel's prologue stores it ((x0,x2) (x4,x6) (x1,x3) (x5,x7) per 8
// elements) with the per-32 sums next to it; nibble unpack, v_dot2c order and the scale / bias fmas are that kernel's, so the
// residual stream is bit-identical to the two-launch step.
template <int NVW, int R>
__device__ __forceinline__ void oproj_phase_q4(const AttnStepArgs& a, u32x4* sm_x, float* sm_xsum, unsigned tag, int lane, int wave,
                                               int o_row0, unsigned long long* tr) {
    static_assert(NVW % 4 == 0, "K must be a multiple of 2048");
    constexpr int ST = NVW / 4;
    u32x4 ow[R][ST];
    uint32_t sbv[R][ST];
    const int words_per_row = NVW * 64, groups_per_row = NVW * 512 / a.o_group;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int row = min(o_row0 + r, a.o_rows - 1);
        const uint32_t* p = a.o_wq + (size_t)row * words_per_row;
        const uint32_t* psb = a.o_sb + (size_t)row * groups_per_row;
#pragma unroll
        for (int st = 0; st < ST; ++st) {
            const int chunk = st * 64 + lane;
            ow[r][st] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p + (size_t)chunk * 4));
            sbv[r][st] = psb[chunk * 32 / a.o_group];
        }
    }
    bf16_t o_res[R];
#pragma unroll
    for (int r = 0; r < R; ++r) o_res[r] = a.o_resid[min(o_row0 + r, a.o_rows - 1)];
    __builtin_amdgcn_sched_barrier(0);
    oproj_await_vector<NVW>(a, sm_x, tag, lane, wave);
    // re-pair + per-chunk sums: thread t owns the 8 elements of vector t (whole waves: NVW * 64 threads)
    if ((int)threadIdx.x < NVW * 64) {
        const u32x4 o = sm_x[threadIdx.x];
        u32x4 t;
        t[0] = __builtin_amdgcn_perm(o[1], o[0], 0x05040100u); t[1] = __builtin_amdgcn_perm(o[3], o[2], 0x05040100u);
        t[2] = __builtin_amdgcn_perm(o[1], o[0], 0x07060302u); t[3] = __builtin_amdgcn_perm(o[3], o[2], 0x07060302u);
        sm_x[threadIdx.x] = t;
        float sv = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) sv += bf16lo(o[q]) + bf16hi(o[q]);
        sv += dpp_f<kDppXor1>(sv);
        sv += dpp_f<kDppXor2>(sv);
        if ((threadIdx.x & 3) == 0) sm_xsum[threadIdx.x >> 2] = sv;
    }
    __syncthreads();
    if (tr && threadIdx.x == 0) tr[5] = wall_clock64();
    float acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.f;
#pragma unroll
    for (int st = 0; st < ST; ++st) {
        const int chunk = st * 64 + lane;
        uint32_t xp[16];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const u32x4 xv = sm_x[chunk * 4 + j];
#pragma unroll
            for (int q = 0; q < 4; ++q) xp[j * 4 + q] = xv[q];
        }
        const float xsm = sm_xsum[chunk];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float d = 0.f;
            const float scl = bf16lo(sbv[r][st]);
            float bia = bf16hi(sbv[r][st]);
#pragma unroll
            for (int wi = 0; wi < 4; ++wi) {
                const uint32_t wdw = ow[r][st][wi];
                const uint32_t lo = wdw & 0x0F0F0F0Fu, hi = (wdw >> 4) & 0x0F0F0F0Fu;
                const uint32_t c43 = 0x43434343u;
                const uint32_t q0 = __builtin_amdgcn_perm(c43, lo, 0x04010400u), q1 = __builtin_amdgcn_perm(c43, lo, 0x04030402u);
                const uint32_t q2 = __builtin_amdgcn_perm(c43, hi, 0x04010400u), q3 = __builtin_amdgcn_perm(c43, hi, 0x04030402u);
                d = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, xp[wi * 4 + 0]), __builtin_bit_cast(bf16x2_t, q0), d, false);
                d = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, xp[wi * 4 + 1]), __builtin_bit_cast(bf16x2_t, q1), d, false);
                d = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, xp[wi * 4 + 2]), __builtin_bit_cast(bf16x2_t, q2), d, false);
                d = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, xp[wi * 4 + 3]), __builtin_bit_cast(bf16x2_t, q3), d, false);
            }
            bia = fmaf(-128.0f, scl, bia);
            acc[r] = fmaf(scl, d, acc[r]);
            acc[r] = fmaf(bia, xsm, acc[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = wave_sum(acc[r]);
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (o_row0 + r < a.o_rows) a.o_out[o_row0 + r] = f32_to_bf16(bf16_to_f32(o_res[r]) + round_bf16(acc[r]));
    }
    if (tr && threadIdx.x == 0) tr[6] = wall_clock64();
}


template <int D, int GT, bool TRACE, int NVW, bool F16 = false, bool GU = false, bool DN = false>
__global__ __launch_bounds__(kBlock, 1) void attn_step_kernel(const AttnStepArgs a) {
    static_assert(!DN || GU, "down + the next q/k/v follow gate/up only");
    static_assert(!F16 || NVW == 0, "the O projection rides in the launch for bfloat16 models only");
    static_assert(!GU || (NVW == kGuNV && D == 128), "gate/up follows the bf16 O projection of hidden 4096 only");
    typedef Act16<F16> A16;
    constexpr int LPR = D / 8;            // lanes per K/V row
    constexpr int TPW = 64 / LPR;         // token rows per wave-instruction == one unit
    constexpr bool QO = NVW >= 100;       // 100 + n: the O matrix is 4-bit packed (oproj_phase_q4)
    constexpr int NV = QO ? NVW - 100 : NVW;
    constexpr bool OPROJ = NV > 0;        // K = H * D = NV * 512
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* sm_o = reinterpret_cast<float*>(smem);                 // [kWaves][TPW][GT][D]
    float* sm_m = sm_o + kWaves * TPW * GT * D;                   // [kWaves][GT]
    float* sm_l = sm_m + kWaves * GT;                             // [kWaves][GT]
    u32x4* sm_q = reinterpret_cast<u32x4*>(sm_l + kWaves * GT);   // [GT + 1][LPR]: roped q heads and the new k row, packed bf16
    u32x4* sm_x = sm_q + (GT + 1) * LPR;                          // OPROJ: [NV * 64] the attention vector, packed bf16
    float* sm_xsum = reinterpret_cast<float*>(sm_x + NV * 64);    // QO: [NV * 16] sums of 32 consecutive elements
    int* sm_gu = reinterpret_cast<int*>(sm_x + NV * 64);          // GU: [kGuWords] the gate/up phase's ticket counter and TRACE count

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int c = lane % LPR;             // 8-element chunk of the head dim owned by this lane
    const int sg = lane / LPR;            // token row inside the unit
    const int kvh = blockIdx.x, split = blockIdx.y;
    const int G = a.H / a.Hkv;
    unsigned long long* tr = TRACE ? a.trace + ((size_t)split * a.Hkv + kvh) * kAttnTraceWords : nullptr;
    if (TRACE && threadIdx.x == 0) tr[0] = wall_clock64();
    if constexpr (GU) {   // (every wave passes the barrier below before it draws a ticket)
        if (threadIdx.x < (DN ? kDnWords : kGuWords)) sm_gu[threadIdx.x] = 0;
    }

    bf16_t* Kb = a.k + (size_t)kvh * a.kv_head_stride;
    bf16_t* Vb = a.v + (size_t)kvh * a.kv_head_stride;
    const int t_begin = split * a.chunk;
    const int n_units = a.chunk / TPW;

    // ---- ONE round of loads: nothing below depends on the position ----
    const bf16_t* kraw = a.qkv + (size_t)a.H * D + (size_t)kvh * D;
    const bool does_q = wave < GT, does_k = wave == GT % kWaves;
    // the row this wave normalises: query head `wave` (clamped) or, for the key wave without a query head, the new key row
    const bf16_t* my_raw = does_q ? a.qkv + (size_t)(kvh * G + min(wave, G - 1)) * D : kraw;
    const u32x4 raw0 = *reinterpret_cast<const u32x4*>(my_raw + c * 8);
    const u32x4 raw1 = *reinterpret_cast<const u32x4*>(kraw + c * 8);                        // (key wave that also owns a head)
    const u32x4 vnew = *reinterpret_cast<const u32x4*>(kraw + (size_t)a.Hkv * D + c * 8);
    const int i0 = (c % (LPR / 2)) * 8;
    const f32x4* cp = reinterpret_cast<const f32x4*>(a.rope_cur + i0);
    const f32x4* sp = reinterpret_cast<const f32x4*>(a.rope_cur + D / 2 + i0);
    const f32x4 c0 = cp[0], c1 = cp[1], s0 = sp[0], s1 = sp[1];
    u32x4 wq_raw = {0, 0, 0, 0}, wk_raw = {0, 0, 0, 0};
    if (a.q_norm_w) {
        wq_raw = *reinterpret_cast<const u32x4*>(a.q_norm_w + c * 8);
        wk_raw = *reinterpret_cast<const u32x4*>(a.k_norm_w + c * 8);
    }
    u32x4 kr[kKU], vr[kKU];
    auto issue_kv = [&](int u0) {
#pragma unroll
        for (int u = 0; u < kKU; ++u) {
            const int tc = min(t_begin + (u0 + u * kWaves) * TPW + sg, a.cap - 1);   // rows past the position are masked below
            kr[u] = *reinterpret_cast<const u32x4*>(Kb + (size_t)tc * D + c * 8);
            vr[u] = *reinterpret_cast<const u32x4*>(Vb + (size_t)tc * D + c * 8);
        }
    };
    issue_kv(wave);
    const int pos = *a.pos_ptr;                                    // tokens already cached == RoPE offset (model.rs:186-194)
    const unsigned tag = *a.seq_ptr * a.tag_mul + a.tag_add;

    // ---- per-head RMSNorm (optional) + RoPE with the reference's bf16 roundings: one row per wave, shared through LDS ----
    {
        float cs[8], sn[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            cs[e] = c0[e]; cs[4 + e] = c1[e];
            sn[e] = s0[e]; sn[4 + e] = s1[e];
        }
        const bool first_half = c < LPR / 2;
        auto norm_rope = [&](const u32x4 raw, const u32x4 w_raw) -> u32x4 {
            float x[8], w[8];
            unpack8<F16>(raw, x);
            unpack8<F16>(w_raw, w);
            float ss = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) ss = fmaf(x[e], x[e], ss);
            ss = group_sum<LPR>(ss);
            const float rstd = a.q_norm_w ? 1.0f / sqrtf(ss / (float)D + a.eps) : 1.0f;   // no q/k norm (Mixtral, Qwen2): x goes to RoPE as it is
            float y[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float xn = a.q_norm_w ? A16::rnd(x[e] * rstd * w[e]) : x[e];   // RMSNorm output is rounded to the model's dtype
                const float other = swap_halves<LPR>(xn);                               // element i +- D/2
                y[e] = first_half ? xn * cs[e] - other * sn[e] : other * sn[e] + xn * cs[e];
            }
            u32x4 out;
#pragma unroll
            for (int e = 0; e < 4; ++e) out[e] = A16::pack(y[2 * e], y[2 * e + 1]);     // RoPE output likewise
            return out;
        };
        if (does_q && sg == 0) sm_q[wave * LPR + c] = norm_rope(raw0, wq_raw);
        if (does_k && sg == 0) sm_q[GT * LPR + c] = norm_rope(does_q ? raw1 : raw0, wk_raw);
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // LDS only: the K/V loads stay in flight across it
    u32x4 q[GT];
#pragma unroll
    for (int g = 0; g < GT; ++g) q[g] = sm_q[g * LPR + c];
    const u32x4 knew = sm_q[GT * LPR + c];

    const int Tk = pos + 1;
    const int n_active = (Tk + a.chunk - 1) / a.chunk;                  // splits that own at least one token
    const int t_end = min(Tk, t_begin + a.chunk);
    const bool active = split < n_active;
    if (TRACE && threadIdx.x == 0) tr[1] = wall_clock64();

    float m[GT], l[GT];
    f32x2 o[GT][4];
#pragma unroll
    for (int g = 0; g < GT; ++g) {
        m[g] = -INFINITY;
        l[g] = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[g][e] = f32x2{0.f, 0.f};
    }
    // one round = the kKU units a wave holds in registers.  The FIRST round is straight-line code ahead of the loop: hipcc's waitcnt
    // pass counts loads exactly there, so its waits on the K/V rows do not cover the O-projection weights issued after them (inside
    // the loop it falls back to small counts that drain everything older: own-chunk time went from 1.2 to 2.9 us)
    auto round = [&](const int u0) {
        float s[kKU][GT];
        f32x2 vf[kKU][4];
#pragma unroll
        for (int u = 0; u < kKU; ++u) {
            const int unit = u0 + u * kWaves;
            const int tok = t_begin + unit * TPW + sg;
            const bool live = unit < n_units && tok < t_end;
            u32x4 kp = kr[u], vp = vr[u];
            if (tok == pos && unit < n_units) {
                // this lane group owns the NEW token: use the row built above and append it to the cache (cache.rs:183-188)
                kp = knew;
                vp = vnew;
                *reinterpret_cast<u32x4*>(Kb + (size_t)pos * D + c * 8) = kp;
                *reinterpret_cast<u32x4*>(Vb + (size_t)pos * D + c * 8) = vp;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)   // a row past the position: its p is 0, but 0 * garbage must stay 0
                vf[u][e] = live ? f32x2{A16::lo(vp[e]), A16::hi(vp[e])} : f32x2{0.f, 0.f};
#pragma unroll
            for (int g = 0; g < GT; ++g) {
                const float d = group_sum<LPR>(dot8_16<F16>(q[g], kp)) * a.scale;
                s[u][g] = live ? d : -INFINITY;
            }
        }
        if (u0 + kWaves * kKU < n_units && t_begin + (u0 + kWaves * kKU) * TPW < t_end) issue_kv(u0 + kWaves * kKU);
#pragma unroll
        for (int g = 0; g < GT; ++g) {                  // one running max per head for the whole wave
            float mx = s[0][g];
#pragma unroll
            for (int u = 1; u < kKU; ++u) mx = fmaxf(mx, s[u][g]);
            float wmx = readlane_f(mx, 0);
#pragma unroll
            for (int r = 1; r < TPW; ++r) wmx = fmaxf(wmx, readlane_f(mx, r * LPR));
            const float mn = fmaxf(m[g], wmx);
            const float alpha = (mn == -INFINITY) ? 1.f : __expf(m[g] - mn);
            m[g] = mn;
            l[g] *= alpha;
            const f32x2 al = {alpha, alpha};
#pragma unroll
            for (int e = 0; e < 4; ++e) o[g][e] *= al;
#pragma unroll
            for (int u = 0; u < kKU; ++u) {
                const float p = (mn == -INFINITY) ? 0.f : __expf(s[u][g] - mn);
                l[g] += p;
                const f32x2 pp = {p, p};
#pragma unroll
                for (int e = 0; e < 4; ++e) o[g][e] = __builtin_elementwise_fma(pp, vf[u][e], o[g][e]);
            }
        }
    };
    if (wave < n_units && t_begin + wave * TPW < t_end) round(wave);
    for (int u0 = wave + kWaves * kKU; u0 < n_units && t_begin + u0 * TPW < t_end; u0 += kWaves * kKU) round(u0);
    if (TRACE && threadIdx.x == 0) tr[2] = wall_clock64();

    if (active) {
        // ---- every token row of every wave parks its partial in LDS (same m inside a wave: plain sums) ----
#pragma unroll
        for (int g = 0; g < GT; ++g) {
            float* dst = sm_o + (((size_t)(wave * TPW + sg) * GT + g) * D + c * 8);
            *reinterpret_cast<f32x4*>(dst) = f32x4{o[g][0][0], o[g][0][1], o[g][1][0], o[g][1][1]};
            *reinterpret_cast<f32x4*>(dst + 4) = f32x4{o[g][2][0], o[g][2][1], o[g][3][0], o[g][3][1]};
            float lw = readlane_f(l[g], 0);   // the LPR lanes of a row hold identical l
#pragma unroll
            for (int r = 1; r < TPW; ++r) lw += readlane_f(l[g], r * LPR);
            if (lane == 0) {
                sm_m[wave * GT + g] = m[g];
                sm_l[wave * GT + g] = lw;
            }
        }
        __syncthreads();
        if (TRACE && !GU && threadIdx.x == 0) tr[7] = wall_clock64();   // (GU: the stamp marks the first reduced pair instead)
        // ---- merge the 8 waves x TPW rows; the split's partial leaves as tagged granules ----
        for (int idx = threadIdx.x; idx < G * D; idx += kBlock) {
            const int g = idx / D, d = idx % D;
            float M = sm_m[g];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) M = fmaxf(M, sm_m[w * GT + g]);
            float L = 0.f, O = 0.f;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) {
                const float mw = sm_m[w * GT + g];
                const float f = (mw == -INFINITY) ? 0.f : __expf(mw - M);
                float ow = 0.f;
#pragma unroll
                for (int r = 0; r < TPW; ++r) ow += sm_o[((size_t)(w * TPW + r) * GT + g) * D + d];
                L = fmaf(f, sm_l[w * GT + g], L);
                O = fmaf(f, ow, O);
            }
            uint64_t* gr = a.ws + ((size_t)(kvh * G + g) * a.nsplit + split) * (D + 2);
            st_granule(gr + d, tag, O);
            if (d == 0) {
                st_granule(gr + D, tag, M);
                st_granule(gr + D + 1, tag, L);
            }
        }
    }
    if (TRACE && threadIdx.x == 0) tr[3] = wall_clock64();

    // ---- OPROJ: the blocks that are not consumers (split >= G) share the output rows; rows per wave is a compile-time constant of the
    //      phase (a runtime-predicated load block per row made hipcc drain the queue between rows: three serial round trips) ----
    if (OPROJ && split >= G) {
        // wave g of the (blocks - H) * 8 producer waves: the first o_nhi waves take o_rpw rows, the others o_rpw - 1 -- together exactly
        // o_rows (with o_rpw rows everywhere the surplus waves re-read the last row: 44 MB of traffic for a 33.6 MB matrix)
        const int g = ((split - G) * (int)gridDim.x + kvh) * kWaves + wave;
        const bool hi = g < a.o_nhi;
        const int rows = hi ? a.o_rpw : a.o_rpw - 1;
        const int o_row0 = hi ? g * a.o_rpw : a.o_nhi * a.o_rpw + (g - a.o_nhi) * (a.o_rpw - 1);
        unsigned long long* otr = TRACE ? tr : nullptr;
        if constexpr (GU) {
            // the block's eight waves hold consecutive rows: from where, and how many (wave 0 publishes them)
            auto row0_of = [&](int w) { return w < a.o_nhi ? w * a.o_rpw : a.o_nhi * a.o_rpw + (w - a.o_nhi) * (a.o_rpw - 1); };
            const int pub_row0 = row0_of(g - wave), pub_rows = row0_of(g - wave + kWaves) - pub_row0;
            uint16_t* sm_pub = reinterpret_cast<uint16_t*>(sm_l);   // (the split merge is done with sm_m / sm_l: a block barrier ago)
            if (rows == 2) oproj_phase<NV, 2, true>(a, sm_x, tag, lane, wave, o_row0, otr, sm_pub, pub_row0);
            else oproj_phase<NV, 3, true>(a, sm_x, tag, lane, wave, o_row0, otr, sm_pub, pub_row0);
            gateup_phase<TRACE, DN, true>(a, sm_x, sm_m, sm_gu, sm_pub, tag, lane, wave, pub_row0, pub_rows, otr, smem);
            return;
        } else
        if constexpr (QO) {
            if (rows <= 1) oproj_phase_q4<NV, 1>(a, sm_x, sm_xsum, tag, lane, wave, o_row0, otr);
            else if (rows == 2) oproj_phase_q4<NV, 2>(a, sm_x, sm_xsum, tag, lane, wave, o_row0, otr);
            else if (rows == 3) oproj_phase_q4<NV, 3>(a, sm_x, sm_xsum, tag, lane, wave, o_row0, otr);
            else oproj_phase_q4<NV, 4>(a, sm_x, sm_xsum, tag, lane, wave, o_row0, otr);
        } else {
            if (rows <= 1) oproj_phase<(NV > 0 ? NV : 1), 1>(a, sm_x, tag, lane, wave, o_row0, otr);
            else if (rows == 2) oproj_phase<(NV > 0 ? NV : 1), 2>(a, sm_x, tag, lane, wave, o_row0, otr);
            else if (rows == 3) oproj_phase<(NV > 0 ? NV : 1), 3>(a, sm_x, tag, lane, wave, o_row0, otr);
            else oproj_phase<(NV > 0 ? NV : 1), 4>(a, sm_x, tag, lane, wave, o_row0, otr);
        }
        return;
    }

    // ---- consumers: block (kvh, j < G) merges head kvh*G + j ----
    if (split < G && wave < D / 64) {
        const int head = kvh * G + split;
        const uint64_t* base = a.ws + (size_t)head * a.nsplit * (D + 2);
        bf16_t* out = a.out + (size_t)head * D;
        const int dim = wave * 64 + lane;
        const int nb = (a.nsplit + 15) / 16;
        uint64_t* xg_head = OPROJ ? a.xg + (size_t)head * (D / 2) : nullptr;
        if (nb <= 1) gather_head<D, 1, F16>(a, base, n_active, tag, lane, dim, out, xg_head);
        else if (nb == 2) gather_head<D, 2, F16>(a, base, n_active, tag, lane, dim, out, xg_head);
        else gather_head<D, 3, F16>(a, base, n_active, tag, lane, dim, out, xg_head);
        if (TRACE && threadIdx.x == 0) tr[4] = wall_clock64();
    }
    if constexpr (GU) {
        // the consumer blocks take their share of the pairs once their heads are merged and published (block-uniform: split < G here)
        lds_barrier();
        gateup_phase<TRACE, DN, false>(a, sm_x, sm_m, sm_gu, nullptr, tag, lane, wave, 0, 0, TRACE ? tr : nullptr, smem);
    }
}

}  // namespace

int attn_step_block_tokens(int D) { return 64 / (D / 8); }   // granularity of a split's token range: one wave-instruction

// token range per split and split count for a context bucket of `tk_max` tokens: one block per CU (<= 256 blocks: every block
// of the launch is resident, the consumers cannot starve a producer), at most kMaxSplits splits (the consumer gathers 3
// batches of 16), at least G (one consumer block per query head of a KV group)
constexpr int kMaxSplits = 48;
void attn_step_plan(int tk_max, int Hkv, int G, int D, int* chunk, int* nsplit) {
    const int unit = attn_step_block_tokens(D);
    int target = std::max(1, std::min(kMaxSplits, 256 / std::max(Hkv, 1)));
    if (const char* v = getenv("OMX_ATTN_STEP_SPLITS")) target = std::max(1, std::min(kMaxSplits, atoi(v)));
    int ch = unit * ((tk_max + unit * target - 1) / (unit * target));
    if (ch < unit) ch = unit;
    int ns = (tk_max + ch - 1) / ch;
    if (ns < G) ns = G;
    *chunk = ch;
    *nsplit = ns;
}

size_t attn_step_ws_granules(int H, int D) { return (size_t)H * kMaxSplits * (D + 2); }

// rows per wave when the waves of the non-consumer blocks (split >= G: blocks - H of them) share the O projection's output rows
static int oproj_rows_per_wave(int H, int Hkv, int nsplit, int o_rows) {
    const int waves = (Hkv * nsplit - H) * kWaves;
    return waves > 0 ? (o_rows + waves - 1) / waves : 1 << 20;
}
// the O projection can ride in the launch when K = H * D is one of the register layouts (NVW x 512, NVW in {1, 2, 4, 7, 8}: the
// GEMV instantiations gemv_kernel<NVW, 1, ...> whose arithmetic the phase reproduces; 7 = Qwen2.5-7B's 28 heads of 128) and at most
// kORows rows per wave of the non-consumer blocks cover the output
bool attn_step_oproj_ok(int H, int Hkv, int D, int nsplit, int o_rows) {
    const int K = H * D, nvw = K / 512;
    return K % 512 == 0 && (nvw == 1 || nvw == 2 || nvw == 4 || nvw == 7 || nvw == 8) && oproj_rows_per_wave(H, Hkv, nsplit, o_rows) <= kORows;
}

// ... on a 4-bit packed matrix: K a multiple of 2048 (quant.hip's four-word lane chunk) with the register layouts 4 and 8
bool attn_step_oproj_q4_ok(int H, int Hkv, int D, int nsplit, int o_rows, int group) {
    const int K = H * D;
    return (K == 2048 || K == 4096) && (group == 32 || group == 64 || group == 128) && attn_step_oproj_ok(H, Hkv, D, nsplit, o_rows);
}

// ... and [RMSNorm + gate/up + SwiGLU] behind it: the one shape whose 256 blocks take kGuBlockPairs (gate, up) pairs each, every
// O block holding whole granules (two or three rows per wave, the three-row waves filling whole blocks)
bool attn_step_gateup_ok(int H, int Hkv, int D, int nsplit, int o_rows, int gu_rows) {
    const int blocks = Hkv * nsplit, waves = (blocks - H) * kWaves;
    if (D != 128 || H * D != kGuHidden || o_rows != kGuHidden || H / std::max(Hkv, 1) != 4 || blocks != 256) return false;
    if (gu_rows != blocks * kGuBlockPairs || !attn_step_oproj_ok(H, Hkv, D, nsplit, o_rows)) return false;
    return oproj_rows_per_wave(H, Hkv, nsplit, o_rows) == 3 && (o_rows - waves * 2) % kWaves == 0;
}

// ... and [down + residual] + the next layer's [RMSNorm + q/k/v] behind that: gate/up's shape (256 blocks, hidden 4096) with sixteen down
// rows a block over the intermediate size the units are cut for, and three q/k/v rows a wave covering the next layer's rows exactly as
// gemv_chain.hip's waves do
bool attn_step_down_ok(int o_rows, int gu_rows, int nq_rows) {
    const int waves = 256 * kWaves;
    return o_rows == 256 * kDnBlockRows && gu_rows == kDnInter && nq_rows > (kDnQRows - 1) * waves && nq_rows <= kDnQRows * waves;
}

// one instantiation's launch: the dynamic-LDS attribute where the block needs more than the default 48 KB, the (timed or recorded) launch
template <int D, int GT, bool TRACE, int NVW, bool F16 = false, bool GU = false, bool DN = false>
static int launch_instance(dim3 grid, size_t shmem, hipStream_t s, const AttnStepArgs& a) {
    if (shmem > 48 * 1024)
        OMX_HIP_CHECK(hipFuncSetAttribute((const void*)attn_step_kernel<D, GT, TRACE, NVW, F16, GU, DN>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
    OMX_LAUNCH_TIMED((attn_step_kernel<D, GT, TRACE, NVW, F16, GU, DN>), grid, dim3(kBlock), shmem, s, a);
    OMX_LAUNCH_CHECK();
    return 0;
}

int launch_attn_step(const AttnStepArgs& a_in, int D, hipStream_t s) {
    AttnStepArgs a = a_in;
    const int G = a.H / a.Hkv;
    OMX_REQUIRE(a.H % a.Hkv == 0 && G >= 1 && G <= 8, "decode attention: %d query heads over %d KV heads unsupported (group of at most 8)", a.H, a.Hkv);
    OMX_REQUIRE(a.nsplit >= G && a.nsplit <= kMaxSplits && a.chunk > 0 && a.chunk % attn_step_block_tokens(D) == 0 && a.Hkv * a.nsplit <= 256,
                "decode attention: bad split plan (chunk %d, %d splits, group %d, %d kv heads)", a.chunk, a.nsplit, G, a.Hkv);
    OMX_REQUIRE(a.ws && a.rope_cur && a.pos_ptr && a.seq_ptr && a.abort_flag && a.tag_mul > a.tag_add - 1u && a.tag_add >= 1u,
                "decode attention: missing step state");
    int nvw = 0;
    const bool qo = a.o_wq != nullptr;
    if (qo)
        OMX_REQUIRE(!a.o_w && a.o_sb && a.o_out && !a.o_out_f32 && attn_step_oproj_q4_ok(a.H, a.Hkv, D, a.nsplit, a.o_rows, a.o_group),
                    "decode attention + packed O projection: shape does not qualify (H*D = %d, group %d)", a.H * D, a.o_group);
    if (a.o_w || qo) {
        OMX_REQUIRE(a.o_resid && (a.o_out || a.o_out_f32) && a.xg && attn_step_oproj_ok(a.H, a.Hkv, D, a.nsplit, a.o_rows),
                    "decode attention + O projection: shape does not qualify (H*D = %d, %d rows, %d blocks)", a.H * D, a.o_rows, a.Hkv * a.nsplit);
        nvw = a.H * D / 512;
        a.o_rpw = oproj_rows_per_wave(a.H, a.Hkv, a.nsplit, a.o_rows);
        const int waves = (a.Hkv * a.nsplit - a.H) * kWaves;
        // o_nhi waves with o_rpw rows + the rest with o_rpw - 1 = o_rows; with one row per wave at most (o_rpw == 1) every wave keeps
        // its (possibly clamped) row: a wave of the phase always holds at least one
        a.o_nhi = a.o_rpw > 1 ? a.o_rows - waves * (a.o_rpw - 1) : waves;
    }
    if (a.gu_gate)
        OMX_REQUIRE(a.o_w && a.o_out && !a.o_out_f32 && !a.f16 && a.gu_up && a.gu_norm_w && a.gu_out && a.hg &&
                        attn_step_gateup_ok(a.H, a.Hkv, D, a.nsplit, a.o_rows, a.gu_rows),
                    "decode attention + gate/up: shape does not qualify (%d blocks, %d O rows, %d pairs)", a.Hkv * a.nsplit, a.o_rows, a.gu_rows);
    if (a.dn_w)
        OMX_REQUIRE(a.gu_gate && a.dn_out && a.ag && a.rg && a.nq.w0 && a.nq.w1 && a.nq.w2 && a.nq_norm_w && a.nq_out &&
                        a.nq.n0 > 0 && a.nq.n1 > 0 && a.nq.rows > a.nq.n0 + a.nq.n1 && attn_step_down_ok(a.o_rows, a.gu_rows, a.nq.rows),
                    "decode attention + down + q/k/v: shape does not qualify (%d rows, %d pairs, %d q/k/v rows)", a.o_rows, a.gu_rows, a.nq.rows);
    const dim3 grid(a.Hkv, a.nsplit);
    const int gt = G <= 1 ? 1 : G <= 2 ? 2 : G <= 4 ? 4 : 8;
#define OMX_ATTN_STEP_CASE(DD, GG)                                                                                       \
    if (D == DD && gt == GG) {                                                                                           \
        const size_t shmem = ((size_t)kWaves * (64 / (DD / 8)) * GG * DD + 2 * kWaves * GG) * sizeof(float) +            \
                             (size_t)(GG + 1) * (DD / 8) * 16 + (size_t)nvw * 64 * 16 + (qo ? (size_t)nvw * 64 : 0) +    \
                             (a.dn_w ? kDnWords * sizeof(int) : a.gu_gate ? kGuWords * sizeof(int) : 0);                 \
        if (a.gu_gate) {   /* gate/up behind the O projection: one shape (attn_step_gateup_ok) */                         \
            if constexpr (DD == 128 && GG == 4) {                                                                        \
                static_assert(kDnLdsBytes <= kWaves * 4 * 4 * 128 * 4, "the down phase lives in the split-merge area");  \
                if (a.dn_w && a.trace) return launch_instance<128, 4, true, kGuNV, false, true, true>(grid, shmem, s, a); \
                if (a.dn_w) return launch_instance<128, 4, false, kGuNV, false, true, true>(grid, shmem, s, a);          \
                if (a.trace) return launch_instance<128, 4, true, kGuNV, false, true>(grid, shmem, s, a);                \
                return launch_instance<128, 4, false, kGuNV, false, true>(grid, shmem, s, a);                            \
            }                                                                                                            \
            return set_error("decode attention + gate/up: no instantiation for head_dim %d, group %d", DD, GG);         \
        }                                                                                                                \
        if (a.trace && !qo) {   /* timeline builds: the plain kernel and the widest fused one */                        \
            if (nvw == 0) return launch_instance<DD, GG, true, 0>(grid, shmem, s, a);                                    \
            if (nvw == 8) return launch_instance<DD, GG, true, 8>(grid, shmem, s, a);                                    \
            return set_error("decode attention: no traced instantiation for H*D = %d", a.H * DD);                       \
        }                                                                                                                \
        if (qo) {                                                                                                        \
            if (nvw == 4) return launch_instance<DD, GG, false, 104>(grid, shmem, s, a);                                 \
            return launch_instance<DD, GG, false, 108>(grid, shmem, s, a);                                               \
        }                                                                                                                \
        if (a.f16) {   /* a float16 checkpoint's model: float16 q / k / v, cache and output; D = 128, no O projection in the launch */ \
            if constexpr (DD == 128) {                                                                                   \
                if (nvw == 0) return launch_instance<DD, GG, false, 0, true>(grid, shmem, s, a);                         \
            }                                                                                                            \
            return set_error("decode attention: float16 models take head_dim 128 without the O projection in the launch"); \
        }                                                                                                                \
        if (nvw == 0) return launch_instance<DD, GG, false, 0>(grid, shmem, s, a);                                       \
        if (nvw == 1) return launch_instance<DD, GG, false, 1>(grid, shmem, s, a);                                       \
        if (nvw == 2) return launch_instance<DD, GG, false, 2>(grid, shmem, s, a);                                       \
        if (nvw == 4) return launch_instance<DD, GG, false, 4>(grid, shmem, s, a);                                       \
        if (nvw == 7) return launch_instance<DD, GG, false, 7>(grid, shmem, s, a);                                       \
        return launch_instance<DD, GG, false, 8>(grid, shmem, s, a);                                                     \
    }
    OMX_ATTN_STEP_CASE(128, 1) OMX_ATTN_STEP_CASE(128, 2) OMX_ATTN_STEP_CASE(128, 4) OMX_ATTN_STEP_CASE(128, 8)
    OMX_ATTN_STEP_CASE(64, 1) OMX_ATTN_STEP_CASE(64, 2) OMX_ATTN_STEP_CASE(64, 4) OMX_ATTN_STEP_CASE(64, 8)
#undef OMX_ATTN_STEP_CASE
    return set_error("decode attention: head_dim %d unsupported (64 or 128)", D);
}

}  // namespace omx
