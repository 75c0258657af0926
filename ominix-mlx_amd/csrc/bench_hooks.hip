// Measurement hooks (not part of the drop-in surface): time one kernel family with HIP events on
// the stream it is launched on.  Weight buffers are rotated through `n_copies` distinct
// allocations so that the 256 MiB Infinity Cache cannot serve re-reads (MI355X_MICROARCH.md).
#include <algorithm>
#include <vector>

#include "gemm.hpp"
#include "gemv.hpp"
#include "attn.hpp"

extern "C" int omx_bench_gemv(int N, int K, int pro, int epi, int rows_per_wave, int n_copies, int iters,
                              float* avg_ms) {
    using namespace omx;
    OMX_REQUIRE(avg_ms && n_copies > 0 && iters > 0, "omx_bench_gemv: bad arguments");
    const int mats = (epi == EPI_SWIGLU) ? 2 : 1;
    const size_t wbytes = (size_t)N * K * 2 * mats;
    std::vector<void*> w(n_copies, nullptr);
    void *x = nullptr, *nw = nullptr, *out = nullptr, *resid = nullptr, *slot = nullptr;
    for (auto& p : w) {
        OMX_HIP_CHECK(hipMalloc(&p, wbytes));
        if (omx_fill_uniform(p, wbytes / 2, 17u + (uint32_t)(&p - &w[0]), 0.03f, 0.f, OMX_BFLOAT16, nullptr)) return 1;
    }
    OMX_HIP_CHECK(hipMalloc(&x, (size_t)K * 2));
    OMX_HIP_CHECK(hipMalloc(&nw, (size_t)K * 2));
    OMX_HIP_CHECK(hipMalloc(&out, (size_t)N * 4));
    OMX_HIP_CHECK(hipMalloc(&resid, (size_t)N * 2));
    OMX_HIP_CHECK(hipMalloc(&slot, 8 * 65536));
    omx_fill_uniform(x, K, 3, 1.0f, 0.f, OMX_BFLOAT16, nullptr);
    omx_fill_uniform(nw, K, 4, 0.1f, 1.f, OMX_BFLOAT16, nullptr);
    omx_fill_uniform(resid, N, 5, 1.0f, 0.f, OMX_BFLOAT16, nullptr);
    OMX_HIP_CHECK(hipMemset(slot, 0, 8 * 65536));
    hipStream_t s;
    OMX_HIP_CHECK(hipStreamCreate(&s));
    hipEvent_t e0, e1;
    OMX_HIP_CHECK(hipEventCreate(&e0));
    OMX_HIP_CHECK(hipEventCreate(&e1));
    auto run = [&](int i) {
        GemvArgs a = {};
        const bf16_t* base = (const bf16_t*)w[i % n_copies];
        a.w0 = base;
        a.w1 = base + (size_t)N * K;
        a.n0 = N; a.N = N; a.K = K;
        a.x = (const bf16_t*)x;
        a.norm_w = (const bf16_t*)nw;
        a.eps = 1e-6f;
        a.resid = (const bf16_t*)resid;
        a.out = out;
        a.argmax_slot = (unsigned long long*)slot;
        a.rows_per_wave = rows_per_wave;
        return launch_gemv(a, pro, epi, s);
    };
    for (int i = 0; i < n_copies + 2; ++i)
        if (run(i)) return 1;
    OMX_HIP_CHECK(hipStreamSynchronize(s));
    OMX_HIP_CHECK(hipEventRecord(e0, s));
    for (int i = 0; i < iters; ++i)
        if (run(i)) return 1;
    OMX_HIP_CHECK(hipEventRecord(e1, s));
    OMX_HIP_CHECK(hipEventSynchronize(e1));
    float ms = 0.f;
    OMX_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    *avg_ms = ms / iters;
    for (auto p : w) (void)hipFree(p);
    (void)hipFree(x); (void)hipFree(nw); (void)hipFree(out); (void)hipFree(resid); (void)hipFree(slot);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipStreamDestroy(s);
    return 0;
}

// per-block timeline of `chain` back-to-back launches of one GEMV shape on distinct weight buffers (tools/gemv_trace.py):
// host receives [chain][blocks][4] wall-clock stamps (gemv.hpp GemvArgs::trace); *blocks = blocks per launch
extern "C" int omx_bench_gemv_trace(int N, int K, int pro, int epi, int rows_per_wave, int chain, unsigned long long* host,
                                    size_t n_words, int* blocks) {
    using namespace omx;
    OMX_REQUIRE(host && blocks && chain > 0, "omx_bench_gemv_trace: bad arguments");
    const int mats = (epi == EPI_SWIGLU) ? 2 : 1;
    const size_t wbytes = (size_t)N * K * 2 * mats;
    const int nb = gemv_grid(N, K, epi, rows_per_wave);
    OMX_REQUIRE(n_words >= (size_t)chain * nb * 4, "omx_bench_gemv_trace: buffer too small (%d blocks)", nb);
    std::vector<void*> w(chain + 2, nullptr);
    void *x = nullptr, *nw = nullptr, *out = nullptr, *resid = nullptr, *slot = nullptr;
    unsigned long long* tr = nullptr;
    for (auto& p : w) {
        OMX_HIP_CHECK(hipMalloc(&p, wbytes));
        if (omx_fill_uniform(p, wbytes / 2, 17u + (uint32_t)(&p - &w[0]), 0.03f, 0.f, OMX_BFLOAT16, nullptr)) return 1;
    }
    OMX_HIP_CHECK(hipMalloc(&x, (size_t)K * 2));
    OMX_HIP_CHECK(hipMalloc(&nw, (size_t)K * 2));
    OMX_HIP_CHECK(hipMalloc(&out, (size_t)N * 4));
    OMX_HIP_CHECK(hipMalloc(&resid, (size_t)N * 2));
    OMX_HIP_CHECK(hipMalloc(&slot, 8 * 65536));
    OMX_HIP_CHECK(hipMalloc((void**)&tr, (size_t)chain * nb * 4 * 8));
    omx_fill_uniform(x, K, 3, 1.0f, 0.f, OMX_BFLOAT16, nullptr);
    omx_fill_uniform(nw, K, 4, 0.1f, 1.f, OMX_BFLOAT16, nullptr);
    omx_fill_uniform(resid, N, 5, 1.0f, 0.f, OMX_BFLOAT16, nullptr);
    OMX_HIP_CHECK(hipMemset(slot, 0, 8 * 65536));
    OMX_HIP_CHECK(hipMemset(tr, 0, (size_t)chain * nb * 4 * 8));
    OMX_HIP_CHECK(hipDeviceSynchronize());
    hipStream_t s;
    OMX_HIP_CHECK(hipStreamCreate(&s));
    auto run = [&](int i, unsigned long long* t) {
        GemvArgs a = {};
        const bf16_t* base = (const bf16_t*)w[i % w.size()];
        a.w0 = base; a.w1 = base + (size_t)N * K;
        a.n0 = N; a.N = N; a.K = K;
        a.x = (const bf16_t*)x; a.norm_w = (const bf16_t*)nw; a.eps = 1e-6f;
        a.resid = (const bf16_t*)resid; a.out = out;
        a.argmax_slot = (unsigned long long*)slot;
        a.rows_per_wave = rows_per_wave;
        a.trace = t;
        return launch_gemv(a, pro, epi, s);
    };
    for (int i = 0; i < 2; ++i)
        if (run(i, nullptr)) return 1;
    for (int i = 0; i < chain; ++i)
        if (run(2 + i, tr + (size_t)i * nb * 4)) return 1;
    OMX_HIP_CHECK(hipStreamSynchronize(s));
    OMX_HIP_CHECK(hipMemcpy(host, tr, (size_t)chain * nb * 4 * 8, hipMemcpyDeviceToHost));
    *blocks = nb;
    for (auto p : w) (void)hipFree(p);
    (void)hipFree(x); (void)hipFree(nw); (void)hipFree(out); (void)hipFree(resid); (void)hipFree(slot); (void)hipFree(tr);
    (void)hipStreamDestroy(s);
    return 0;
}

// time the bf16 MFMA GEMM out[M,N] = x[M,K] . W[N,K]^T with HIP events (operands rotated over n_copies buffers)
extern "C" int omx_bench_gemm(int M, int N, int K, int n_copies, int iters, float* avg_ms) {
    using namespace omx;
    OMX_REQUIRE(avg_ms && n_copies > 0 && iters > 0, "omx_bench_gemm: bad arguments");
    std::vector<void*> w(n_copies, nullptr), x(n_copies, nullptr);
    void* out = nullptr;
    for (int i = 0; i < n_copies; ++i) {
        OMX_HIP_CHECK(hipMalloc(&w[i], (size_t)N * K * 2));
        OMX_HIP_CHECK(hipMalloc(&x[i], (size_t)M * K * 2));
        // OMX_BENCH_GEMM_DATA=zero | one: constant operands -- what the same instruction stream costs when no operand bit toggles (the chip's
        // power limit, not the kernel, sets the pace of a full-chip GEMM: EXPERIMENTS.md R5-4)
        const char* de = getenv("OMX_BENCH_GEMM_DATA");
        if (de && (de[0] == 'z' || de[0] == 'o')) {
            const int v = de[0] == 'z' ? 0 : 0x3f;      // bytes 0x3f3f = bf16 0.746
            OMX_HIP_CHECK(hipMemset(w[i], v, (size_t)N * K * 2));
            OMX_HIP_CHECK(hipMemset(x[i], v, (size_t)M * K * 2));
            continue;
        }
        if (omx_fill_uniform(w[i], (size_t)N * K, 100 + i, 0.05f, 0.f, OMX_BFLOAT16, nullptr)) return 1;
        if (omx_fill_uniform(x[i], (size_t)M * K, 200 + i, 1.0f, 0.f, OMX_BFLOAT16, nullptr)) return 1;
    }
    OMX_HIP_CHECK(hipMalloc(&out, (size_t)M * N * 2));
    hipStream_t s;
    OMX_HIP_CHECK(hipStreamCreate(&s));
    hipEvent_t e0, e1;
    OMX_HIP_CHECK(hipEventCreate(&e0));
    OMX_HIP_CHECK(hipEventCreate(&e1));
    OMX_HIP_CHECK(hipDeviceSynchronize());
    for (int i = 0; i < 3; ++i)
        if (launch_gemm_bf16((bf16_t*)out, (const bf16_t*)x[i % n_copies], (const bf16_t*)w[i % n_copies], nullptr, M, N, K, s)) return 1;
    OMX_HIP_CHECK(hipEventRecord(e0, s));
    for (int i = 0; i < iters; ++i)
        if (launch_gemm_bf16((bf16_t*)out, (const bf16_t*)x[i % n_copies], (const bf16_t*)w[i % n_copies], nullptr, M, N, K, s)) return 1;
    OMX_HIP_CHECK(hipEventRecord(e1, s));
    OMX_HIP_CHECK(hipEventSynchronize(e1));
    float ms = 0.f;
    OMX_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    *avg_ms = ms / iters;
    for (int i = 0; i < n_copies; ++i) { (void)hipFree(w[i]); (void)hipFree(x[i]); }
    (void)hipFree(out);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipStreamDestroy(s);
    return 0;
}

// ---- device-wide barrier probe (gridsync.hpp): average cost of one exchange + barrier over `iters` ----
#include "gridsync.hpp"
namespace {
// variant 0: gridsync.hpp as shipped (flags + coherent accessors, no fences)
// variant 1: the textbook form it replaced: one atomic counter, agent-scope release/acquire fences
template <int VAR>
__global__ __launch_bounds__(256) void grid_barrier_probe_kernel(unsigned* words, unsigned* counter, unsigned* mismatches,
                                                                 int iters, float* sink) {
    omx::GridSync g{words, 1u, gridDim.x, false};
    const unsigned nb = gridDim.x;
    for (int i = 0; i < iters; ++i) {
        // double-buffered exchange: read what the neighbour wrote LAST round, write this round's value
        float* src = sink + ((size_t)((i + 1) & 1) * nb + (blockIdx.x + 1) % nb) * 256 + threadIdx.x;
        float* dst = sink + ((size_t)(i & 1) * nb + blockIdx.x) * 256 + threadIdx.x;
        if (VAR == 0) {
            if (omx::ld_coh_f32(src) != (float)i) atomicAdd(mismatches, 1u);
            omx::st_coh_f32(dst, (float)(i + 1));
            omx::grid_sync(g);
        } else {
            if (*src != (float)i) atomicAdd(mismatches, 1u);
            *dst = (float)(i + 1);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            __syncthreads();
            if (threadIdx.x == 0) {
                __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                while (__hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < (unsigned)(i + 1) * nb)
                    __builtin_amdgcn_s_sleep(2);
            }
            __syncthreads();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        }
    }
}
// variant 2: XCD-LOCAL groups.  Blocks are dispatched to XCDs round-robin (block b runs on XCD b % 8), so the blocks with
// the same b % 8 share one L2.  They exchange and synchronise through that L2 only: workgroup-scope relaxed atomics lower to
// `global_load/store ... sc0`, which miss the per-CU vector cache but are served by the XCD's L2 -- no write-through to
// memory, no re-validation against the other XCDs.  The question this answers: what does a barrier + a 1 KiB hand-over cost
// when a dependent phase is kept inside one XCD (a tensor-parallel-over-XCDs decode step would need only two device-wide
// exchanges per layer instead of five)?  A wrong placement assumption shows up as stale reads (failed & 2) or a timeout.
// (measured: an sc0 LOAD may still be served by the CU's vector cache -- polls never saw the flag.  What works: poll with a
//  read-modify-write atomic, which always executes in the L2, then drop the vector cache with `buffer_inv sc0` before the
//  plain data loads.)
__device__ __forceinline__ unsigned ld_l2_32(const void* p) {
    // written as asm: the compiler folds an idempotent `fetch_or(p, 0)` back into an (sc0) load
    unsigned r;
    const unsigned zero = 0u;
    asm volatile("global_atomic_or %0, %1, %2, off sc0\n\ts_waitcnt vmcnt(0)" : "=&v"(r) : "v"(p), "v"(zero) : "memory");
    return r;
}
__device__ __forceinline__ void l1_invalidate() { asm volatile("buffer_inv sc0" ::: "memory"); }
__device__ __forceinline__ void st_l2_32(void* p, unsigned v) {
    __hip_atomic_store(reinterpret_cast<unsigned*>(p), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__global__ __launch_bounds__(256) void xcd_barrier_probe_kernel(unsigned* words, unsigned* mismatches, int iters, float* sink) {
    const unsigned nb = gridDim.x, xcd = blockIdx.x % 8, member = blockIdx.x / 8, members = nb / 8;
    unsigned* flags = words + 64 + 16 * nb + 32;           // after the device-wide area and the counters: [8 groups][members] flags, 64 B apart
    unsigned* my_group = flags + (size_t)xcd * members * 16;
    unsigned* release = words + 64 + 16 * xcd;             // one release word per group
    bool dead = false;
    for (int i = 0; i < iters; ++i) {
        const unsigned epoch = (unsigned)i + 1;
        const unsigned peer = xcd + 8 * ((member + 1) % members);   // the next block of the same XCD
        float* src = sink + ((size_t)((i + 1) & 1) * nb + peer) * 256 + threadIdx.x;
        float* dst = sink + ((size_t)(i & 1) * nb + blockIdx.x) * 256 + threadIdx.x;
        l1_invalidate();
        if (*reinterpret_cast<volatile float*>(src) != (float)i) atomicAdd(mismatches, 1u);
        *reinterpret_cast<volatile float*>(dst) = (float)(i + 1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x == 0) st_l2_32(my_group + 16 * member, epoch);
        if (member == 0) {
            for (unsigned b = threadIdx.x; b < members; b += blockDim.x) {
                unsigned it = 0;
                while (!dead && (int)(ld_l2_32(my_group + 16 * b) - epoch) < 0) {
                    __builtin_amdgcn_s_sleep(1);
                    if (++it > (1u << 22)) { dead = true; atomicAdd(mismatches + 1, 1u); }
                }
            }
            __syncthreads();
            if (threadIdx.x == 0) st_l2_32(release, epoch);
        } else if (threadIdx.x == 0) {
            unsigned it = 0;
            while (!dead && (int)(ld_l2_32(release) - epoch) < 0) {
                __builtin_amdgcn_s_sleep(1);
                if (++it > (1u << 22)) { dead = true; atomicAdd(mismatches + 1, 1u); }
            }
        }
        __syncthreads();
    }
}
}  // namespace

// which XCD (XCC_ID hardware register, gfx942+: hwreg 20, bits 3:0) and CU each block of a plain launch runs on
namespace {
__global__ void xcc_id_kernel(unsigned* out) {
    if (threadIdx.x == 0) out[blockIdx.x] = __builtin_amdgcn_s_getreg(20 | (0 << 6) | ((4 - 1) << 11));
}
}  // namespace
extern "C" int omx_bench_xcc_ids(int nblocks, unsigned* host_out) {
    OMX_REQUIRE(nblocks > 0 && host_out, "omx_bench_xcc_ids: bad arguments");
    unsigned* d = nullptr;
    OMX_HIP_CHECK(hipMalloc(&d, (size_t)nblocks * 4));
    xcc_id_kernel<<<nblocks, 256>>>(d);
    OMX_LAUNCH_CHECK();
    OMX_HIP_CHECK(hipMemcpy(host_out, d, (size_t)nblocks * 4, hipMemcpyDeviceToHost));
    (void)hipFree(d);
    return 0;
}

extern "C" int omx_bench_grid_barrier(int nblocks, int iters, int variant, float* us_per_barrier, int* failed) {
    using namespace omx;
    OMX_REQUIRE(nblocks > 0 && iters > 0 && us_per_barrier && failed, "omx_bench_grid_barrier: bad arguments");
    unsigned* words = nullptr;
    float* sink = nullptr;
    OMX_REQUIRE(variant != 2 || (nblocks % 8 == 0 && nblocks <= 512), "omx_bench_grid_barrier: the XCD-local variant needs a multiple of 8 blocks (<= 512)");
    const size_t wbytes = (grid_sync_words(nblocks) + 32 + 16 * (size_t)nblocks + 64) * 4;   // + counter, mismatch count, XCD-group flags
    OMX_HIP_CHECK(hipMalloc(&words, wbytes));
    OMX_HIP_CHECK(hipMalloc(&sink, (size_t)nblocks * 512 * 4));
    OMX_HIP_CHECK(hipMemset(words, 0, wbytes));
    OMX_HIP_CHECK(hipMemset(sink, 0, (size_t)nblocks * 512 * 4));
    unsigned* extra = words + grid_sync_words(nblocks);
    hipEvent_t e0, e1;
    OMX_HIP_CHECK(hipEventCreate(&e0));
    OMX_HIP_CHECK(hipEventCreate(&e1));
    OMX_HIP_CHECK(hipDeviceSynchronize());
    OMX_HIP_CHECK(hipEventRecord(e0, nullptr));
    if (variant == 2) xcd_barrier_probe_kernel<<<nblocks, 256>>>(words, extra + 16, iters, sink);
    else if (variant == 0) grid_barrier_probe_kernel<0><<<nblocks, 256>>>(words, extra, extra + 16, iters, sink);
    else grid_barrier_probe_kernel<1><<<nblocks, 256>>>(words, extra, extra + 16, iters, sink);
    OMX_LAUNCH_CHECK();
    OMX_HIP_CHECK(hipEventRecord(e1, nullptr));
    OMX_HIP_CHECK(hipEventSynchronize(e1));
    float ms = 0.f;
    OMX_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    unsigned abort_word = 0, mism = 0;
    OMX_HIP_CHECK(hipMemcpy(&abort_word, words + 16, 4, hipMemcpyDeviceToHost));
    OMX_HIP_CHECK(hipMemcpy(&mism, extra + 16, 4, hipMemcpyDeviceToHost));
    *us_per_barrier = ms * 1000.f / iters;
    unsigned timeouts = 0;
    OMX_HIP_CHECK(hipMemcpy(&timeouts, extra + 17, 4, hipMemcpyDeviceToHost));
    *failed = ((abort_word || timeouts) ? 1 : 0) | (mism ? 2 : 0);   // 1: a waiter timed out; 2: an exchange read a stale value
    (void)hipFree(words); (void)hipFree(sink);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return 0;
}

// ---- packed-weight GEMV (quant.hip): one shape, weights rotated over n_copies buffers, HIP events ----
#include "quant.hpp"
extern "C" int omx_bench_qgemv(int N, int K, int bits, int pro, int epi, int n_copies, int iters, float* avg_ms) {
    using namespace omx;
    OMX_REQUIRE(avg_ms && n_copies > 0 && iters > 0, "omx_bench_qgemv: bad arguments");
    const int mats = (epi == EPI_SWIGLU) ? 2 : 1;
    const size_t wwords = (size_t)N * K * bits / 32, ngroups = (size_t)N * K / 64;
    std::vector<uint32_t*> w(n_copies * mats, nullptr);
    std::vector<bf16_t*> sc(n_copies * mats, nullptr), bi(n_copies * mats, nullptr);
    for (size_t i = 0; i < w.size(); ++i) {
        OMX_HIP_CHECK(hipMalloc((void**)&w[i], wwords * 4));
        OMX_HIP_CHECK(hipMalloc((void**)&sc[i], ngroups * 2));
        OMX_HIP_CHECK(hipMalloc((void**)&bi[i], ngroups * 2));
        if (omx_fill_uniform(w[i], wwords * 2, 70u + (uint32_t)i, 1.0f, 0.f, OMX_BFLOAT16, nullptr)) return 1;   // arbitrary nibbles
        if (omx_fill_uniform(sc[i], ngroups, 90u + (uint32_t)i, 0.002f, 0.004f, OMX_BFLOAT16, nullptr)) return 1;
        if (omx_fill_uniform(bi[i], ngroups, 110u + (uint32_t)i, 0.03f, 0.f, OMX_BFLOAT16, nullptr)) return 1;
    }
    void *x = nullptr, *nw = nullptr, *out = nullptr, *resid = nullptr, *slot = nullptr;
    OMX_HIP_CHECK(hipMalloc(&x, (size_t)K * 2));
    OMX_HIP_CHECK(hipMalloc(&nw, (size_t)K * 2));
    OMX_HIP_CHECK(hipMalloc(&out, (size_t)N * 4));
    OMX_HIP_CHECK(hipMalloc(&resid, (size_t)N * 2));
    OMX_HIP_CHECK(hipMalloc(&slot, 8 * 65536));
    omx_fill_uniform(x, K, 3, 1.0f, 0.f, OMX_BFLOAT16, nullptr);
    omx_fill_uniform(nw, K, 4, 0.1f, 1.f, OMX_BFLOAT16, nullptr);
    omx_fill_uniform(resid, N, 5, 1.0f, 0.f, OMX_BFLOAT16, nullptr);
    hipStream_t s;
    OMX_HIP_CHECK(hipStreamCreate(&s));
    hipEvent_t e0, e1;
    OMX_HIP_CHECK(hipEventCreate(&e0));
    OMX_HIP_CHECK(hipEventCreate(&e1));
    std::vector<uint32_t*> tiles(w.size(), nullptr);       // the matrix-core kernel's form of the same matrices (qgemv_mfma.hip)
    const char* mfma_env = getenv("OMX_QGEMV_MFMA");
    if (qgemv4m_shape_ok(K, 64, bits) && !(mfma_env && mfma_env[0] == '0'))
        for (size_t i = 0; i < w.size(); ++i) {
            OMX_HIP_CHECK(hipMalloc((void**)&tiles[i], qgemv4m_tile_words(N, K) * 4));
            if (launch_qgemv4m_repack(tiles[i], w[i], sc[i], bi[i], N, K, nullptr)) return 1;
        }
    auto run = [&](int i) {
        QGemvArgs a = {};
        const int c = (i % n_copies) * mats;
        a.m[0] = QMat{w[c], sc[c], bi[c], N};
        a.m[0].tiles = tiles[c];
        if (mats == 2) { a.m[1] = QMat{w[c + 1], sc[c + 1], bi[c + 1], N}; a.m[1].tiles = tiles[c + 1]; }
        a.N = N; a.K = K; a.group = 64;
        a.x = (const bf16_t*)x; a.norm_w = (const bf16_t*)nw; a.eps = 1e-6f; a.resid = (const bf16_t*)resid;
        a.out = (bf16_t*)out; a.argmax_slot = (unsigned long long*)slot;
        return launch_qgemv(a, bits, pro, epi, s);
    };
    OMX_HIP_CHECK(hipDeviceSynchronize());
    for (int i = 0; i < n_copies + 2; ++i)
        if (run(i)) return 1;
    OMX_HIP_CHECK(hipStreamSynchronize(s));
    OMX_HIP_CHECK(hipEventRecord(e0, s));
    for (int i = 0; i < iters; ++i)
        if (run(i)) return 1;
    OMX_HIP_CHECK(hipEventRecord(e1, s));
    OMX_HIP_CHECK(hipEventSynchronize(e1));
    float ms = 0.f;
    OMX_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    *avg_ms = ms / iters;
    for (size_t i = 0; i < w.size(); ++i) { (void)hipFree(w[i]); (void)hipFree(sc[i]); (void)hipFree(bi[i]); if (tiles[i]) (void)hipFree(tiles[i]); }
    (void)hipFree(x); (void)hipFree(nw); (void)hipFree(out); (void)hipFree(resid); (void)hipFree(slot);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipStreamDestroy(s);
    return 0;
}

/* test hook (tests/test_gpu_quant.py): ONE fused packed-GEMV launch of the decode step on caller-owned device tensors -- the
 * prologue / epilogue forms the engine uses (pro: 0 none, 1 RMSNorm; epi: gemv.hpp EPI_*), which the raw omx_quantized_matmul never
 * reaches.  w1 / s1 / b1: the up matrix of a SwiGLU pair, or null; n0: rows of the first member when w1 stacks below it (q | k). */
extern "C" int omx_debug_qgemv(void* out, float* out_f32, unsigned long long* argmax_slot, const void* x, const void* norm_w, const void* resid,
                               const void* w0, const void* s0, const void* b0, const void* w1, const void* s1, const void* b1, int n0,
                               int N, int K, int group, int bits, int pro, int epi, float eps, int single_round, void* stream) {
    using namespace omx;
    QGemvArgs a = {};
    if (epi == EPI_SWIGLU) {
        a.m[0] = QMat{(const uint32_t*)w0, (const bf16_t*)s0, (const bf16_t*)b0, N};
        a.m[1] = QMat{(const uint32_t*)w1, (const bf16_t*)s1, (const bf16_t*)b1, N};
    } else {
        a.m[0] = QMat{(const uint32_t*)w0, (const bf16_t*)s0, (const bf16_t*)b0, w1 ? n0 : N};
        if (w1) a.m[1] = QMat{(const uint32_t*)w1, (const bf16_t*)s1, (const bf16_t*)b1, N - n0};
    }
    a.N = N; a.K = K; a.group = group;
    a.x = (const bf16_t*)x; a.norm_w = (const bf16_t*)norm_w; a.eps = eps; a.resid = (const bf16_t*)resid;
    a.out = (bf16_t*)out; a.out_f32 = out_f32; a.argmax_slot = argmax_slot; a.swiglu_single_round = single_round;
    uint32_t* tiles[2] = {nullptr, nullptr};
    if (qgemv4m_shape_ok(K, group, bits))
        for (int i = 0; i < 2; ++i)
            if (a.m[i].w) {
                OMX_HIP_CHECK(hipMalloc((void**)&tiles[i], qgemv4m_tile_words(a.m[i].n, K) * 4));
                if (launch_qgemv4m_repack(tiles[i], a.m[i].w, a.m[i].scales, a.m[i].biases, a.m[i].n, K, (hipStream_t)stream)) return 1;
                a.m[i].tiles = tiles[i];
            }
    const int rc = launch_qgemv(a, bits, pro, epi, (hipStream_t)stream);
    OMX_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    for (int i = 0; i < 2; ++i)
        if (tiles[i]) (void)hipFree(tiles[i]);
    return rc;
}
extern "C" int omx_debug_qgemv_grid(int N) { return omx::qgemv_grid(N); }

/* test hook (tests/test_gpu_mixed_quant.py): a row-stacked packed GEMV whose members carry their OWN formats -- up to three members
 * (w, scales, biases, n, bits, group; bf16 triplets), EPI_STORE, pro 0 none / 1 RMSNorm: the one launch of qgemv_stack_kernel.  The
 * interleaved scale | bias words are built for K % 2048 == 0, as the engine builds them.  Synchronises the stream. */
extern "C" int omx_debug_qgemv_mixed(void* out, const void* x, const void* norm_w, const void* const* w, const void* const* scales, const void* const* biases,
                                     const int* n, const int* bits, const int* group, int n_members, int K, int pro, float eps, void* stream) {
    using namespace omx;
    OMX_REQUIRE(out && x && w && scales && biases && n && bits && group && n_members >= 1 && n_members <= 3, "omx_debug_qgemv_mixed: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    QGemvArgs a = {};
    std::vector<void*> owned;
    int rc = 0;
    for (int i = 0; i < n_members && !rc; ++i) {
        OMX_REQUIRE(w[i] && scales[i] && n[i] > 0, "omx_debug_qgemv_mixed: member %d is empty", i);
        a.m[i] = QMat{(const uint32_t*)w[i], (const bf16_t*)scales[i], (const bf16_t*)biases[i], n[i]};
        a.m[i].bits = bits[i]; a.m[i].group = group[i];
        a.N += n[i];
        if (group[i] > 0 && K % 2048 == 0 && K % group[i] == 0) {
            uint32_t* sb = nullptr;
            const size_t ng = (size_t)n[i] * (K / group[i]);
            if (hipMalloc((void**)&sb, ng * 4) != hipSuccess) { rc = set_error("omx_debug_qgemv_mixed: out of memory"); break; }
            owned.push_back(sb);
            rc = launch_quant_interleave(sb, a.m[i].scales, a.m[i].biases, ng, s);
            a.m[i].sb = sb;
        }
    }
    a.K = K; a.group = group[0];
    a.x = (const bf16_t*)x; a.norm_w = (const bf16_t*)norm_w; a.eps = eps; a.out = (bf16_t*)out;
    if (!rc) rc = launch_qgemv(a, bits[0], pro, EPI_STORE, s);
    (void)hipStreamSynchronize(s);
    for (void* p : owned) (void)hipFree(p);
    return rc;
}

/* test hook of the dense decode GEMV (gemv.hip): one launch_gemv of the given prologue / epilogue, bf16 (f16 = 0) or float16 (f16 = 1).
 * w0 [n0, K] | w1 | w2 row-stacked (q | k | v; N = n0 + n1 + rest), or gate (w0) / up (w1) [N, K] for EPI_SWIGLU.  EPI_ARGMAX writes
 * omx_debug_gemv_grid(N, K) partial keys to argmax_slot.  Synchronises the stream. */
extern "C" int omx_debug_gemv(void* out, unsigned long long* argmax_slot, const void* x, const void* norm_w, const void* resid, const void* bias,
                              const void* w0, const void* w1, const void* w2, int n0, int n1, int N, int K, int pro, int epi, int f16, float eps,
                              int single_round, void* stream) {
    using namespace omx;
    OMX_REQUIRE(out && x && w0 && N > 0, "omx_debug_gemv: bad arguments");
    GemvArgs a = {};
    a.w0 = (const bf16_t*)w0; a.w1 = (const bf16_t*)w1; a.w2 = (const bf16_t*)w2;
    if (epi == EPI_SWIGLU || !w1) {
        a.n0 = N;
    } else {
        a.n0 = n0; a.n1 = w2 ? n1 : N - n0; a.n2 = w2 ? N - n0 - n1 : 0;
    }
    a.N = N; a.K = K;
    a.x = (const bf16_t*)x; a.norm_w = (const bf16_t*)norm_w; a.eps = eps; a.resid = (const bf16_t*)resid;
    a.out = out; a.out_bias = (const bf16_t*)bias; a.argmax_slot = argmax_slot; a.swiglu_single_round = single_round;
    a.f16 = f16;
    const int rc = launch_gemv(a, pro, epi, (hipStream_t)stream);
    OMX_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    return rc;
}
extern "C" int omx_debug_gemv_grid(int N, int K) { return omx::gemv_grid(N, K, omx::EPI_ARGMAX, 0); }

extern "C" int omx_debug_gemv_ex(omx_gemv_ex* d, void* stream) {
    using namespace omx;
    OMX_REQUIRE(d && d->N > 0 && d->K > 0, "omx_debug_gemv_ex: bad arguments");
    OMX_REQUIRE(d->pro == PRO_NONE || d->pro == PRO_RMSNORM, "omx_debug_gemv_ex: prologue %d (PRO_ROUTE is not taken here)", d->pro);
    GemvArgs a = {};
    a.w0 = (const bf16_t*)d->w0; a.w1 = (const bf16_t*)d->w1; a.w2 = (const bf16_t*)d->w2;
    if (d->epi == EPI_SWIGLU || !d->w1) {
        a.n0 = d->N;
    } else {
        a.n0 = d->n0; a.n1 = d->w2 ? d->n1 : d->N - d->n0; a.n2 = d->w2 ? d->N - d->n0 - d->n1 : 0;
    }
    a.N = d->N; a.K = d->K;
    a.x = (const bf16_t*)d->x; a.norm_w = (const bf16_t*)d->norm_w; a.eps = d->eps; a.resid = (const bf16_t*)d->resid;
    a.out = d->out; a.out_bias = (const bf16_t*)d->bias; a.argmax_slot = d->argmax_slot; a.swiglu_single_round = d->single_round;
    a.f16 = d->f16;
    a.rows_per_wave = d->rows_per_wave; a.row_offset = d->row_offset;
    a.x_partial = d->x_partial; a.x_partial_n = d->x_partial_n; a.x_out = (bf16_t*)d->x_out; a.out_scale = (const bf16_t*)d->out_scale;
    a.n_batch = d->n_batch; a.x_div = d->x_div; a.x_bstride = (size_t)d->x_bstride; a.out_bstride_bytes = (size_t)d->out_bstride_bytes;
    a.w_sel = d->w_sel; a.w_estride = (size_t)d->w_estride; a.w_sel_lo = d->w_sel_lo; a.w_sel_n = d->w_sel_n;
    const GemvRoute r = gemv_route(a, d->pro, d->epi);
    d->route_nv = r.nv; d->route_ksplit = r.ksplit; d->route_tail = r.tail; d->route_rows_per_wave = r.rows_per_wave; d->route_blocks = r.blocks;
    if (d->dry_run) return 0;
    OMX_REQUIRE(d->out && d->x && d->w0, "omx_debug_gemv_ex: out, x and w0 are required");
    OMX_REQUIRE(d->epi != EPI_ARGMAX || (d->argmax_slot && r.blocks <= d->argmax_slot_n),
                "omx_debug_gemv_ex: the launch writes %d argmax partials, the slot holds %d", r.blocks, d->argmax_slot_n);
    OMX_REQUIRE(!(d->n_batch > 1 || d->w_sel) || (d->x_div >= 1 && d->out_bstride_bytes > 0), "omx_debug_gemv_ex: batched launch needs x_div and out_bstride_bytes");
    OMX_REQUIRE(!d->x_partial || d->x_partial_n >= 1, "omx_debug_gemv_ex: x_partial needs x_partial_n >= 1");
    const int rc = launch_gemv(a, d->pro, d->epi, (hipStream_t)stream);
    OMX_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    return rc;
}

extern "C" int omx_debug_attn_step(omx_attn_step_dbg* d, void* stream) {
    using namespace omx;
    OMX_REQUIRE(d && d->qkv && d->k && d->v && d->rope_cur && d->granules && d->out, "omx_debug_attn_step: missing buffer");
    OMX_REQUIRE(d->H > 0 && d->Hkv > 0 && d->H % d->Hkv == 0 && (d->D == 64 || d->D == 128) && d->cap > 0,
                "omx_debug_attn_step: bad geometry (H %d, Hkv %d, D %d, cap %d)", d->H, d->Hkv, d->D, d->cap);
    OMX_REQUIRE(d->pos >= 0 && d->pos < d->cap, "omx_debug_attn_step: position %d outside the cache of %d rows", d->pos, d->cap);
    OMX_REQUIRE(!d->q_norm_w == !d->k_norm_w, "omx_debug_attn_step: q and k norm weights go together");
    const int G = d->H / d->Hkv;
    if (d->chunk <= 0 || d->nsplit <= 0) {
        OMX_REQUIRE(d->tk_max > 0, "omx_debug_attn_step: give chunk and nsplit, or tk_max");
        attn_step_plan(d->tk_max, d->Hkv, G, d->D, &d->chunk, &d->nsplit);
    }
    OMX_REQUIRE((long long)d->chunk * d->nsplit >= (long long)d->pos + 1,
                "omx_debug_attn_step: plan (chunk %d, %d splits) does not cover position %d", d->chunk, d->nsplit, d->pos);
    OMX_REQUIRE((long long)d->H * d->nsplit * (d->D + 2) <= d->granules_n, "omx_debug_attn_step: %lld granules, the plan needs %lld",
                d->granules_n, (long long)d->H * d->nsplit * (d->D + 2));
    hipStream_t s = (hipStream_t)stream;
    unsigned* st = nullptr;   // pos | seq | abort flag
    OMX_HIP_CHECK(hipMalloc((void**)&st, 3 * sizeof(unsigned)));
    const unsigned host[3] = {(unsigned)d->pos, d->seq, 0u};
    OMX_HIP_CHECK(hipMemcpyAsync(st, host, sizeof(host), hipMemcpyHostToDevice, s));
    AttnStepArgs a = {};
    a.qkv = (const bf16_t*)d->qkv; a.k = (bf16_t*)d->k; a.v = (bf16_t*)d->v; a.kv_head_stride = (int64_t)d->cap * d->D;
    a.H = d->H; a.Hkv = d->Hkv; a.cap = d->cap; a.scale = d->scale; a.eps = d->eps;
    a.q_norm_w = (const bf16_t*)d->q_norm_w; a.k_norm_w = (const bf16_t*)d->k_norm_w; a.rope_cur = d->rope_cur;
    a.pos_ptr = (const int*)st; a.seq_ptr = st + 1; a.tag_mul = d->tag_mul; a.tag_add = d->tag_add;
    a.chunk = d->chunk; a.nsplit = d->nsplit; a.ws = (uint64_t*)d->granules; a.out = (bf16_t*)d->out; a.abort_flag = st + 2;
    a.f16 = d->f16;
    int rc = launch_attn_step(a, d->D, s);
    unsigned back[3] = {0u, 0u, 0u};
    if (rc == 0) {
        OMX_HIP_CHECK(hipMemcpyAsync(back, st, sizeof(back), hipMemcpyDeviceToHost, s));
        OMX_HIP_CHECK(hipStreamSynchronize(s));
    }
    d->abort_flag = back[2];
    OMX_HIP_CHECK(hipFree(st));
    return rc;
}

extern "C" int omx_debug_gemv_rows(omx_gemv_rows_dbg* d, void* stream) {
    using namespace omx;
    OMX_REQUIRE(d && d->x, "omx_debug_gemv_rows: x is required");
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if (!d->segmented) {
        OMX_REQUIRE(d->w && d->out, "omx_debug_gemv_rows: w and out are required");
        OMX_REQUIRE(!d->gate || d->resid, "omx_debug_gemv_rows: the gated epilogue reads resid");
        d->route_rpw = gemv_rows_rpw(d->N, 0);
        rc = launch_gemv_rows((bf16_t*)d->out, (const bf16_t*)d->x, (const bf16_t*)d->w, (const bf16_t*)d->bias, (const bf16_t*)d->resid,
                              (const bf16_t*)d->gate, d->M, d->N, d->K, d->relu, s);
    } else {
        OMX_REQUIRE(d->n_plain >= 0 && d->n_plain <= 3, "omx_debug_gemv_rows: %d plain segments (0..3)", d->n_plain);
        GemmSegs g = {};
        int rows = 0;
        for (int i = 0; i < d->n_plain; ++i) {
            const omx_gemv_rows_seg& p = d->seg[i];
            OMX_REQUIRE(p.ld >= p.cols, "omx_debug_gemv_rows: segment %d has row stride %d < %d columns", i, p.ld, p.cols);
            g.plain[i] = GemmSeg{(const bf16_t*)p.w, (const bf16_t*)p.bias, (bf16_t*)p.out, p.cols, p.ld, 0};
            rows += p.cols;
        }
        g.n_plain = d->n_plain;
        OMX_REQUIRE(d->half <= 0 || d->ld_act >= d->half, "omx_debug_gemv_rows: activation row stride %d < %d columns", d->ld_act, d->half);
        g.w_gate = (const bf16_t*)d->w_gate; g.w_up = (const bf16_t*)d->w_up; g.out_act = (bf16_t*)d->out_act;
        g.half = d->half; g.ld_act = d->ld_act; g.act_mode = d->act_mode;
        g.pre_norm_w = (const bf16_t*)d->pre_norm_w; g.pre_norm_eps = d->pre_norm_eps;
        d->route_rpw = gemv_rows_rpw(rows + 2 * d->half, d->half);
        rc = launch_gemv_rows_segmented((const bf16_t*)d->x, d->M, d->K, g, s);
    }
    if (rc) return rc;
    OMX_HIP_CHECK(hipStreamSynchronize(s));
    return 0;
}

namespace omx { extern int g_qgemv_mfma_mode; }   // qgemv_mfma.hip

/* test hook of the packed decode GEMV: ONE launch_qgemv with every field of the launch, as the engines fill them in (include/omx.h
 * lists the fields), and the route the launchers report.  The route is taken first, on the host; what the launch needs (argmax slots)
 * is checked against it before anything runs.  Synchronises the stream. */
extern "C" int omx_debug_qgemv_ex(omx_qgemv_ex* d, void* stream) {
    using namespace omx;
    OMX_REQUIRE(d && d->N > 0 && d->K > 0, "omx_debug_qgemv_ex: bad arguments");
    OMX_REQUIRE(d->pro == PRO_NONE || d->pro == PRO_RMSNORM, "omx_debug_qgemv_ex: prologue %d", d->pro);
    hipStream_t s = (hipStream_t)stream;
    const uint32_t* const kDummy = reinterpret_cast<const uint32_t*>(uintptr_t(64));   // "present" in a launch that never runs
    const int n_experts = d->n_experts > 1 ? d->n_experts : 1;
    QGemvArgs a = {};
    int rows = 0, n_members = 0;
    for (int i = 0; i < 3; ++i) {
        const omx_qgemv_member& m = d->m[i];
        if (m.n <= 0) break;
        OMX_REQUIRE(d->dry_run || (m.w && m.scales), "omx_debug_qgemv_ex: member %d has no weights / scales", i);
        a.m[i] = QMat{d->dry_run ? kDummy : (const uint32_t*)m.w, (const bf16_t*)m.scales, (const bf16_t*)m.biases, m.n};
        a.m[i].bits = m.bits; a.m[i].group = m.group;
        rows += m.n; n_members = i + 1;
    }
    OMX_REQUIRE(n_members >= 1, "omx_debug_qgemv_ex: no member");
    if (d->epi == EPI_SWIGLU) OMX_REQUIRE(n_members == 2 && d->m[0].n == d->N && d->m[1].n == d->N, "omx_debug_qgemv_ex: SwiGLU takes gate and up of N rows each");
    else OMX_REQUIRE(rows == d->N, "omx_debug_qgemv_ex: the members hold %d rows, N = %d", rows, d->N);
    a.N = d->N; a.K = d->K; a.group = d->group;
    a.x = (const bf16_t*)d->x; a.norm_w = (const bf16_t*)d->norm_w; a.eps = d->eps; a.resid = (const bf16_t*)d->resid;
    a.out = (bf16_t*)d->out; a.out_f32 = d->out_f32; a.argmax_slot = d->argmax_slot; a.swiglu_single_round = d->single_round;
    a.scales_f16 = d->scales_f16; a.row_offset = d->row_offset; a.rolled_stage = d->rolled_stage;
    a.n_batch = d->n_batch; a.x_div = d->x_div; a.w_sel = d->w_sel; a.w_estride = (size_t)d->w_estride; a.s_estride = (size_t)d->s_estride;
    a.w_sel_lo = d->w_sel_lo; a.w_sel_n = d->w_sel_n;
    // the route first, with placeholders where the repacks will be
    bool tiles_ok[3] = {false, false, false};
    for (int i = 0; i < n_members; ++i) {
        const int b = qmat_bits(a.m[i], d->bits), g = qmat_group(a.m[i], d->group);
        OMX_REQUIRE(g > 0 && d->K % g == 0, "omx_debug_qgemv_ex: the row width (%d) must be divisible by the group size (%d)", d->K, g);
        if (d->use_sb) a.m[i].sb = kDummy;
        tiles_ok[i] = d->use_tiles && n_experts == 1 && qgemv4m_shape_ok(d->K, g, b);
        if (tiles_ok[i]) a.m[i].tiles = kDummy;
    }
    QGemvRoute r = {};
    r.dry_run = 1;
    const int saved_mode = g_qgemv_mfma_mode;
    g_qgemv_mfma_mode = d->mfma;
    int rc = launch_qgemv(a, d->bits, d->pro, d->epi, s, &r);
    g_qgemv_mfma_mode = saved_mode;
    if (rc) return rc;
    OMX_REQUIRE(r.kernel != 0, "omx_debug_qgemv_ex: the launchers reported no route");
    d->route_kernel = r.kernel; d->route_bits = r.bits; d->route_w = r.W; d->route_rb = r.RB; d->route_rows_per_wave = r.rows_per_wave;
    d->route_sb = r.SB; d->route_f16s = r.F16S; d->route_blocks = r.blocks; d->route_lds_bytes = r.lds_bytes;
    d->route_ks = r.KS; d->route_nu = r.NU; d->route_nbuf = r.NBUF;
    if (d->dry_run) return 0;
    OMX_REQUIRE(d->x && (d->epi == EPI_F32 ? (void*)d->out_f32 : d->out), "omx_debug_qgemv_ex: x and the output are required");
    OMX_REQUIRE(d->pro != PRO_RMSNORM || d->norm_w, "omx_debug_qgemv_ex: the RMSNorm prologue reads norm_w");
    OMX_REQUIRE(d->epi != EPI_RESIDUAL || d->resid, "omx_debug_qgemv_ex: the residual epilogue reads resid");
    if (d->epi == EPI_ARGMAX) {
        // the matrix-core kernel also clears the slots up to qgemv_grid(N), which the engines reduce
        const int need = r.kernel == 3 ? std::max(r.blocks, qgemv_grid(d->N)) : r.blocks;
        OMX_REQUIRE(d->argmax_slot && need <= d->argmax_slot_n, "omx_debug_qgemv_ex: the launch writes %d argmax partials, the slot holds %d",
                    need, d->argmax_slot_n);
    }
    OMX_REQUIRE(!d->w_sel || (d->n_batch >= 1 && d->x_div >= 1), "omx_debug_qgemv_ex: an expert-selected launch needs n_batch and x_div");
    std::vector<void*> owned;
    for (int i = 0; i < n_members && !rc; ++i) {
        const int g = qmat_group(a.m[i], d->group);
        a.m[i].sb = nullptr; a.m[i].tiles = nullptr;
        if (d->use_sb) {
            const size_t per = (size_t)a.m[i].n * (d->K / g), ng = n_experts > 1 ? (size_t)(n_experts - 1) * a.s_estride + per : per;
            uint32_t* sb = nullptr;
            if (hipMalloc((void**)&sb, ng * 4) != hipSuccess) { rc = set_error("omx_debug_qgemv_ex: out of memory"); break; }
            owned.push_back(sb);
            rc = launch_quant_interleave(sb, a.m[i].scales, a.m[i].biases, ng, s);
            a.m[i].sb = sb;
        }
        if (tiles_ok[i] && !rc) {
            uint32_t* t = nullptr;
            if (hipMalloc((void**)&t, qgemv4m_tile_words(a.m[i].n, d->K) * 4) != hipSuccess) { rc = set_error("omx_debug_qgemv_ex: out of memory"); break; }
            owned.push_back(t);
            rc = launch_qgemv4m_repack(t, a.m[i].w, a.m[i].scales, a.m[i].biases, a.m[i].n, d->K, s);
            a.m[i].tiles = t;
        }
    }
    if (!rc) {
        QGemvRoute r2 = {};
        g_qgemv_mfma_mode = d->mfma;
        rc = launch_qgemv(a, d->bits, d->pro, d->epi, s, &r2);
        g_qgemv_mfma_mode = saved_mode;
        if (!rc && (r2.kernel != r.kernel || r2.blocks != r.blocks || r2.lds_bytes != r.lds_bytes))
            rc = set_error("omx_debug_qgemv_ex: the launch took kernel %d with %d blocks, the dry pass reported kernel %d with %d", r2.kernel, r2.blocks, r.kernel, r.blocks);
    }
    (void)hipStreamSynchronize(s);
    for (void* p : owned) (void)hipFree(p);
    return rc;
}

/* test hook of qgemv_rows.hip: M activation rows x [M, K] against n_members packed matrices (w / sc / bi / n: arrays of n_members; a
 * q | k | v stack, or gate and up for EPI_SWIGLU), out [M, N] (resid [M, N]).  use_sb: build the interleaved scale | bias words first.
 * reference != 0 runs what the rows kernel must reproduce bit for bit instead: launch_qgemv's VALU kernel (no matrix-core tiles) with
 * n_batch = M -- one launch per row for EPI_RESIDUAL, whose batched form shares one residual row. */
extern "C" int omx_debug_qgemv_rows(void* out, const void* x, const void* norm_w, const void* resid, const void* const* w, const void* const* sc,
                                    const void* const* bi, const int* n, int n_members, int M, int N, int K, int group, int bits, int pro, int epi,
                                    float eps, int single_round, int use_sb, int reference, void* stream) {
    using namespace omx;
    OMX_REQUIRE(out && x && w && sc && n && n_members >= 1 && n_members <= 3 && M >= 1, "omx_debug_qgemv_rows: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    QRowsArgs ra = {};
    QGemvArgs& a = ra.g;
    uint32_t* sb[3] = {nullptr, nullptr, nullptr};
    for (int i = 0; i < n_members; ++i) {
        a.m[i] = QMat{(const uint32_t*)w[i], (const bf16_t*)sc[i], bi ? (const bf16_t*)bi[i] : nullptr, n[i]};
        if (use_sb) {
            const size_t ng = (size_t)n[i] * (K / group);
            OMX_HIP_CHECK(hipMalloc((void**)&sb[i], ng * 4));
            if (launch_quant_interleave(sb[i], a.m[i].scales, a.m[i].biases, ng, s)) return 1;
            a.m[i].sb = sb[i];
        }
    }
    a.N = N; a.K = K; a.group = group;
    a.x = (const bf16_t*)x; a.norm_w = (const bf16_t*)norm_w; a.eps = eps; a.resid = (const bf16_t*)resid;
    a.out = (bf16_t*)out; a.swiglu_single_round = single_round;
    int rc = 0;
    if (!reference) {
        ra.M = M;
        rc = launch_qgemv_rows(ra, bits, pro, epi, s);
    } else if (epi == EPI_RESIDUAL) {
        for (int t = 0; t < M && rc == 0; ++t) {
            QGemvArgs r = a;
            r.x = a.x + (size_t)t * K; r.resid = a.resid + (size_t)t * N; r.out = a.out + (size_t)t * N;
            rc = launch_qgemv(r, bits, pro, epi, s);
        }
    } else {
        a.n_batch = M; a.x_div = 1;
        rc = launch_qgemv(a, bits, pro, epi, s);
    }
    OMX_HIP_CHECK(hipStreamSynchronize(s));
    for (int i = 0; i < 3; ++i)
        if (sb[i]) (void)hipFree(sb[i]);
    return rc;
}

// ---- what does a COLD weight matrix cost a streaming GEMV at its start?  (tools/tlb_probe.py)
//      mode 0: rotate through n_copies matrices (cold, as in a decode step)
//      mode 1: before each GEMV, a tiny kernel reads ONE line every `stride` bytes of that matrix from every XCD
//              (address translations warm, data cold)
//      mode 2: before each GEMV, a kernel streams the whole matrix (translations and Infinity Cache warm)
//      Per-kernel times come from rocprofv3 --kernel-trace --stats (different kernel names).
namespace {
__global__ void page_touch_kernel(const unsigned char* base, size_t bytes, size_t stride, unsigned* sink) {
    // blockIdx % 8 is the XCD (round-robin dispatch): every XCD sweeps ALL pages, 1/(blocks per XCD) each
    const size_t per_xcd = gridDim.x / 8, j = blockIdx.x / 8;
    unsigned acc = 0;
    for (size_t off = (j * blockDim.x + threadIdx.x) * stride; off < bytes; off += per_xcd * blockDim.x * stride)
        acc += *reinterpret_cast<const volatile unsigned*>(base + off);
    if (acc == 0x12345678u) *sink = acc;
}
__global__ void stream_read_kernel(const uint4* base, size_t n16, unsigned* sink) {
    unsigned acc = 0;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x) {
        const uint4 v = base[i];
        acc += v.x ^ v.y ^ v.z ^ v.w;
    }
    if (acc == 0x12345678u) *sink = acc;
}
}  // namespace

extern "C" int omx_bench_gemv_warm(int N, int K, int pro, int epi, int n_copies, int iters, int mode, long stride,
                                   int one_allocation, float* avg_ms) {
    using namespace omx;
    OMX_REQUIRE(avg_ms && n_copies > 0 && iters > 0, "omx_bench_gemv_warm: bad arguments");
    const int mats = (epi == EPI_SWIGLU) ? 2 : 1;
    const size_t wbytes = (((size_t)N * K * 2 * mats) + (2u << 20) - 1) & ~(size_t)((2u << 20) - 1);
    std::vector<void*> w(n_copies, nullptr);
    void* big = nullptr;
    if (one_allocation) {
        OMX_HIP_CHECK(hipMalloc(&big, wbytes * n_copies));
        for (int i = 0; i < n_copies; ++i) w[i] = (char*)big + wbytes * i;
    } else {
        for (auto& p : w) OMX_HIP_CHECK(hipMalloc(&p, wbytes));
    }
    for (int i = 0; i < n_copies; ++i)
        if (omx_fill_uniform(w[i], (size_t)N * K * mats, 17u + i, 0.03f, 0.f, OMX_BFLOAT16, nullptr)) return 1;
    void *x = nullptr, *nw = nullptr, *out = nullptr, *resid = nullptr, *slot = nullptr;
    OMX_HIP_CHECK(hipMalloc(&x, (size_t)K * 2));
    OMX_HIP_CHECK(hipMalloc(&nw, (size_t)K * 2));
    OMX_HIP_CHECK(hipMalloc(&out, (size_t)N * 4));
    OMX_HIP_CHECK(hipMalloc(&resid, (size_t)N * 2));
    OMX_HIP_CHECK(hipMalloc(&slot, 8 * 65536));
    omx_fill_uniform(x, K, 3, 1.0f, 0.f, OMX_BFLOAT16, nullptr);
    omx_fill_uniform(nw, K, 4, 0.1f, 1.f, OMX_BFLOAT16, nullptr);
    omx_fill_uniform(resid, N, 5, 1.0f, 0.f, OMX_BFLOAT16, nullptr);
    OMX_HIP_CHECK(hipMemset(slot, 0, 8 * 65536));
    hipStream_t s;
    OMX_HIP_CHECK(hipStreamCreate(&s));
    hipEvent_t e0, e1;
    OMX_HIP_CHECK(hipEventCreate(&e0));
    OMX_HIP_CHECK(hipEventCreate(&e1));
    auto run = [&](int i) {
        const bf16_t* base = (const bf16_t*)w[i % n_copies];
        if (mode == 1) page_touch_kernel<<<64, 256, 0, s>>>((const unsigned char*)base, (size_t)N * K * 2 * mats, (size_t)stride, (unsigned*)slot);
        if (mode == 2) stream_read_kernel<<<2048, 256, 0, s>>>((const uint4*)base, (size_t)N * K * 2 * mats / 16, (unsigned*)slot);
        GemvArgs a = {};
        a.w0 = base;
        a.w1 = base + (size_t)N * K;
        a.n0 = N; a.N = N; a.K = K;
        a.x = (const bf16_t*)x;
        a.norm_w = (const bf16_t*)nw;
        a.eps = 1e-6f;
        a.resid = (const bf16_t*)resid;
        a.out = out;
        a.argmax_slot = (unsigned long long*)slot;
        return launch_gemv(a, pro, epi, s);
    };
    for (int i = 0; i < n_copies + 2; ++i)
        if (run(i)) return 1;
    OMX_HIP_CHECK(hipStreamSynchronize(s));
    OMX_HIP_CHECK(hipEventRecord(e0, s));
    for (int i = 0; i < iters; ++i)
        if (run(i)) return 1;
    OMX_HIP_CHECK(hipEventRecord(e1, s));
    OMX_HIP_CHECK(hipEventSynchronize(e1));
    float ms = 0.f;
    OMX_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    *avg_ms = ms / iters;
    if (big) (void)hipFree(big);
    else for (auto p : w) (void)hipFree(p);
    (void)hipFree(x); (void)hipFree(nw); (void)hipFree(out); (void)hipFree(resid); (void)hipFree(slot);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipStreamDestroy(s);
    return 0;
}

// ---- test hooks of the decode step's forms (tests/test_gpu_down_qkv_chain.py) ----
#include "engine_model.hpp"

/* which in-launch folds the NEXT step of this engine would take, as the step itself decides (environment switches read now):
 * forms[0] = down + the next layer's q/k/v in one launch, forms[1] = the O projection inside the attention launch, forms[2] = the
 * persistent-step mode; forms[3] = 1 once a give-up switched the first fold off for this engine; forms[4] = gate/up + SwiGLU inside the
 * attention launch (of any layer), forms[5] = 1 once a give-up switched THAT off, forms[6] = down + the next layer's q/k/v inside the
 * attention launch as well (of any layer) */
extern "C" int omx_qwen3_debug_step_forms(omx_qwen3 m, int* forms) {
    OMX_REQUIRE(m && forms, "omx_qwen3_debug_step_forms: null argument");
    forms[0] = omx::down_takes_qkv(m) ? 1 : 0;
    forms[1] = omx::any_layer_takes_oproj(m) ? 1 : 0;
    forms[2] = omx::step_engine_mode(m);
    forms[3] = m->chain_disabled ? 1 : 0;
    forms[4] = 0;
    for (int l = 0; l < m->cfg.num_hidden_layers; ++l) forms[4] |= omx::attention_takes_gateup(m, l) ? 1 : 0;
    forms[5] = m->gateup_disabled ? 1 : 0;
    forms[6] = 0;
    for (int l = 0; l < m->cfg.num_hidden_layers; ++l) forms[6] |= omx::attention_takes_down(m, l) ? 1 : 0;
    return 0;
}

/* raise, from the host, the word a wait inside a launch raises when it gives up: the next omx_qwen3_decode finds its steps void and goes
 * down the fallback ladder (step_fallback) exactly as after a real give-up -- without starving a launch to provoke one */
extern "C" int omx_qwen3_debug_raise_give_up(omx_qwen3 m) {
    OMX_REQUIRE(m, "omx_qwen3_debug_raise_give_up: null argument");
    const unsigned one = 1u;
    OMX_HIP_CHECK(hipMemcpyAsync(m->wait_abort, &one, 4, hipMemcpyHostToDevice, m->stream));
    OMX_HIP_CHECK(hipStreamSynchronize(m->stream));
    return 0;
}
