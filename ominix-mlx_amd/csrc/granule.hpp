// Data-tagged 8-byte granules {32-bit payload, 32-bit tag}: the in-launch hand-off of the decode step's kernels (attn_step.hip: split
// partials and the merged attention vector; gemv_chain.hip: the residual row between down and the next layer's q/k/v).
// A producer writes a granule with ONE relaxed agent-scope 8-byte store (write-through: no store-ack wait, no arrival counter, no flag);
// a consumer re-reads it with relaxed agent-scope loads until the tag matches (cdna_hip_programming.md Guideline 16, form R2).  The tag
// is derived from the step sequence number, so nothing has to be reset between launches.
// Who calls what: st_granule* / ld_granule -- attn_step.hip, gemv_chain.hip; sweep_granules -- gemv_chain.hip (wave 0 of
// down_qkv_kernel: the residual row; attn_step.hip's down_qkv_phase writes this text out for the activation vector, half per sweeping wave,
// and for the residual row, for the first pass's counted wait); kGranuleSpinLimit -- every bounded wait of those two files.
#pragma once
#include "common.hpp"

namespace omx {

typedef __attribute__((address_space(1))) unsigned long long gu64;

__device__ __forceinline__ void st_granule_u32(uint64_t* p, unsigned tag, unsigned v) {
    __hip_atomic_store((gu64*)p, ((unsigned long long)tag << 32) | (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_granule(uint64_t* p, unsigned tag, float v) { st_granule_u32(p, tag, __float_as_uint(v)); }
__device__ __forceinline__ unsigned long long ld_granule(const uint64_t* p) {
    return __hip_atomic_load((gu64*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}


constexpr unsigned kGranuleSpinLimit = 1u << 15;   // passes (~1 us each) before a wait gives up

// a wave brings its share -- part `part` of NW -- of a vector of `N2` granules into LDS (natural element order): it watches one granule per
// lane politely (the last of every GPL-th run of its share), then asks for all of its GPL granules per lane in ONE pass (a pass is a round trip
// through a memory system that is busy with the weight streams: three passes of 32 cost the activation hop 8 us, EXPERIMENTS C-4) and
// re-reads them until every tag matches; a wait that gives up raises abort_flag
template <int N2, int NW>
__device__ __forceinline__ void sweep_granules(const uint64_t* gr, unsigned* sx, int part, unsigned tag, int lane, unsigned* abort_flag) {
    constexpr int GPL = N2 / NW / 64;   // granules per lane
    static_assert(N2 % (NW * 64) == 0 && GPL <= 48, "whole lanes, at most 96 registers of granules");
    gr += (size_t)part * (N2 / NW);
    sx += part * (N2 / NW);
    for (unsigned spins = 0; spins < kGranuleSpinLimit; ++spins) {
        const unsigned long long g = ld_granule(gr + (size_t)lane * GPL + (GPL - 1));
        if (__all((unsigned)(g >> 32) == tag)) break;
        __builtin_amdgcn_s_sleep(4);
    }
    unsigned long long g[GPL];
    for (unsigned spins = 0;; ++spins) {
#pragma unroll
        for (int i = 0; i < GPL; ++i) g[i] = ld_granule(gr + (size_t)i * 64 + lane);
        bool ok = true;
#pragma unroll
        for (int i = 0; i < GPL; ++i) ok &= (unsigned)(g[i] >> 32) == tag;
        if (__all(ok)) break;
        if (spins >= kGranuleSpinLimit) {   // a producer never showed up: void result, loud flag, no hang
            if (lane == 0) __hip_atomic_store(abort_flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            break;
        }
        __builtin_amdgcn_s_sleep(4);
    }
#pragma unroll
    for (int i = 0; i < GPL; ++i) sx[i * 64 + lane] = (unsigned)g[i];
}

}  // namespace omx
