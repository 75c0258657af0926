// Data-tagged 8-byte granules {32-bit payload, 32-bit tag}: the in-launch hand-off of the decode step's kernels (attn_step.hip: split
// partials and the merged attention vector; gemv_chain.hip: the residual row between down and the next layer's q/k/v).
// A producer writes a granule with ONE relaxed agent-scope 8-byte store (write-through: no store-ack wait, no arrival counter, no flag);
// a consumer re-reads it with relaxed agent-scope loads until the tag matches (cdna_hip_programming.md Guideline 16, form R2).  The tag
// is derived from the step sequence number, so nothing has to be reset between launches.
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

}  // namespace omx
