// Step state of the decode engine: lives in device memory so that a captured step never needs host patching (engine.hip).
#pragma once
#include "common.hpp"

namespace omx {

struct StepState {
    int pos;               // tokens in the cache == RoPE offset of the token being processed
    uint32_t cur_token;    // token fed to the embedding this step
    int out_count;         // tokens sampled so far
    int prompt_idx;        // next prompt token to feed during a token-serial prefill
};

// One slot of a batch object (engine_batch.hip) in device memory: the step's kernels read and advance it there, so that the steps of
// one omx_qwen3_batch_decode call follow each other without the host.
struct BatchSlot {
    int pos;               // tokens in the slot's cache == RoPE offset of the pending token
    uint32_t pending;      // token the slot's next step feeds to the embedding
    uint32_t rng[4];       // the slot's sampler: [0..1] key-sequence state, [2..3] key of the current draw (as omx_qwen3_::rng)
    int owner;             // the slot whose slabs hold the span this slot shares (omx_qwen3_batch_fork); itself when it shares nothing
    int shared_len;        // rows [0, shared_len) of this slot's slabs and of owner's hold the same bits; a multiple of the split width
};

}  // namespace omx
