// The top-n form of the per-row log-probability (logprob.hip) as the decode steps launch it: two launches over rows of bf16 logits with
// the caller's own scratch, every argument fixed at enqueue time (a captured step replays them unchanged).
#pragma once
#include "common.hpp"

namespace omx {

// Where the merge launch of the top-n form writes.  Row r of the launch goes to entry r of logprobs / greedy / lse and to entries
// [r, 0 .. top_n) of top_ids / top_lp.  ring_count set: ONE row, written at entry (*ring_count - 1) % ring_cap instead -- the entry of
// the token a step's finalize has just counted, read on the device.  row_slot set: a second copy at entry row_slot[r] of slot_lp /
// slot_ids / slot_top (a batch's last values per slot).
struct LogprobTopOut {
    float* logprobs;
    uint32_t* greedy;        // nullable
    float* lse;              // nullable
    uint32_t* top_ids;       // [.., top_n]; unused when top_n == 0
    float* top_lp;
    const int* ring_count;   // nullable
    int ring_cap;
    const int* row_slot;     // nullable
    float* slot_lp;
    uint32_t* slot_ids;
    float* slot_top;
};

// bytes of scratch the two launches need for `rows` rows of V columns
size_t logprob_top_scratch_bytes(int64_t rows, int V, int top_n);

// [chunk partials (+ the chunks' top_n candidates)] [merge (+ the row's top_n)] over logits [rows, ld] bf16; targets: device u32 [rows].
// 0 <= top_n <= OMX_LOGPROBS_MAX_TOP (0: the target's log-probability only, the plain partial kernel).  Shapes as omx_logprob_rows.
int launch_logprob_top(const LogprobTopOut& out, void* scratch, const bf16_t* logits, int64_t ld, const uint32_t* targets, int64_t rows,
                       int V, int top_n, hipStream_t s);

}  // namespace omx
