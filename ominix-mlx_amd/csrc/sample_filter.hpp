// Filtered sampling (sample_filter.hip): engine hooks.
#pragma once
#include "common.hpp"
#include "step_state.hpp"

namespace omx {

size_t sample_select_ws_bytes();   // device scratch of the selection (histograms per level, the descent's carried state)
// [select]: [max, with top-p] [one histogram launch per level: 3 for top-k, 3 for top-p, the first shared] [resolve: threshold -> ws,
// histograms cleared for the next call]; nothing when the parameters filter nothing.  ws must be ZERO before the first call
// (hipMemsetAsync of sample_select_ws_bytes()) and after a call that failed midway.
int launch_sample_select(void* ws, const bf16_t* logits, bool logits_f16, int V, const omx_sampling& p, const uint8_t* seen,
                         hipStream_t s);
// [noise] n_partials blocks: (value, ~index) partials over the kept set the selection left in ws;
// temperature 0 = no noise (argmax of the penalised logits)
int launch_sample_filtered_noise(unsigned long long* partials, int n_partials, const bf16_t* logits, bool logits_f16, int V,
                                 const omx_sampling& p, const uint8_t* seen, void* ws, const uint32_t* sub_key, hipStream_t s);
// [mark] seen[st->cur_token] = 1 (after the finalize of the step)
int launch_mark_seen(uint8_t* seen, int V, const StepState* st, hipStream_t s);

}  // namespace omx
