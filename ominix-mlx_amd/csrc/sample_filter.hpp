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

// ---- the rows of a batch step (engine_batch.hip), each under its own slot's settings ----
int check_sampling(const char* who, const omx_sampling* p, int V);   // the parameter ranges of omx_sample_filtered, refused in `who`'s name
bool sampling_filters(const omx_sampling& p, int V);                 // a penalty, or (temperature != 0) a top-k / top-p that prunes
struct RowRule {
    float inv_temp, rep, pres;
};
constexpr int kBatchFilterRows = 8;
struct BatchFilterRow {   // one row's settings, by value in the launch arguments
    RowRule rule;
    int top_k;
    float top_p;
    uint8_t* seen;        // the slot's history row ([V] bytes), read by the penalties and marked with the drawn token; null: no penalty
    uint8_t k_on, p_on, greedy;
};
BatchFilterRow batch_filter_row(const omx_sampling& p, int V, uint8_t* seen_row);
struct BatchFilterArgs {
    const bf16_t* rows;        // [M, V] logits of this step
    bf16_t* slot_logits;       // [n_slots, V]
    BatchSlot* slots;
    const int* row_slot;
    uint32_t* ring;            // this step's [M] entries
    void* ws;                  // [M] x sample_select_ws_bytes(), zero before the first call (vocabulary-sized rows)
    int V;
    BatchFilterRow row[kBatchFilterRows];
};
// What batch_sample_kernel (engine_batch.hip) does for M rows -- row kept as the slot's logits, token from the NEXT key of the slot's
// sequence, ring / pending / pos / key state advanced -- with the draw under row r's own rule and the token marked in its history.
// Short rows: ONE launch, a block per row.  Vocabulary-sized rows: [max] [hist per level] [resolve] [noise] [finalize], the launches
// the union of the rows' settings needs, grid.y = the row; a row leaves a launch its own settings do not need.
int launch_batch_filtered(const BatchFilterArgs& a, int M, hipStream_t s);

}  // namespace omx
