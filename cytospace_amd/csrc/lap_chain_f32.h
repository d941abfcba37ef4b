// lap_chain_f32.h -- the interface between the float32 driver (lap_jv.hip) and the float32 chain solver (lap_chain_f32.hip).
#pragma once
#include "cyto_common.h"
#include "lap_dev.h"
#include "lap_wide.h"
#include <vector>

namespace cyto {

// A problem of the batch is a SolveJob (lap_wide.h) whose `state` points to CHAIN_STATE_BUFS buffers of the caller: the per-group
// state of jv_chain2 / jv_aug2 (best offsets, stamps) and of jv_aug_lazy (the same two), allocated here only where that state
// misses LDS.
constexpr int CHAIN_STATE_BUFS = 4;

struct ChainPlan {
    int n;
    CachePlan cache;
    // cyto_lap_opts, as given: chain_variant, augmentation, no_handover, inject_exceptions, group_state_global, aux_state_global
    int variant, augmentation, no_handover, inject_exceptions, group_state_global, aux_state_global;
    DevBuf *args;                       // [2] the argument blocks of the batch: the caller's, so that they outlive its last
                                        // synchronisation of the stream; allocated here
};
// The chain solve of a batch after its column reduction: reduction transfer and row reduction (jv_chain2), then the augmentation
// (jv_aug2, or jv_aug_lazy with jv_aug2 taking over the searches it gives up) -- one launch per phase, a workgroup per problem.
// ev_cache_done is recorded behind the first cache build, ev_arr_done behind jv_chain2.
int chain_solve_batch(const ChainPlan &pl, const std::vector<SolveJob> &jobs, hipStream_t stream, hipEvent_t ev_cache_done,
                      hipEvent_t ev_arr_done);
// the chain solver's fields of cyto_lap_info (the driver has zeroed it)
void chain_info(cyto_lap_info *info, const ChainPlan &pl, const LapStatus &h);

}  // namespace cyto
