// anytime.h -- the DEVICE side of the Max-Sum engine's best-state record and cost trace (mxs_track_best,
// include/maxsum_gpu_anytime.h; the host side is Engine::launch_track in engine.hip).  One evaluation is three
// launches in stream order: k_eval (kernels.h, as mxs_eval_cost launches it) leaves the per-block partials,
// k_any_final folds them and decides, k_any_copy takes the snapshot.  Nothing is read back and nothing is an
// atomic: one thread finalises, the same bits from run to run.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mxs {

constexpr int ANY_MAX_PARTS = 1024;  // the most blocks k_eval is launched with (Engine::EVAL_BLOCKS)
constexpr int ANY_TPB = 256;

// the engine's one record, on the device
struct AnyState {
    long long next_cycle;  // the cycle of the next periodic evaluation: a captured graph freezes kernel arguments, so
                           // the cycle number of an evaluation inside a replay comes from here
    long long evals;       // evaluations since the trace was cleared (stored or not)
    double best_cost;
    long long best_viol, best_cycle;
    double cur_cost;       // the evaluation k_any_final has just made, for k_any_copy
    long long cur_viol, cur_cycle;
    int32_t improved, pad;
};

struct AnyTrace {
    long long* cycle;  // [cap]
    double* cost;
    long long* viol;
    int32_t cap;
};

// One block.  The partials are staged in LDS by all threads (coalesced), then thread 0 adds them in index order:
// the order of the host loop of mxs_eval_cost, so the cost has the same bits.  first_cycle >= 0: a first record at
// that cycle -- taken whatever its cost -- and the periodic evaluations carry on from the next multiple of `every`;
// first_cycle < 0: the periodic evaluation at next_cycle.  The record is replaced on STRICT improvement only (fewer
// violations, or as many and a lower -- max: higher -- cost; the rule of repcost::k_cost_final), never by a NaN cost.
static __global__ void __launch_bounds__(ANY_TPB) k_any_final(int nb, int is_max, const double* part_cost,
                                                              const unsigned long long* part_viol, long long first_cycle,
                                                              int every, AnyState* st, AnyTrace tr) {
    __shared__ double s_cost[ANY_MAX_PARTS];
    __shared__ unsigned long long s_viol[ANY_MAX_PARTS];
    for (int b = (int)threadIdx.x; b < nb; b += ANY_TPB) {
        s_cost[b] = part_cost[b];
        s_viol[b] = part_viol[b];
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double soft = 0.0;
    long long hard = 0;
    for (int b = 0; b < nb; ++b) {
        soft += s_cost[b];
        hard += (long long)s_viol[b];
    }
    const bool first = first_cycle >= 0;
    const long long cyc = first ? first_cycle : st->next_cycle;
    st->next_cycle = first ? (first_cycle / every + 1) * every : cyc + every;
    const long long k = st->evals;
    if (k < tr.cap) {
        tr.cycle[k] = cyc;
        tr.cost[k] = soft;
        tr.viol[k] = hard;
    }
    st->evals = k + 1;
    st->cur_cost = soft;
    st->cur_viol = hard;
    st->cur_cycle = cyc;
    const long long bv = st->best_viol;
    const double bc = st->best_cost;
    const bool better = soft == soft && (hard < bv || (hard == bv && (is_max ? soft > bc : soft < bc)));
    st->improved = (first || better) ? 1 : 0;
}

// A launch of its own behind k_any_final: when the state improved, `sel` (internal order) becomes the snapshot and
// the evaluation becomes the record.  Nothing in this launch reads a record.
static __global__ void __launch_bounds__(ANY_TPB) k_any_copy(int n_vars, const int32_t* sel, int32_t* snap, AnyState* st) {
    if (!st->improved) return;
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < n_vars) snap[i] = sel[i];
    if (i == 0) {
        st->best_cost = st->cur_cost;
        st->best_viol = st->cur_viol;
        st->best_cycle = st->cur_cycle;
    }
}

}  // namespace mxs
