// replica_cost.h -- the DEVICE side of what the engines that advance R seeded runs of one instance in one engine share
// (dsa.hip, mgm.hip, mgm2.h, gdba.h; the host side, which launches these kernels, is replica_host.h): the fold of the
// replica into blockIdx.x, the solution cost of every replica's current assignment reduced on the device, and the
// best state a replica has shown (BestRec, k_best_copy: the engines that track it, DSA and GDBA).  G is the engine's
// Dev: it carries n_vars, bpr (blocks per replica of the launch being made), the CSR arrays
// of the constraints (factor_rowptr, edge_var, dom_size, table_off, tables) and q (graph index -> position in the
// dynamic state); the values are passed beside it, [replicas][n_vars] in the engine's order (q).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace repcost {

constexpr int MAX_REPLICAS = 4096;

// the replica of this block and the block's index inside the replica (block-uniform): block = replica * bpr + b.
// REP = false: the instantiation for ONE replica -- nothing is derived from blockIdx.x, the code of a single-run
// engine is what it was before there were replicas.
template <bool REP, typename G>
__device__ inline int replica_of_block(const G& g, int* b) {
    if constexpr (!REP) {
        *b = (int)blockIdx.x;
        return 0;
    } else {
        const int r = (int)(blockIdx.x / (unsigned)g.bpr);
        *b = (int)blockIdx.x - r * g.bpr;
        return r;
    }
}

// ---- the solution cost of every replica's current assignment (HostGraph::eval_cost = DCOP.solution_cost):
// the constraints' entries plus the variables' own eval_var_cost, an entry equal to `infinity` counted as a
// violation instead.  Items = the constraints, then the variables.  FIXED SHAPE: a thread folds COST_RUN
// consecutive items in index order, the block's COST_TPB sums are combined by one tree in LDS, the block's
// partial goes to part[r][b]; k_cost_final adds a replica's partials in index order.  No atomics: the same
// bits from run to run.  Sums in f64; the tables are the engine's (T): in f32 mode the cost is that of the
// narrowed tables (eval_var_cost is kept in f64).
constexpr int COST_TPB = 256, COST_RUN = 4;
struct CostArgs {
    const int32_t* cur;      // [n_rep][n_vars] the values, in packed order
    const int64_t* coff;     // [n_vars + 1] offsets into evc
    const double* evc;       // eval_var_cost
    int32_t n_factors;
    double infinity;
    double* part_cost;       // [n_rep][bpr]
    long long* part_viol;
};
template <typename G>
__global__ void __launch_bounds__(COST_TPB) k_cost_partial(G g, CostArgs a) {
    __shared__ double s_cost[COST_TPB];
    __shared__ long long s_viol[COST_TPB];
    int b;
    const int r = replica_of_block<true>(g, &b);
    const int32_t* cur = a.cur + (int64_t)r * g.n_vars;
    const int t = (int)threadIdx.x;
    const int64_t n_items = (int64_t)a.n_factors + g.n_vars;
    const int64_t i0 = ((int64_t)b * COST_TPB + t) * COST_RUN;
    double soft = 0.0;
    long long hard = 0;
    for (int64_t i = i0; i < i0 + COST_RUN && i < n_items; ++i) {
        double e;
        if (i < a.n_factors) {
            const int f = (int)i;
            int64_t lin = 0;
            for (int k = g.factor_rowptr[f]; k < g.factor_rowptr[f + 1]; ++k) {
                const int u = g.edge_var[k];
                lin = lin * g.dom_size[u] + cur[g.q[u]];
            }
            e = (double)g.tables[g.table_off[f] + lin];
        } else {
            const int v = (int)(i - a.n_factors);
            e = a.evc[a.coff[v] + cur[g.q[v]]];
        }
        if (e != a.infinity) soft += e;
        else hard += 1;
    }
    s_cost[t] = soft;
    s_viol[t] = hard;
    __syncthreads();
    for (int s = COST_TPB / 2; s > 0; s >>= 1) {
        if (t < s) {
            s_cost[t] += s_cost[t + s];
            s_viol[t] += s_viol[t + s];
        }
        __syncthreads();
    }
    if (t == 0) {
        a.part_cost[(int64_t)r * g.bpr + b] = s_cost[0];
        a.part_viol[(int64_t)r * g.bpr + b] = s_viol[0];
    }
}

// the best state a replica has shown (rephost::BestTracker): the record and the snapshot, in the order of the state
struct BestRec {
    double* cost;          // [n_rep]
    long long* viol;
    long long* cycle;      // the engine's cycle or round of the record
    int32_t* improved;     // [n_rep] written by k_cost_final, read by the copy kernel (the next launch)
    int32_t* idx;          // [n_rep][n_vars]
};
// thread per replica: the partials in index order; mode 0: the costs alone, 1: improved[r] = the current state
// is STRICTLY better than the record (fewer violations, or as many and a lower -- max: higher -- cost),
// 2: improved[r] = 1 (the first record).  The record itself is not touched here.  (A template so that the
// header can be included by more than one unit.)
template <typename Rec>
__global__ void __launch_bounds__(64) k_cost_final(int n_rep, int n_blocks, int is_max, const double* part_cost,
                                                   const long long* part_viol, double* cost, long long* viol, int mode,
                                                   Rec best) {
    const int r = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (r >= n_rep) return;
    double soft = 0.0;
    long long hard = 0;
    for (int b = 0; b < n_blocks; ++b) {
        soft += part_cost[(int64_t)r * n_blocks + b];
        hard += part_viol[(int64_t)r * n_blocks + b];
    }
    cost[r] = soft;
    viol[r] = hard;
    if (mode == 2) {
        best.improved[r] = 1;
    } else if (mode == 1) {
        const long long bv = best.viol[r];
        const double bc = best.cost[r];
        best.improved[r] = (hard < bv || (hard == bv && (is_max ? soft > bc : soft < bc))) ? 1 : 0;
    }
}

// a launch of its own, after k_cost_final in stream order: the replicas that improved copy their state (as stored)
// and take the new record; nothing in this launch reads a record.  Blocks of BEST_TPB threads, bpr per replica.
// (A template for the same reason.)
constexpr int BEST_TPB = 256;
template <typename Rec>
__global__ void __launch_bounds__(BEST_TPB) k_best_copy(int n_vars, int bpr, const int32_t* cur, const double* cost,
                                                        const long long* viol, long long cycle, Rec best) {
    const int r = (int)(blockIdx.x / (unsigned)bpr);
    const int b = (int)blockIdx.x - r * bpr;
    if (!best.improved[r]) return;
    const int i = b * (int)blockDim.x + (int)threadIdx.x;
    if (i < n_vars) best.idx[(int64_t)r * n_vars + i] = cur[(int64_t)r * n_vars + i];
    if (i == 0) {
        best.cost[r] = cost[r];
        best.viol[r] = viol[r];
        best.cycle[r] = cycle;
    }
}

// (violations, cost -- negated in max mode --, index): the lexicographic minimum
inline int best_replica(int n_rep, bool is_max, const double* hc, const long long* hv) {
    int best = 0;
    for (int r = 1; r < n_rep; ++r) {
        const double a = is_max ? -hc[r] : hc[r], b = is_max ? -hc[best] : hc[best];
        if (hv[r] < hv[best] || (hv[r] == hv[best] && a < b)) best = r;
    }
    return best;
}

}  // namespace repcost
