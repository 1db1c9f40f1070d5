// dsa.hip -- the reference's DSA (pydcop/algorithms/dsa.py: variants A, B, C; Zhang & al. 2005)
// on gfx950, on the same flat factor-graph arrays as the Max-Sum engine (SURVEY.md section
// 8(f).4).  DSA is bulk-synchronous by construction (a computation evaluates a cycle once ALL
// its neighbours' values of that cycle are in and parks the next ones, dsa.py:300-317): one cycle =
// ONE launch, reading the neighbours' values of the previous cycle and the variable's constraints'
// tables at them -- on the PACKED view (local_search.h: one lane per (variable, constraint), unary /
// binary constraints over domains of at most four values) where the instance allows it, thread per
// variable on the slot view or the CSR walk otherwise; bit-identical results.  The dynamic state lives
// in packed order (Dev::q).
//
// REPLICAS: one engine advances R seeded runs of the instance with the same launches (the restarts a user of
// a randomised local search makes anyway).  Everything static -- CSR arrays, slot view, row view, packed
// records, tables, f_opt, prob -- is stored once; the dynamic state is [R][n_vars] (cur[2], cost), the seeds
// are a device array, the packed kernel's keys are [R][packed variables].  The replica is folded into
// blockIdx.x (block = replica * blocks_per_replica + block of the replica): whole blocks belong to one
// replica, everything a kernel derives from the replica is block-uniform (R = 1 runs instantiations without it).  Replica r is bit for bit the
// single-seed run with seed seeds[r]; mxs_dsa_create is R = 1 of the same path.  Per replica, the solution
// cost of the current assignment is reduced on the device (replica_cost.h, shared with mgm.hip: fixed
// shape, no atomics) and the best state seen can be kept on the device (rephost::BestTracker, repcost::k_best_copy).
// The host side that does not depend on the algorithm -- set-up, views, uploads, start values, the cost launches,
// the best-state records -- is rephost::Host and rephost::BestTracker (replica_host.h, shared with mgm.hip); this
// file keeps the kernels, Dev, the per-lane extras and the cycle's launches.
//
// The reference draws from Python's unseeded `random` module (initial value, move test, choice
// among the best values).  Here every draw comes from a counter-based generator keyed on (seed,
// variable, cycle, draw) -- uniform() of engine_common.h, the same function in oracle/dsa_oracle.c and, patched into
// the reference's `random` for the duration of a run, in oracle/ref_harness.py -- so that the
// stochastic algorithm has a pinned parity: bit for bit the reference's own DsaComputation objects
// under that generator (tests/test_dsa_oracle_vs_reference.py), independent of scheduling.  The
// reference's quirks are restated as they are (variable costs never enter, initial values are
// ignored, the held cost is 0 until the first move): see oracle/dsa_oracle.c.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/maxsum_gpu.h"
#include "engine_common.h"
#include "local_search.h"
#include "replica_cost.h"
#include "replica_host.h"

namespace dsa {

using mxs_host::Buf;
using mxs_host::fail;
using mxs_host::uniform;            // draws 0 (start value), 1 (move test), 2 (choice among the best values)
using mxs_host::uniform_from_key;
using mxs_host::uniform_key;

constexpr int TPB = 64;  // one wave per block: 100k variables spread over every CU (latency-bound CSR walks)

template <typename T>
struct Dev {
    int32_t n_vars, is_max, variant;
    int32_t bpr;          // blocks per replica of the launch being made (block = replica * bpr + b)
    int32_t n_pack;       // packed variables (the row length of pack_key)
    const uint64_t* seeds;  // [replicas]
    int64_t cycle;        // cycle_count of the evaluation being made
    const int32_t *dom_size, *factor_rowptr, *edge_var, *edge_factor, *var_rowptr, *var_edges, *n_neigh;
    const int64_t* table_off;
    const T *tables, *f_opt;
    const double* prob;
    const int32_t* cur;          // [replicas][n_vars], as cur_out and cost: replica r at + r * n_vars (64-bit)
    int32_t* cur_out;
    T* cost;
    lsearch::Slots slots;
    lsearch::Pack pack;          // the packed view (local_search.h): lane per (variable, constraint)
    const T* pack_fopt;          // [lanes] optimum of the lane's constraint (variant B)
    const int32_t* var_list;     // the variables a thread-per-variable launch works on (NULL: all)
    int32_t n_list;
    // The dynamic state (cur, cost) is stored in PACKED ORDER, position q[v] = the variable's rank in the
    // packed view's wave order (the others after them): a packed wave's variables are q = first ..
    // first + nv - 1, what lane k = 0 of each reads and writes of its own state is one line per array
    // instead of one per variable (mgm.hip, Dev::q).  The packed view holds positions (nb); the
    // thread-per-variable kernels translate through q[]; the random draws stay keyed on graph indices.
    const int32_t* q;
    const int32_t* pack_dom;               // [packed variables] dom_size, in packed order
    const uint64_t* pack_key;              // [replicas][packed variables] uniform_key(seeds[r], graph index): the draws' key
    const double* pack_prob;               // [packed variables] the change probability
};

using repcost::replica_of_block;   // block = replica * bpr + b (replica_cost.h); REP = false: one replica, nothing derived

template <typename T>
__device__ T constraint_at(const Dev<T>& g, const int32_t* cur, int f, int v, int x) {
    int64_t lin = 0;
    for (int e = g.factor_rowptr[f]; e < g.factor_rowptr[f + 1]; ++e) {
        const int u = g.edge_var[e];
        lin = lin * g.dom_size[u] + (u == v ? x : cur[g.q[u]]);
    }
    return g.tables[g.table_off[f] + lin];
}

// assignment_cost (relations.py:1513-1533): cost = 0; cost += c(...) in constraints order
template <typename T>
__device__ T assignment_cost(const Dev<T>& g, const int32_t* cur, int v, int x) {
    T cost = (T)0;
    for (int k = g.var_rowptr[v]; k < g.var_rowptr[v + 1]; ++k)
        cost += constraint_at(g, cur, g.edge_factor[g.var_edges[k]], v, x);
    return cost;
}

// evaluate_cycle, dsa.py:319-359 + variant_a/b/c :361-409 + probabilistic_change :411-419
template <typename T, bool REP>
__global__ void __launch_bounds__(TPB) k_dsa_cycle(Dev<T> g) {
    int b;
    const int r = replica_of_block<REP>(g, &b);
    const int tid = b * (int)blockDim.x + (int)threadIdx.x;
    if (tid >= g.n_list) return;
    const int64_t roff = (int64_t)r * g.n_vars;
    const int32_t* cur = g.cur + roff;
    const uint64_t seed = g.seeds[r];
    const int v = g.var_list ? g.var_list[tid] : tid;
    const int qv = g.q[v];
    const int mine = cur[qv];
    int out = mine;
    if (g.n_neigh[v] != 0) {
        const int D = g.dom_size[v];
        T best_cost = g.is_max ? -(T)INFINITY : (T)INFINITY;   // find_optimal, relations.py:1622-1638
        int n_best = 0, first_best = -1;
        bool has_cur = false;
        for (int x = 0; x < D; ++x) {
            const T c = assignment_cost(g, cur, v, x);
            if (c == best_cost) {
                n_best += 1;
                if (x == mine) has_cur = true;
            } else if ((!g.is_max && c < best_cost) || (g.is_max && c > best_cost)) {
                best_cost = c;
                n_best = 1;
                first_best = x;
                has_cur = x == mine;
            }
        }
        const T current_cost = assignment_cost(g, cur, v, mine);
        const T diff = current_cost - best_cost;
        const T delta = diff < (T)0 ? -diff : diff;
        bool attempt = false, drop_cur = false;
        if (delta > (T)0) {
            attempt = true;
        } else if (delta == (T)0) {
            if (g.variant == 1) {  // B: some constraint is not at its optimum (dsa.py:421-433)
                for (int k = g.var_rowptr[v]; k < g.var_rowptr[v + 1] && !attempt; ++k) {
                    const int f = g.edge_factor[g.var_edges[k]];
                    if (constraint_at(g, cur, f, v, mine) != g.f_opt[f]) attempt = true;
                }
            } else if (g.variant == 2) {
                attempt = true;
            }
            if (attempt && n_best > 1 && has_cur) drop_cur = true;  // best_values.remove(current_value)
        }
        if (attempt && g.prob[v] > uniform(seed, v, g.cycle + 1, 1)) {
            const int n = n_best - (drop_cur ? 1 : 0);
            int j = (int)(uniform(seed, v, g.cycle + 1, 2) * n);
            int pick = first_best;
            for (int x = 0; x < D; ++x) {  // the j-th best value in domain order, the current one skipped
                if (assignment_cost(g, cur, v, x) != best_cost) continue;
                if (drop_cur && x == mine) continue;
                if (j-- == 0) {
                    pick = x;
                    break;
                }
            }
            out = pick;
            g.cost[roff + qv] = best_cost;  // value_selection(choice, best_cost)
        }
    }
    g.cur_out[roff + qv] = out;
}

// the same cycle on the slot view (local_search.h): the D costs in registers, one pass over the
// variable's constraints instead of 2D+1 CSR walks; domains of at most MAXD values
template <typename T, int MAXD, bool REP>
__global__ void __launch_bounds__(TPB) k_dsa_cycle_slots(Dev<T> g) {
    int b;
    const int r = replica_of_block<REP>(g, &b);
    const int tid = b * (int)blockDim.x + (int)threadIdx.x;
    if (tid >= g.n_list) return;
    const int64_t roff = (int64_t)r * g.n_vars;
    const int32_t* cur = g.cur + roff;
    const uint64_t seed = g.seeds[r];
    const int v = g.var_list ? g.var_list[tid] : tid;
    const int qv = g.q[v];
    const int mine = cur[qv];
    int out = mine;
    if (g.n_neigh[v] != 0) {
        const int D = g.dom_size[v];
        const int s0 = g.var_rowptr[v], s1 = g.var_rowptr[v + 1];
        T c[MAXD];
        if (g.slots.rows != nullptr && s0 < s1 && g.slots.row_base[s0] >= 0) {  // contiguous rows (local_search.h)
            if (g.slots.rows_int8) lsearch::costs_of_values_rows<T, int8_t, MAXD>(g.slots, cur, s0, s1, D, true, c);
            else lsearch::costs_of_values_rows<T, T, MAXD>(g.slots, cur, s0, s1, D, true, c);
        } else {
            lsearch::costs_of_values<T, MAXD>(g.slots, g.tables, cur, s0, s1, D, true, c);
        }
        T best_cost = g.is_max ? -(T)INFINITY : (T)INFINITY;
        int n_best = 0, first_best = -1;
        bool has_cur = false;
#pragma unroll
        for (int x = 0; x < MAXD; ++x)
            if (x < D) {
                if (c[x] == best_cost) {
                    n_best += 1;
                    if (x == mine) has_cur = true;
                } else if ((!g.is_max && c[x] < best_cost) || (g.is_max && c[x] > best_cost)) {
                    best_cost = c[x];
                    n_best = 1;
                    first_best = x;
                    has_cur = x == mine;
                }
            }
        const T diff = lsearch::pick<T, MAXD>(c, mine) - best_cost;
        const T delta = diff < (T)0 ? -diff : diff;
        bool attempt = false, drop_cur = false;
        if (delta > (T)0) {
            attempt = true;
        } else if (delta == (T)0) {
            if (g.variant == 1) {
                for (int s = s0; s < s1 && !attempt; ++s) {
                    int64_t off = g.slots.base[s] + (int64_t)mine * g.slots.stride_v[s];
                    for (int k = g.slots.nb_rowptr[s]; k < g.slots.nb_rowptr[s + 1]; ++k)
                        off += (int64_t)cur[g.slots.nb_var[k]] * g.slots.nb_stride[k];
                    if (g.tables[off] != g.f_opt[g.edge_factor[g.var_edges[s]]]) attempt = true;
                }
            } else if (g.variant == 2) {
                attempt = true;
            }
            if (attempt && n_best > 1 && has_cur) drop_cur = true;
        }
        if (attempt && g.prob[v] > uniform(seed, v, g.cycle + 1, 1)) {
            const int n = n_best - (drop_cur ? 1 : 0);
            int j = (int)(uniform(seed, v, g.cycle + 1, 2) * n);
            int pick = first_best;
            bool done = false;
#pragma unroll
            for (int x = 0; x < MAXD; ++x)
                if (x < D && !done && c[x] == best_cost && !(drop_cur && x == mine)) {
                    if (j-- == 0) {
                        pick = x;
                        done = true;
                    }
                }
            out = pick;
            g.cost[roff + qv] = best_cost;
        }
    }
    g.cur_out[roff + qv] = out;
}

// the same cycle on the PACKED view (local_search.h): one lane per (variable, constraint), the
// constraint's entries for the neighbour's current value from the lane's private transposed
// record, the D costs by cross-lane sums in slot order; every lane of a variable then takes the
// same decision, lane k = 0 writes it.  TT = int8_t (records of small integers) or T.
constexpr int PACK_TPB = 256;
template <typename T, typename TT, bool REP>
__global__ void __launch_bounds__(PACK_TPB) k_dsa_cycle_pack(Dev<T> g) {
    constexpr int MAXD = lsearch::PACK_D;
    int b;
    const int r = replica_of_block<REP>(g, &b);
    const int64_t pos = (int64_t)b * blockDim.x + threadIdx.x;
    if (pos >= g.pack.n_lanes) return;  // whole waves (n_lanes is a multiple of 64)
    const int64_t roff = (int64_t)r * g.n_vars;
    const int32_t* cur = g.cur + roff;
    const lsearch::PackWave wm = g.pack.waves[__builtin_amdgcn_readfirstlane((int)(pos >> 6))];
    const uint32_t dn = (uint32_t)wm.deg_nv;
    const int deg = (int)(dn & 255u), nv = (int)((dn >> 8) & 255u);
    const int l = (int)threadIdx.x & 63;
    const int var = (int)(((uint32_t)l * (dn >> 16)) >> 15);  // l / deg (exact for l < 64)
    const int k = l - var * deg;
    const bool has = var < nv;
    const int qv = wm.first + (has ? var : 0);  // packed position: the index into the dynamic state
    const int seg = l - k;
    const int mine = cur[qv];
    const int D = g.pack_dom[qv];
    const uint64_t key = g.pack_key[(int64_t)r * g.n_pack + qv];     // the variable's key of the random draws (its graph index inside)
    const double prob = g.pack_prob[qv];     // requested with the others, used after the decision
    T t[MAXD], c[MAXD];
    lsearch::pack_costs<T, TT>(g.pack, cur, pos, deg, seg, true, t, c);
    T best_cost = g.is_max ? -(T)INFINITY : (T)INFINITY;   // find_optimal, relations.py:1622-1638
    int n_best = 0, first_best = -1;
    bool has_cur = false;
    // (selects, no branches: "equal" and "better" exclude each other)
#pragma unroll
    for (int x = 0; x < MAXD; ++x) {
        const bool in = x < D;
        const bool lt = c[x] < best_cost, gt = c[x] > best_cost;
        const bool eq = in & (c[x] == best_cost);
        const bool better = in & (g.is_max ? gt : lt);
        n_best = better ? 1 : n_best + (eq ? 1 : 0);
        first_best = better ? x : first_best;
        has_cur = better ? x == mine : (has_cur || (eq && x == mine));
        best_cost = better ? c[x] : best_cost;
    }
    const T diff = lsearch::pick<T, MAXD>(c, mine) - best_cost;
    const T delta = diff < (T)0 ? -diff : diff;
    // variant B (dsa.py:421-433): some constraint of the variable is not at its optimum -- the
    // lanes of the variable vote (a padding lane has no constraint)
    bool off_opt = false;
    if (g.variant == 1 && has) off_opt = lsearch::pick<T, MAXD>(t, mine) != g.pack_fopt[pos];
    const unsigned long long votes = __ballot(off_opt ? 1 : 0);
    const unsigned long long mine_mask = (deg >= 64 ? ~0ull : ((1ull << deg) - 1ull)) << seg;
    bool attempt = false, drop_cur = false;
    if (delta > (T)0) {
        attempt = true;
    } else if (delta == (T)0) {
        if (g.variant == 1) attempt = (votes & mine_mask) != 0ull;
        else if (g.variant == 2) attempt = true;
        if (attempt && n_best > 1 && has_cur) drop_cur = true;  // best_values.remove(current_value)
    }
    int out = mine;
    bool moved = false;
    if (attempt && prob > uniform_from_key(key, g.cycle + 1, 1)) {
        const int n = n_best - (drop_cur ? 1 : 0);
        int j = (int)(uniform_from_key(key, g.cycle + 1, 2) * n);
        int pick = first_best;
        bool done = false;
#pragma unroll
        for (int x = 0; x < MAXD; ++x)
            if (x < D && !done && c[x] == best_cost && !(drop_cur && x == mine)) {
                if (j-- == 0) {
                    pick = x;
                    done = true;
                }
            }
        out = pick;
        moved = true;
    }
    if (has && k == 0) {
        g.cur_out[roff + qv] = out;
        if (moved) g.cost[roff + qv] = best_cost;  // value_selection(choice, best_cost)
    }
}

// the start state of every replica: draw 0 of cycle 0 under seeds[r] (random_value_selection, dsa.py:291); a
// variable without neighbours takes its optimal_cost_value (iso_val >= 0, the same in every replica).  Both
// `cur` buffers: the packed launch writes only the variables that have neighbours.
constexpr int AUX_TPB = 256;
template <typename T>
__global__ void __launch_bounds__(AUX_TPB) k_dsa_init(Dev<T> g, const int32_t* iso_val, const T* iso_cost, int32_t* cur0,
                                                      int32_t* cur1) {
    int b;
    const int r = replica_of_block<true>(g, &b);
    const int v = b * (int)blockDim.x + (int)threadIdx.x;
    if (v >= g.n_vars) return;
    const int64_t at = (int64_t)r * g.n_vars + g.q[v];
    const int iso = iso_val[v];
    const int x = iso >= 0 ? iso : (int32_t)(uniform(g.seeds[r], v, 0, 0) * g.dom_size[v]);
    cur0[at] = x;
    cur1[at] = x;
    g.cost[at] = iso >= 0 ? iso_cost[v] : (T)0;
}

// ---- the solution cost of every replica's current assignment: k_cost_partial / k_cost_final of replica_cost.h,
// launched by replica_host.h (one implementation, shared with mgm.hip), as is the snapshot of the best state a
// replica has shown (mxs_dsa_track_best)

struct Base {
    virtual ~Base() {}
    virtual int init(const mxs_graph& G, const mxs_params& p, int variant, double probability, int arity_mode,
                     const uint64_t* seeds, int n_replicas, int device) = 0;
    virtual int reset() = 0;
    virtual int set_value_rank(const int32_t* rank) = 0;
    virtual int run(int32_t n) = 0;
    virtual int get_state(int32_t r, int32_t* idx, double* cost) = 0;
    virtual int eval_cost(const int32_t* idx, double infinity, double* cost, int64_t* viol) = 0;
    virtual int replica_costs(double infinity, double* cost, int64_t* viol) = 0;
    virtual int track_best(int32_t every, double infinity) = 0;
    virtual int get_best(int32_t r, int32_t* replica, int64_t* cycle, double* cost, int64_t* viol, int32_t* idx) = 0;
    int64_t cycles = 0;
    int32_t n_rep = 1;
};

using rephost::alloc_rep;
using rephost::blocks_of;
static_assert(TPB == rephost::VAR_TPB && PACK_TPB == rephost::PACK_TPB && AUX_TPB == rephost::AUX_TPB,
              "replica_host.h sizes its grid refusal by these");

template <typename T>
struct Engine : Base {
    // the stream, the graph, the views, the CSR arrays, the seeds, the start values, the device cost (replica_host.h)
    rephost::Host<T> rh;
    Dev<T> g{};
    int which = 0;
    Buf<int32_t> cur[2];    // [R][n_vars]
    Buf<T> f_opt, cost;
    Buf<double> prob;
    Buf<uint64_t> pk_key;   // what only DSA keeps per packed variable / lane (Dev::pack_key, pack_prob, pack_fopt)
    Buf<double> pk_prob;
    Buf<T> pk_fopt;
    rephost::BestTracker<T> bt;  // the best state every replica has shown (track_best, get_best)

    int init(const mxs_graph& G, const mxs_params& p, int variant, double probability, int arity_mode,
             const uint64_t* sds, int n_replicas, int dev) override {
        if (int rc = rh.open(sds, n_replicas, dev, true)) return rc;
        n_rep = rh.n_rep;
        if (variant < 0 || variant > 2) return fail(MXS_E_INVALID, "variant must be 0 (A), 1 (B) or 2 (C)");
        if (int rc = rh.hg.load(G, p)) return rc;  // (init_idx is not read: the reference's DSA ignores initial values)
        const mxs_host::HostGraph& hg = rh.hg;
        const hipStream_t stream = rh.stream;
        const int nV = hg.nV, nF = hg.nF;
        const size_t R = (size_t)n_rep;
        std::vector<int64_t> n_count(nV, 0);
        for (int f = 0; f < nF; ++f)
            for (int e = hg.frow[f]; e < hg.frow[f + 1]; ++e) n_count[hg.evar[e]] += hg.frow[f + 1] - hg.frow[f] - 1;
        std::vector<double> pr(nV);
        for (int v = 0; v < nV; ++v)  // p_mode arity: 1 / sum(arity - 1) * 1.2 (dsa.py:256-259)
            pr[v] = (arity_mode && n_count[v] > 0) ? 1.0 / (double)n_count[v] * 1.2 : probability;
        std::vector<T> fo(nF);
        for (int f = 0; f < nF; ++f) {  // find_optimum (relations.py:1367-1401) of the tables in T: variant B
            T opt = (T)hg.tables[hg.toff[f]];
            for (int64_t k = hg.toff[f] + 1; k < hg.toff[f + 1]; ++k) {
                const T x = (T)hg.tables[k];
                if (hg.is_max ? x > opt : x < opt) opt = x;
            }
            fo[f] = opt;
        }
        lsearch::HostSlots hs;
        lsearch::HostPack hp;
        if (int rc = rh.build_views(hs, hp)) return rc;
        // DSA's extras: per packed lane the optimum of its constraint, per packed variable its probability and, per
        // replica, the key of its draws
        const size_t nP = hp.vars.size();
        const std::vector<int32_t>& h_q = rh.h_q;
        std::vector<T> fopt_lane(hp.slot.size(), (T)0);
        for (size_t i = 0; i < hp.slot.size(); ++i)
            if (hp.slot[i] >= 0) fopt_lane[i] = fo[hg.efac[hg.vedges[hp.slot[i]]]];
        std::vector<double> pprob(nP);
        for (int v : hp.vars) pprob[h_q[v]] = pr[v];
        MXS_TRY(pk_prob.upload(pprob, stream));
        MXS_TRY(pk_fopt.upload(fopt_lane, stream));
        std::vector<uint64_t> pkey(R * nP);
        for (size_t r = 0; r < R; ++r)
            for (int v : hp.vars) pkey[r * nP + h_q[v]] = uniform_key(rh.h_seeds[r], v);
        if (int rc = alloc_rep(pk_key, R * nP, "keys")) return rc;
        if (!pkey.empty())
            MXS_TRY(hipMemcpyAsync(pk_key.p, pkey.data(), 8 * pkey.size(), hipMemcpyHostToDevice, stream));
        MXS_TRY(hipStreamSynchronize(stream));
        if (int rc = rh.upload_views(hs, hp)) return rc;
        if (int rc = rh.upload_graph()) return rc;
        MXS_TRY(f_opt.upload(fo, stream));
        MXS_TRY(prob.upload(pr, stream));
        for (int b = 0; b < 2; ++b)
            if (int rc = alloc_rep(cur[b], R * nV, "values")) return rc;
        if (int rc = alloc_rep(cost, R * nV, "held costs")) return rc;
        rh.bind(g);
        g.variant = variant;
        g.n_pack = (int32_t)nP;
        g.pack_key = pk_key.p;
        g.pack_prob = pk_prob.p;
        g.pack_fopt = pk_fopt.p;
        g.f_opt = f_opt.p; g.prob = prob.p; g.cost = cost.p;
        return reset();
    }

    int set_value_rank(const int32_t* rank) override {
        rh.set_value_rank(rank);
        return reset();
    }

    // every replica back to its start state (k_dsa_init); the records of track_best start again
    int reset() override {
        if (int rc = rh.start_values()) return rc;  // optimal_cost_value (dsa.py:278-289)
        which = 0;
        cycles = 0;
        if (g.n_vars) {
            g.bpr = blocks_of(g.n_vars, AUX_TPB);
            const dim3 grid((unsigned)(g.bpr * n_rep)), block(AUX_TPB);
            hipLaunchKernelGGL((k_dsa_init<T>), grid, block, 0, rh.stream, g, rh.iso_val.p, rh.iso_cost.p, cur[0].p, cur[1].p);
            MXS_TRY(hipGetLastError());
        }
        const int rc = bt.on_reset(rh, g, cur[which].p);
        MXS_TRY(hipStreamSynchronize(rh.stream));  // (also when the record failed)
        return rc;
    }

    // the launches of one cycle of all replicas: packed plus rest, or thread per variable alone
    template <bool REP>
    int launch_cycle(bool packed, bool generic) {
        const hipStream_t stream = rh.stream;
        if (packed) {
            g.bpr = blocks_of(g.pack.n_lanes, PACK_TPB);
            const dim3 pgrid((unsigned)(g.bpr * n_rep)), pblock(PACK_TPB);
            if (rh.pk.int8) hipLaunchKernelGGL((k_dsa_cycle_pack<T, int8_t, REP>), pgrid, pblock, 0, stream, g);
            else hipLaunchKernelGGL((k_dsa_cycle_pack<T, T, REP>), pgrid, pblock, 0, stream, g);
            MXS_TRY(hipGetLastError());
            g.var_list = rh.pk.rest.p;
            g.n_list = rh.pk.n_rest;
        }
        if (g.n_list > 0) {
            g.bpr = blocks_of(g.n_list, TPB);
            const dim3 grid((unsigned)(g.bpr * n_rep)), block(TPB);
            if (generic || rh.max_dom > 32) hipLaunchKernelGGL((k_dsa_cycle<T, REP>), grid, block, 0, stream, g);
            else if (rh.max_dom <= 4) hipLaunchKernelGGL((k_dsa_cycle_slots<T, 4, REP>), grid, block, 0, stream, g);
            else if (rh.max_dom <= 8) hipLaunchKernelGGL((k_dsa_cycle_slots<T, 8, REP>), grid, block, 0, stream, g);
            else if (rh.max_dom <= 16) hipLaunchKernelGGL((k_dsa_cycle_slots<T, 16, REP>), grid, block, 0, stream, g);
            else hipLaunchKernelGGL((k_dsa_cycle_slots<T, 32, REP>), grid, block, 0, stream, g);
            MXS_TRY(hipGetLastError());
        }
        return MXS_OK;
    }

    int run(int32_t n) override {
        MXS_TRY(hipSetDevice(rh.device));
        const int nV = g.n_vars;
        const rephost::KernelChoice k = rephost::kernel_choice(g.pack.n_lanes > 0);
        for (int32_t c = 0; c < n; ++c) {
            g.cur = cur[which].p;
            g.cur_out = cur[which ^ 1].p;
            g.cycle = cycles;
            g.var_list = nullptr;
            g.n_list = nV;
            if (int rc = n_rep == 1 ? launch_cycle<false>(k.packed, k.generic) : launch_cycle<true>(k.packed, k.generic)) return rc;
            which ^= 1;
            cycles += 1;
            if (int rc = bt.after_step(rh, g, cur[which].p, cycles)) return rc;
        }
        MXS_TRY(hipStreamSynchronize(rh.stream));
        return MXS_OK;
    }

    int get_state(int32_t r, int32_t* idx, double* cst) override {
        if (r < 0 || r >= n_rep) return fail(MXS_E_INVALID, "replica out of range");
        MXS_TRY(hipSetDevice(rh.device));
        const int nV = g.n_vars;
        if (!nV) return MXS_OK;
        std::vector<T> hc(nV);
        std::vector<int32_t> hi(nV);
        const size_t roff = (size_t)r * nV;
        MXS_TRY(hipMemcpyAsync(hi.data(), cur[which].p + roff, 4 * (size_t)nV, hipMemcpyDeviceToHost, rh.stream));
        MXS_TRY(hipMemcpyAsync(hc.data(), cost.p + roff, sizeof(T) * (size_t)nV, hipMemcpyDeviceToHost, rh.stream));
        MXS_TRY(hipStreamSynchronize(rh.stream));
        if (idx) rh.unpack(hi, idx);
        for (int v = 0; v < nV; ++v)
            if (cst) cst[v] = (double)hc[rh.h_q[v]];
        return MXS_OK;
    }

    int eval_cost(const int32_t* idx, double infinity, double* cst, int64_t* viol) override {
        return rh.eval_cost(idx, infinity, cst, viol, [&](int32_t* out) { return get_state(0, out, nullptr); });
    }

    int replica_costs(double infinity, double* cst, int64_t* viol) override {
        return rh.replica_costs(g, cur[which].p, infinity, cst, viol);
    }

    int track_best(int32_t ev, double infinity) override {
        return bt.track(rh, g, cur[which].p, cycles, ev, infinity);
    }

    int get_best(int32_t r, int32_t* replica, int64_t* cycle, double* cst, int64_t* viol, int32_t* idx) override {
        return bt.get(rh, g, cur[which].p, cycles, r, replica, cycle, cst, viol, idx,
                      [&](int32_t rep, int32_t* out) { return get_state(rep, out, nullptr); }, "mxs_dsa");
    }
};

}  // namespace dsa

struct mxs_dsa {
    dsa::Base* impl;
};

extern "C" {

int mxs_dsa_create(const mxs_graph* g, const mxs_params* p, int32_t variant, double probability, int32_t arity_mode,
                   uint64_t seed, int32_t device, mxs_dsa** out) {
    return mxs_dsa_create_replicas(g, p, variant, probability, arity_mode, &seed, 1, device, out);
}
int mxs_dsa_create_replicas(const mxs_graph* g, const mxs_params* p, int32_t variant, double probability,
                            int32_t arity_mode, const uint64_t* seeds, int32_t n_replicas, int32_t device, mxs_dsa** out) {
    return mxs_host::create<mxs_dsa, dsa::Engine>(g, p, out, variant, probability, arity_mode, seeds, n_replicas, device);
}
int mxs_dsa_replicas(const mxs_dsa* e, int32_t* n) {
    if (!e) return mxs_host::fail(MXS_E_INVALID, "null handle");
    if (n) *n = e->impl->n_rep;
    return MXS_OK;
}
int mxs_dsa_reset(mxs_dsa* e) { return e ? e->impl->reset() : mxs_host::fail(MXS_E_INVALID, "null handle"); }
int mxs_dsa_set_value_rank(mxs_dsa* e, const int32_t* value_rank) {
    return e ? e->impl->set_value_rank(value_rank) : mxs_host::fail(MXS_E_INVALID, "null handle");
}
int mxs_dsa_run(mxs_dsa* e, int32_t n_cycles) {
    if (!e) return mxs_host::fail(MXS_E_INVALID, "null handle");
    if (n_cycles < 0) return mxs_host::fail(MXS_E_INVALID, "negative cycle count");
    return e->impl->run(n_cycles);
}
int mxs_dsa_cycles(const mxs_dsa* e, int64_t* cycles) {
    if (!e) return mxs_host::fail(MXS_E_INVALID, "null handle");
    if (cycles) *cycles = e->impl->cycles;
    return MXS_OK;
}
int mxs_dsa_get_state(mxs_dsa* e, int32_t* idx, double* cost) {
    return e ? e->impl->get_state(0, idx, cost) : mxs_host::fail(MXS_E_INVALID, "null handle");
}
int mxs_dsa_get_state_replica(mxs_dsa* e, int32_t r, int32_t* idx, double* cost) {
    return e ? e->impl->get_state(r, idx, cost) : mxs_host::fail(MXS_E_INVALID, "null handle");
}
int mxs_dsa_eval_cost(mxs_dsa* e, const int32_t* idx, double infinity, double* cost, int64_t* violations) {
    return e ? e->impl->eval_cost(idx, infinity, cost, violations) : mxs_host::fail(MXS_E_INVALID, "null handle");
}
int mxs_dsa_replica_costs(mxs_dsa* e, double infinity, double* cost, int64_t* violations) {
    return e ? e->impl->replica_costs(infinity, cost, violations) : mxs_host::fail(MXS_E_INVALID, "null handle");
}
int mxs_dsa_track_best(mxs_dsa* e, int32_t every, double infinity) {
    return e ? e->impl->track_best(every, infinity) : mxs_host::fail(MXS_E_INVALID, "null handle");
}
int mxs_dsa_get_best(mxs_dsa* e, int32_t r, int32_t* replica, int64_t* cycle, double* cost, int64_t* violations,
                     int32_t* idx) {
    return e ? e->impl->get_best(r, replica, cycle, cost, violations, idx) : mxs_host::fail(MXS_E_INVALID, "null handle");
}
int mxs_dsa_destroy(mxs_dsa* e) {
    if (e) {
        delete e->impl;
        delete e;
    }
    return MXS_OK;
}

}  // extern "C"
