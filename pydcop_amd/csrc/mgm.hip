// mgm.hip -- the reference's MGM (pydcop/algorithms/mgm.py: Maheswaran, Pearce, Tambe 2004) on
// gfx950, on the same flat factor-graph arrays as the Max-Sum engine (SURVEY.md section 8(f).4:
// "per-variable segmented argmin over neighbour values -- same layout, different semiring").
//
// MGM is bulk-synchronous by construction (a computation handles a round's values only when ALL
// its neighbours' values are in, then the gains; early messages are parked, mgm.py:311-333,
// 476-497): one round = two launches over all variables,
//   k_mgm_gain   values in  -> the best unilateral move and its gain   (mgm.py:335-391, 428-454)
//   k_mgm_move   gains in   -> the largest gain of a neighbourhood moves, ties by name (:499-588)
// Three families of the two kernels, bit-identical results: the PACKED view (local_search.h: one lane
// per (variable, constraint) for unary / binary constraints over domains of at most four values -- what
// runs by default where the instance allows it), the slot view (thread per variable, register arrays
// for domains up to 32 values) for the other variables, and the CSR walk (anything).  The dynamic
// state lives in packed order (Dev::q); a variable's gain, new value and name rank are one 16-byte
// record (GainRec), its own cost at the current value is kept (Dev::vcc).  The reference's quirks
// are restated as they are and listed in oracle/mgm_oracle.c, whose arithmetic this file follows
// expression for expression (the oracle is pinned against the reference's own MgmComputation).
// The reference's draws from the unseeded `random` module are fixed the way the oracle fixes them:
// first domain value at start, first of equally good values (mxs_mgm_create).
//
// KEYED DRAWS (mxs_mgm_create_keyed): the two draws come from the counter-based generator of engine_common.h,
// u = uniform(seeds[r], v, cycle, draw) with v the GRAPH index of the variable (never its packed position):
//   draw 10  start value of a variable with neighbours and no initial value: int(u * D), cycle 0    (mgm.py:301)
//   draw 11  one of the best values, when the gain strictly improves: B[int(u * |B|)], B = the values whose
//            utilities_at equals the optimum exactly (in T), in domain order (find_arg_optimal)      (mgm.py:379)
// The cycle of draw 11 is the computation's cycle_count when it handles the round's values: the counter starts
// at 1 and new_cycle() runs after the decision, so engine round k (1-based) is cycle k = rounds + 1 (Dev::round;
// pinned against the reference's own MgmComputation by tests/test_mgm_keyed_oracle_vs_reference.py).  The
// random.random() of _send_gain (mgm.py:407) has no effect and gets no draw.
//
// REPLICAS: a keyed engine advances R seeded runs with the same launches, as dsa.hip does.  Everything static is
// stored once; the dynamic state -- cur[2], cost[2], has_cost, grec, vcc[2] -- is [R][n_vars] in packed order, the
// seeds are a device array.  The replica is folded into blockIdx.x (block = replica * bpr + b, replica_cost.h):
// whole blocks belong to one replica, which shifts the state pointers of its copy of Dev once (enter_replica).
// Replica r is bit for bit the keyed single run with seeds[r].  The kernels are templates <REP, KEYED>: the
// fixed-draw engine runs <false, false> on the plain Dev -- the parent's argument layout and instructions --,
// a keyed engine <R > 1, true> on DevR.  MGM's own sum never rises, so its final state is its best: no best-state
// tracking, the final states are ranked (replica_cost.h: the reduction shared with dsa.hip).  The host side that does
// not depend on the algorithm -- set-up, views, uploads, start values, the cost launches -- is rephost::Host
// (replica_host.h, shared with dsa.hip); this file keeps the kernels, the Dev structs, the per-lane extras and the
// round's launches.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/maxsum_gpu.h"
#include "engine_common.h"
#include "local_search.h"
#include "replica_cost.h"
#include "replica_host.h"

namespace mgm {

using mxs_host::Buf;
using mxs_host::fail;
using mxs_host::uniform;   // draws 10 (start value) and 11 (one of the best values)
using repcost::replica_of_block;

constexpr int D_START = 10, D_BEST = 11;

constexpr int TPB = 64;  // one wave per block: 100k variables spread over every CU (latency-bound CSR walks)

template <typename T>
struct alignas(16) GainRec {
    T gain;
    int32_t newv, rank;  // rank: written once at init
};

template <typename T>
struct Dev {
    int32_t n_vars, is_max;
    const int32_t *dom_size, *factor_rowptr, *edge_var, *edge_factor, *var_rowptr, *var_edges, *init_idx, *name_rank, *n_neigh;
    const int64_t *table_off, *cost_off;
    const T *tables, *var_cost;
    const int32_t* cur;    // values of the round being handled
    const T* cost;
    int32_t* cur_out;      // k_mgm_move: after the round
    T* cost_out;
    uint8_t* has_cost;
    GainRec<T>* grec;      // [n_vars] gain, new value and name rank of a variable in ONE 16-byte record: what a
                           // neighbour's move reads of it is one random request instead of three
    const T* vcc;          // [n_vars] var_cost at the variable's value in `cur` (kept by the move kernels):
    T* vcc_out;            // the concerned-variable sums read one word instead of cost_off -> cur -> var_cost
    const T* vc4;          // [n_vars][PACK_D] var_cost of the packed variables, addressed by the variable alone
    lsearch::Slots slots;
    lsearch::Pack pack;          // the packed view (local_search.h): lane per (variable, constraint)
    const int32_t* pack_conc;    // [lanes] element k of the variable's concerned-variables list, -1 = none
    const int32_t* pack_conc_x;  // [lanes] lane k = 0: element `deg` of that list (it has at most deg + 1), else -1
    const int32_t* var_list;     // the variables a thread-per-variable launch works on (NULL: all)
    int32_t n_list;
    // The DYNAMIC per-variable state -- cur, cost, has_cost, grec, vcc -- is stored in PACKED ORDER:
    // position q[v] = the variable's rank in the packed view's wave order (the other variables after them).
    // A packed wave's variables are then q = first .. first + nv - 1: what lane k = 0 of each of them
    // reads and writes of its own state is one line per array instead of one line per variable
    // (scattered 8-byte stores of ~8 lanes per wave cost 0.9 us per store instruction at 100k variables,
    // profiles/r03_local_search_kernels_v2.txt).  The packed view holds q directly (nb, conc, vars); the
    // thread-per-variable kernels translate graph indices through q[].  Everything the semantics depends
    // on -- sum orders, name ranks, the concerned lists' ascending order -- stays on graph indices.
    const int32_t* q;
    const int32_t* pack_dom;     // [packed variables] dom_size in packed order
};

// what a keyed engine's kernels take: Dev plus the replicas and the keys of the draws.  The fixed-draw kernels
// keep the plain Dev, i.e. their argument layout.  The per-replica arrays of Dev -- cur, cost, cur_out, cost_out,
// has_cost, grec, vcc, vcc_out -- are [replicas][n_vars]: replica r at + r * n_vars (64-bit).
template <typename T>
struct DevR : Dev<T> {
    int32_t bpr;               // blocks per replica of the launch being made (block = replica * bpr + b)
    int32_t n_rep;
    const uint64_t* seeds;     // [replicas]
    int64_t round;             // the cycle_count of the round being handled: rounds + 1 (the key of draw 11)
    const int32_t* pack_var;   // [packed variables] graph index of the packed position (the key of draw 11)
};
template <typename T, bool REP, bool KEYED>
using DevOf = typename std::conditional<REP || KEYED, DevR<T>, Dev<T>>::type;

// the replica of this block; REP: the block's copy of Dev (kernel arguments, block-uniform) moves to the
// replica's slice of the dynamic state, so that nothing below knows about replicas
template <bool REP, typename G, typename T>
__device__ inline int enter_replica(G& g, T*& cost_rw, int* b) {
    const int r = replica_of_block<REP>(g, b);
    if constexpr (REP) {
        const int64_t off = (int64_t)r * g.n_vars;
        g.cur += off, g.cost += off, g.cur_out += off, g.cost_out += off;
        g.has_cost += off, g.grec += off, g.vcc += off, g.vcc_out += off;
        if (cost_rw) cost_rw += off;
    }
    return r;
}
// improving: the gain is strictly better than nothing (mgm.py:376-378)
template <typename T>
__device__ inline bool improves(int is_max, T gain) {
    return (!is_max && gain > (T)0) || (is_max && gain < (T)0);
}

// c.slice(neighbours' values)(x): the table entry with v at x, every other scope variable at its value
template <typename T>
__device__ T constraint_at(const Dev<T>& g, int f, int v, int x) {
    int64_t lin = 0;
    for (int e = g.factor_rowptr[f]; e < g.factor_rowptr[f + 1]; ++e) {
        const int u = g.edge_var[e];
        lin = lin * g.dom_size[u] + (u == v ? x : g.cur[g.q[u]]);
    }
    return g.tables[g.table_off[f] + lin];
}

// functools.reduce(operator.add, [f(x) for f in reduced_cs]): utilities order, no initial 0
template <typename T>
__device__ T utilities_at(const Dev<T>& g, int v, int x) {
    T acc = (T)0;
    bool first = true;
    for (int k = g.var_rowptr[v]; k < g.var_rowptr[v + 1]; ++k) {
        const T f = constraint_at(g, g.edge_factor[g.var_edges[k]], v, x);
        acc = first ? f : acc + f;
        first = false;
    }
    return acc;
}

// acc += cost_for_val of every distinct variable of v's constraints (v included) at its current
// value, in ascending variable index (the reference iterates a set, see oracle/mgm_oracle.c)
template <typename T>
__device__ T add_concerned_costs(const Dev<T>& g, int v, T acc) {
    int last = -1;
    for (;;) {
        int best = INT32_MAX;
        for (int k = g.var_rowptr[v]; k < g.var_rowptr[v + 1]; ++k) {
            const int f = g.edge_factor[g.var_edges[k]];
            for (int e = g.factor_rowptr[f]; e < g.factor_rowptr[f + 1]; ++e) {
                const int u = g.edge_var[e];
                if (u > last && u < best) best = u;
            }
        }
        if (best == INT32_MAX) break;
        acc += g.vcc[g.q[best]];  // = var_cost[cost_off[best] + cur[best]], kept by the move kernels
        last = best;
    }
    return acc;
}

template <typename T, bool REP, bool KEYED>
__global__ void __launch_bounds__(TPB) k_mgm_gain(DevOf<T, REP, KEYED> g, T* cost_rw) {
    int b;
    [[maybe_unused]] const int r = enter_replica<REP>(g, cost_rw, &b);
    const int tid = REP ? b * (int)blockDim.x + (int)threadIdx.x : (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (tid >= g.n_list) return;
    const int v = g.var_list ? g.var_list[tid] : tid;
    if (g.n_neigh[v] == 0) return;
    const int qv = g.q[v];
    T cost = cost_rw[qv];
    if (!g.has_cost[qv]) {  // first round: the cost of the current value (mgm.py:349-372)
        cost = add_concerned_costs(g, v, utilities_at(g, v, g.cur[qv]));
        cost_rw[qv] = cost;
        g.has_cost[qv] = 1;
    }
    T best = (T)0;
    int best_x = -1;
    [[maybe_unused]] int n_best = 0;  // KEYED: the length of the list
    for (int x = 0; x < g.dom_size[v]; ++x) {  // find_arg_optimal: strictly better starts a new list
        const T u = utilities_at(g, v, x);
        if (best_x < 0 || (g.is_max ? best < u : best > u)) {
            best = u;
            best_x = x;
            if constexpr (KEYED) n_best = 1;
        } else if constexpr (KEYED) {
            if (u == best) n_best += 1;    // equal joins it
        }
    }
    const T val_cost = add_concerned_costs(g, v, best);  // own cost at the CURRENT value (:449-450)
    const T gain = cost - val_cost;
    if constexpr (KEYED) {  // random.choice(new_values): the j-th of the list, a second pass over the domain
        if (improves(g.is_max, gain) && n_best > 1) {
            int j = (int)(uniform(g.seeds[r], v, g.round, D_BEST) * n_best);
            for (int x = 0; x < g.dom_size[v]; ++x) {
                if (utilities_at(g, v, x) != best) continue;
                if (j-- == 0) {
                    best_x = x;
                    break;
                }
            }
        }
    }
    const int nvl = ((!g.is_max && gain > (T)0) || (g.is_max && gain < (T)0)) ? best_x : g.cur[qv];
    g.grec[qv].gain = gain;
    g.grec[qv].newv = nvl;
}

template <typename T, bool REP>
__global__ void __launch_bounds__(TPB) k_mgm_move(DevOf<T, REP, false> g) {
    int b;
    T* none = nullptr;
    enter_replica<REP>(g, none, &b);
    const int tid = REP ? b * (int)blockDim.x + (int)threadIdx.x : (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (tid >= g.n_list) return;
    const int v = g.var_list ? g.var_list[tid] : tid;
    const int qv = g.q[v];
    int cur = g.cur[qv];
    T cost = g.cost[qv];
    if (g.n_neigh[v] != 0) {
        T max_n = (T)0;
        bool first = true;
        for (int k = g.var_rowptr[v]; k < g.var_rowptr[v + 1]; ++k) {
            const int f = g.edge_factor[g.var_edges[k]];
            for (int e = g.factor_rowptr[f]; e < g.factor_rowptr[f + 1]; ++e) {
                const int u = g.edge_var[e];
                if (u == v) continue;
                const T gu = g.grec[g.q[u]].gain;
                if (first || gu > max_n) max_n = gu;  // max() also in max mode (:513)
                first = false;
            }
        }
        bool wins_tie = true;
        for (int k = g.var_rowptr[v]; k < g.var_rowptr[v + 1]; ++k) {
            const int f = g.edge_factor[g.var_edges[k]];
            for (int e = g.factor_rowptr[f]; e < g.factor_rowptr[f + 1]; ++e) {
                const int u = g.edge_var[e];
                if (u != v && g.grec[g.q[u]].gain == max_n && g.name_rank[u] < g.name_rank[v]) wins_tie = false;
            }
        }
        const T gain = g.grec[qv].gain;
        if (gain > max_n || (gain == max_n && wins_tie)) {  // :514-525, lexic ties :566-588
            cur = g.grec[qv].newv;
            cost = cost - gain;
        }
    }
    g.cur_out[qv] = cur;
    g.cost_out[qv] = cost;
    g.vcc_out[qv] = g.var_cost[g.cost_off[v] + cur];
}

// ---- the same two kernels on the slot view (local_search.h) ---------------------------------
// the costs of the D values in registers from one pass over the variable's constraints; the
// distinct variables of those constraints from a list sorted on the host instead of the
// repeated minimum search of add_concerned_costs; domains of at most MAXD values
// (the variable references of the slot view -- nb0_var, nb_var, conc_var -- are uploaded as packed
// positions q: they index the dynamic state directly)
template <typename T>
__device__ T add_concerned_costs_listed(const Dev<T>& g, int v, T acc) {
    for (int k = g.slots.conc_rowptr[v]; k < g.slots.conc_rowptr[v + 1]; ++k)
        acc += g.vcc[g.slots.conc_var[k]];  // = var_cost[cost_off[u] + cur[u]], kept by the move kernels
    return acc;
}

template <typename T, int MAXD, bool REP, bool KEYED>
__global__ void __launch_bounds__(TPB) k_mgm_gain_slots(DevOf<T, REP, KEYED> g, T* cost_rw) {
    int b;
    [[maybe_unused]] const int r = enter_replica<REP>(g, cost_rw, &b);
    const int tid = REP ? b * (int)blockDim.x + (int)threadIdx.x : (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (tid >= g.n_list) return;
    const int v = g.var_list ? g.var_list[tid] : tid;
    if (g.n_neigh[v] == 0) return;
    const int D = g.dom_size[v];
    T c[MAXD];
    {
        const int s0 = g.var_rowptr[v], s1 = g.var_rowptr[v + 1];
        if (g.slots.rows != nullptr && s0 < s1 && g.slots.row_base[s0] >= 0) {  // contiguous rows (local_search.h)
            if (g.slots.rows_int8) lsearch::costs_of_values_rows<T, int8_t, MAXD>(g.slots, g.cur, s0, s1, D, false, c);
            else lsearch::costs_of_values_rows<T, T, MAXD>(g.slots, g.cur, s0, s1, D, false, c);
        } else {
            lsearch::costs_of_values<T, MAXD>(g.slots, g.tables, g.cur, s0, s1, D, false, c);
        }
    }
    const int qv = g.q[v];
    T cost = cost_rw[qv];
    if (!g.has_cost[qv]) {
        cost = add_concerned_costs_listed(g, v, lsearch::pick<T, MAXD>(c, g.cur[qv]));
        cost_rw[qv] = cost;
        g.has_cost[qv] = 1;
    }
    T best = c[0];
    int best_x = 0;
#pragma unroll
    for (int x = 1; x < MAXD; ++x)
        if (x < D && (g.is_max ? best < c[x] : best > c[x])) {
            best = c[x];
            best_x = x;
        }
    const T val_cost = add_concerned_costs_listed(g, v, best);
    const T gain = cost - val_cost;
    if constexpr (KEYED) {  // random.choice(new_values): the values equal to the optimum, the j-th in domain order
        if (improves(g.is_max, gain)) {
            int n_best = 0;
#pragma unroll
            for (int x = 0; x < MAXD; ++x) n_best += (x < D && c[x] == best) ? 1 : 0;
            if (n_best > 1) {
                int j = (int)(uniform(g.seeds[r], v, g.round, D_BEST) * n_best);
                bool done = false;
#pragma unroll
                for (int x = 0; x < MAXD; ++x)
                    if (x < D && !done && c[x] == best) {
                        if (j-- == 0) {
                            best_x = x;
                            done = true;
                        }
                    }
            }
        }
    }
    const int nvl = ((!g.is_max && gain > (T)0) || (g.is_max && gain < (T)0)) ? best_x : g.cur[qv];
    g.grec[qv].gain = gain;
    g.grec[qv].newv = nvl;
}

template <typename T, bool REP>
__global__ void __launch_bounds__(TPB) k_mgm_move_listed(DevOf<T, REP, false> g) {
    int b;
    T* none = nullptr;
    enter_replica<REP>(g, none, &b);
    const int tid = REP ? b * (int)blockDim.x + (int)threadIdx.x : (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (tid >= g.n_list) return;
    const int v = g.var_list ? g.var_list[tid] : tid;
    const int qv = g.q[v];
    int cur = g.cur[qv];
    T cost = g.cost[qv];
    if (g.n_neigh[v] != 0) {
        const int k0 = g.slots.conc_rowptr[v], k1 = g.slots.conc_rowptr[v + 1];
        const GainRec<T> me = g.grec[qv];
        T max_n = (T)0;
        bool first = true, wins_tie = true;
        for (int k = k0; k < k1; ++k) {  // one pass: the largest gain and whether a lower name holds it
            const int uq = g.slots.conc_var[k];
            if (uq == qv) continue;
            const GainRec<T> r = g.grec[uq];
            const bool lower = r.rank < me.rank;
            if (first || r.gain > max_n) {
                max_n = r.gain;
                wins_tie = !lower;
            } else if (r.gain == max_n && lower) {
                wins_tie = false;
            }
            first = false;
        }
        if (me.gain > max_n || (me.gain == max_n && wins_tie)) {
            cur = me.newv;
            cost = cost - me.gain;
        }
    }
    g.cur_out[qv] = cur;
    g.cost_out[qv] = cost;
    g.vcc_out[qv] = g.var_cost[g.cost_off[v] + cur];
}

// ---- the same two kernels on the PACKED view (local_search.h): one lane per (variable, constraint) ----
// What a lane holds of its variable's concerned-variables list (ascending, the variable included; at most
// deg + 1 entries): element k, and on lane k = 0 also element deg.
constexpr int PACK_TPB = 256;
struct PackLane {
    int deg, nv, var, k, seg, q;  // q: the variable's packed position = its index into the dynamic state
    bool has;
};
template <typename T>
__device__ inline PackLane pack_lane(const Dev<T>& g, int64_t pos) {
    const lsearch::PackWave wm = g.pack.waves[__builtin_amdgcn_readfirstlane((int)(pos >> 6))];
    const uint32_t dn = (uint32_t)wm.deg_nv;
    PackLane p;
    p.deg = (int)(dn & 255u);
    p.nv = (int)((dn >> 8) & 255u);
    const int l = (int)threadIdx.x & 63;
    p.var = (int)(((uint32_t)l * (dn >> 16)) >> 15);
    p.k = l - p.var * p.deg;
    p.has = p.var < p.nv;
    p.seg = l - p.k;
    p.q = wm.first + (p.has ? p.var : 0);
    return p;
}

// acc + cost_for_val of every concerned variable at its current value, in list order: each lane
// fetches ITS element (the fetches of a variable's lanes are in flight together), the additions
// then run in order through cross-lane reads -- every lane of the variable ends with the same sum
template <typename T>
__device__ inline T pack_add_concerned(const Dev<T>& g, const PackLane& p, int64_t pos, T acc) {
    const int u = g.pack_conc[pos], ux = g.pack_conc_x[pos];
    T w = (T)0, wx = (T)0;
    if (u >= 0) w = g.vcc[u];
    if (ux >= 0) wx = g.vcc[ux];
    // which lanes hold an element: one ballot each instead of a lane exchange per step
    const unsigned long long live = __ballot(u >= 0 ? 1 : 0), live_x = __ballot(ux >= 0 ? 1 : 0);
    for (int i = 0; i < p.deg; ++i) {
        const T e = __shfl(w, p.seg + i, 64);
        acc = ((live >> (p.seg + i)) & 1ull) ? acc + e : acc;
    }
    const T ex = __shfl(wx, p.seg, 64);
    acc = ((live_x >> p.seg) & 1ull) ? acc + ex : acc;
    return acc;
}

template <typename T, typename TT, bool REP, bool KEYED>
__global__ void __launch_bounds__(PACK_TPB) k_mgm_gain_pack(DevOf<T, REP, KEYED> g, T* cost_rw) {
    constexpr int MAXD = lsearch::PACK_D;
    int b;
    [[maybe_unused]] const int r = enter_replica<REP>(g, cost_rw, &b);
    const int64_t pos = (int64_t)(REP ? (unsigned)b : blockIdx.x) * blockDim.x + threadIdx.x;
    if (pos >= g.pack.n_lanes) return;  // whole waves
    const PackLane p = pack_lane(g, pos);
    const int v = p.q, D = g.pack_dom[v], mine = g.cur[v];  // (v: packed position; nb / conc hold positions too)
    T t[MAXD], c[MAXD];
    lsearch::pack_costs<T, TT>(g.pack, g.cur, pos, p.deg, p.seg, false, t, c);
    T cost = cost_rw[v];
    const bool first_round = !g.has_cost[v];
    // (wave-uniform in practice: every variable gets its cost in the first round)
    if (__ballot(first_round ? 1 : 0) != 0ull) {
        const T c0 = pack_add_concerned(g, p, pos, lsearch::pick<T, MAXD>(c, mine));
        if (first_round) cost = c0;
    }
    T best = c[0];
    int best_x = 0;
#pragma unroll
    for (int x = 1; x < MAXD; ++x) {
        const bool lt = best < c[x], gt = best > c[x];
        const bool better = (x < D) & (g.is_max ? lt : gt);
        best = better ? c[x] : best;
        best_x = better ? x : best_x;
    }
    const T val_cost = pack_add_concerned(g, p, pos, best);  // own cost at the CURRENT value (mgm.py:449-450)
    const T gain = cost - val_cost;
    if constexpr (KEYED) {  // random.choice(new_values): every lane of the variable takes the same pick
        if (improves(g.is_max, gain)) {
            int n_best = 0;
#pragma unroll
            for (int x = 0; x < MAXD; ++x) n_best += (x < D && c[x] == best) ? 1 : 0;
            if (n_best > 1) {
                int j = (int)(uniform(g.seeds[r], g.pack_var[v], g.round, D_BEST) * n_best);
                bool done = false;
#pragma unroll
                for (int x = 0; x < MAXD; ++x)
                    if (x < D && !done && c[x] == best) {
                        if (j-- == 0) {
                            best_x = x;
                            done = true;
                        }
                    }
            }
        }
    }
    if (p.has && p.k == 0) {
        if (first_round) {
            cost_rw[v] = cost;
            g.has_cost[v] = 1;
        }
        const int nvl = ((!g.is_max && gain > (T)0) || (g.is_max && gain < (T)0)) ? best_x : mine;
        g.grec[v].gain = gain;
        g.grec[v].newv = nvl;
    }
}

template <typename T, bool REP>
__global__ void __launch_bounds__(PACK_TPB) k_mgm_move_pack(DevOf<T, REP, false> g) {
    int b;
    T* none = nullptr;
    enter_replica<REP>(g, none, &b);
    const int64_t pos = (int64_t)(REP ? (unsigned)b : blockIdx.x) * blockDim.x + threadIdx.x;
    if (pos >= g.pack.n_lanes) return;
    const PackLane p = pack_lane(g, pos);
    const int v = p.q;  // packed position (conc / conc_x hold positions too)
    // The largest gain among the OTHER concerned variables and whether a lower name holds it (max() also in
    // max mode, mgm.py:513; lexic ties :566-588).  Order-independent -- the reference's scan keeps (largest so
    // far, "no lower name holds it") -- so the lanes of a variable reduce their elements pairwise in
    // ceil(log2(deg)) steps instead of every lane scanning all of them; lane k = 0 ends with the result.
    const int u = g.pack_conc[pos], ux = g.pack_conc_x[pos];
    const GainRec<T> me = g.grec[v];
    const int cur0 = g.cur[v];
    const T cost0 = g.cost[v];
    const T vc0 = g.vcc[v];
    // the own costs of the variable's values in packed order (through cost_off[] + the new value they
    // would be one dependent load later); the new value's is picked in registers
    T vc[lsearch::PACK_D];
#pragma unroll
    for (int x = 0; x < lsearch::PACK_D; ++x) vc[x] = g.vc4[(int64_t)v * lsearch::PACK_D + x];
    T e = (T)0, ex = (T)0;
    unsigned fl = 0u, fx = 0u;  // bit 0: an element (a concerned variable other than v), bit 1: a lower name holds it
    if (u >= 0 && u != v) {
        const GainRec<T> r = g.grec[u];
        e = r.gain;
        fl = 1u | (r.rank < me.rank ? 2u : 0u);
    }
    if (ux >= 0 && ux != v) {
        const GainRec<T> r = g.grec[ux];
        ex = r.gain;
        fx = 1u | (r.rank < me.rank ? 2u : 0u);
    }
    auto merge = [&](T e2, unsigned f2) {  // (e, fl) <- the larger of the two; equal gains: either's lower name counts
        const bool la = (fl & 1u) != 0u, lb = (f2 & 1u) != 0u;
        const bool b_wins = lb & (!la | (e2 > e));
        const bool tie = la & lb & (e2 == e);
        fl = b_wins ? f2 : (tie ? fl | (f2 & 2u) : fl);
        e = b_wins ? e2 : e;
    };
    const int l = (int)threadIdx.x & 63;
    for (int s = 1; s < p.deg; s <<= 1) {
        const T e2 = __shfl(e, (l + s) & 63, 64);
        const unsigned f2 = (unsigned)__shfl((int)fl, (l + s) & 63, 64);
        merge(e2, p.k + s < p.deg ? f2 : 0u);
    }
    merge(ex, fx);  // element deg of the list: lane k = 0 holds it
    if (p.has && p.k == 0) {
        const bool any = (fl & 1u) != 0u;
        const T max_n = any ? e : (T)0;
        const bool wins_tie = !any || (fl & 2u) == 0u;
        const bool moves = me.gain > max_n || (me.gain == max_n && wins_tie);  // :514-525
        g.cur_out[v] = moves ? me.newv : cur0;
        g.cost_out[v] = moves ? cost0 - me.gain : cost0;
        g.vcc_out[v] = moves ? lsearch::pick<T, lsearch::PACK_D>(vc, me.newv) : vc0;
    }
}

// the start state of every replica (on_start, mgm.py:279-305): a variable without neighbours takes its
// optimal_cost_value (iso_val >= 0, the same in every replica) and holds its cost; the others their initial value,
// else draw 10 of cycle 0 under seeds[r] (keyed) or the first value of the domain (fixed).  Both buffers of cur /
// cost / vcc: the packed launches write only the variables that have neighbours.
constexpr int AUX_TPB = 256;
template <typename T>
__global__ void __launch_bounds__(AUX_TPB) k_mgm_init(DevR<T> g, int keyed, const int32_t* iso_val, const T* iso_cost,
                                                      const int32_t* init, int32_t* cur0, int32_t* cur1, T* cost0, T* cost1,
                                                      T* vcc0, T* vcc1) {
    int b;
    const int r = replica_of_block<true>(g, &b);
    const int v = b * (int)blockDim.x + (int)threadIdx.x;
    if (v >= g.n_vars) return;
    const int64_t at = (int64_t)r * g.n_vars + g.q[v];
    const int iso = iso_val[v];
    int x = 0;
    if (iso >= 0) x = iso;
    else if (init[v] >= 0) x = init[v];
    else if (keyed) x = (int32_t)(uniform(g.seeds[r], v, 0, D_START) * g.dom_size[v]);
    const T held = iso >= 0 ? iso_cost[v] : (T)0;
    const T own = g.var_cost[g.cost_off[v] + x];
    cur0[at] = x, cur1[at] = x;
    cost0[at] = held, cost1[at] = held;
    vcc0[at] = own, vcc1[at] = own;
    g.has_cost[at] = iso >= 0 ? 1 : 0;
    g.grec[at] = GainRec<T>{(T)0, x, g.name_rank[v]};  // no gain yet, the "new value" is the initial one
}

struct Base {
    virtual ~Base() {}
    virtual int init(const mxs_graph& G, const mxs_params& p, const int32_t* rank, bool keyed, const uint64_t* seeds,
                     int n_replicas, int device) = 0;
    virtual int reset() = 0;
    virtual int set_value_rank(const int32_t* rank) = 0;
    virtual int run(int32_t n) = 0;
    virtual int get_state(int32_t r, int32_t* idx, double* cost, uint8_t* has, double* gain, int32_t* newv) = 0;
    virtual int eval_cost(const int32_t* idx, double infinity, double* cost, int64_t* viol) = 0;
    virtual int replica_costs(double infinity, double* cost, int64_t* viol) = 0;
    virtual int best_replica(double infinity, int32_t* replica, double* cost, int64_t* viol) = 0;
    int64_t rounds = 0;
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
    DevR<T> g{};
    int which = 0;
    bool keyed = false;
    Buf<int32_t> name_rank, init_idx;
    Buf<int32_t> cur[2];                    // the dynamic state: [R][n_vars], packed order
    Buf<T> var_cost;
    Buf<T> cost[2], vcc[2], vc4;
    Buf<GainRec<T>> grec;
    Buf<uint8_t> has_cost;
    Buf<int32_t> pk_conc, pk_conc_x;  // what only MGM keeps per lane (Dev::pack_conc, pack_conc_x)
    Buf<int32_t> pk_var;              // [packed variables] graph index (DevR::pack_var)

    int init(const mxs_graph& G, const mxs_params& p, const int32_t* rank, bool kd, const uint64_t* sds, int n_replicas,
             int dev) override {
        keyed = kd;
        if (int rc = rh.open(sds, n_replicas, dev, keyed)) return rc;
        n_rep = rh.n_rep;
        if (int rc = rh.hg.load(G, p)) return rc;
        if (int rc = rh.hg.load_init(G)) return rc;
        const mxs_host::HostGraph& hg = rh.hg;
        const hipStream_t stream = rh.stream;
        const int nV = hg.nV;
        const size_t R = (size_t)n_rep;
        std::vector<int32_t> rk(nV);
        for (int v = 0; v < nV; ++v) rk[v] = rank ? rank[v] : v;
        const std::vector<T> vc = mxs_host::narrowed<T>(hg.var_cost);
        lsearch::HostSlots hs;
        lsearch::HostPack hp;
        if (int rc = rh.build_views(hs, hp)) return rc;
        // MGM's extras: per packed variable its own costs and its graph index, per packed lane its elements of the
        // variable's concerned-variables list
        const std::vector<int32_t>& h_q = rh.h_q;
        std::vector<T> v4(hp.vars.size() * lsearch::PACK_D, (T)0);
        std::vector<int32_t> pvar(hp.vars.size());
        for (int v : hp.vars) {
            pvar[h_q[v]] = v;
            for (int x = 0; x < hg.dom[v]; ++x) v4[(size_t)h_q[v] * lsearch::PACK_D + x] = vc[hg.coff[v] + x];
        }
        std::vector<int32_t> conc(hp.nb.size(), -1), conc_x(hp.nb.size(), -1);
        for (size_t i = 0; i < hp.nb.size(); ++i) {
            const int v = hp.lane_var[i];
            if (v < 0) continue;
            const int c0 = hs.conc_rowptr[v], n_conc = hs.conc_rowptr[v + 1] - c0, k = hp.lane_k[i], deg = hp.lane_deg[i];
            if (n_conc > deg + 1) return fail(MXS_E_STATE, "concerned-variables list longer than the degree + 1");
            if (k < n_conc) conc[i] = hs.conc_var[c0 + k];
            if (k == 0 && n_conc > deg) conc_x[i] = hs.conc_var[c0 + deg];
        }
        MXS_TRY(vc4.upload(v4, stream));
        MXS_TRY(pk_var.upload(pvar, stream));
        MXS_TRY(pk_conc.upload(mxs_host::remap(conc, h_q), stream));
        MXS_TRY(pk_conc_x.upload(mxs_host::remap(conc_x, h_q), stream));
        if (int rc = rh.upload_views(hs, hp)) return rc;
        if (int rc = rh.upload_graph()) return rc;
        MXS_TRY(name_rank.upload(rk, stream));
        MXS_TRY(var_cost.upload(vc, stream));
        MXS_TRY(init_idx.upload(hg.init, stream));
        for (int b = 0; b < 2; ++b) {
            if (int rc = alloc_rep(cur[b], R * nV, "values")) return rc;
            if (int rc = alloc_rep(cost[b], R * nV, "held costs")) return rc;
            if (int rc = alloc_rep(vcc[b], R * nV, "own costs")) return rc;
        }
        if (int rc = alloc_rep(grec, R * nV, "gain records")) return rc;
        if (int rc = alloc_rep(has_cost, R * nV, "cost flags")) return rc;
        rh.bind(g);
        g.n_rep = n_rep;
        g.bpr = 1;
        g.init_idx = nullptr; g.name_rank = name_rank.p;
        g.cost_off = rh.cost_off.p; g.var_cost = var_cost.p;
        g.has_cost = has_cost.p; g.grec = grec.p;
        g.vc4 = vc4.p;
        g.pack_var = pk_var.p;
        g.pack_conc = pk_conc.p;
        g.pack_conc_x = pk_conc_x.p;
        return reset();
    }

    int set_value_rank(const int32_t* rank) override {
        rh.set_value_rank(rank);
        return reset();
    }

    // every replica back to its start state (k_mgm_init): what is uploaded does not grow with the replicas
    int reset() override {
        if (int rc = rh.start_values()) return rc;  // on_start without neighbours: optimal_cost_value (mgm.py:279-290)
        which = 0;
        rounds = 0;
        if (g.n_vars) {
            g.bpr = blocks_of(g.n_vars, AUX_TPB);
            const dim3 grid((unsigned)(g.bpr * n_rep)), block(AUX_TPB);
            hipLaunchKernelGGL((k_mgm_init<T>), grid, block, 0, rh.stream, g, keyed ? 1 : 0, (const int32_t*)rh.iso_val.p,
                               (const T*)rh.iso_cost.p, (const int32_t*)init_idx.p, cur[0].p, cur[1].p, cost[0].p, cost[1].p,
                               vcc[0].p, vcc[1].p);
            MXS_TRY(hipGetLastError());
            MXS_TRY(hipStreamSynchronize(rh.stream));
        }
        return MXS_OK;
    }

    // the four launches of one round (packed plus rest, or thread per variable alone).  <false, false>: the
    // fixed-draw engine, kernels on the plain Dev; REP: all replicas, the replica folded into the grid
    template <bool REP, bool KEYED>
    int launch_round(bool packed, bool generic) {
        const hipStream_t stream = rh.stream;
        const int nV = g.n_vars, max_dom = rh.max_dom;
        T* const cw = cost[which].p;
        g.var_list = packed ? rh.pk.rest.p : nullptr;
        g.n_list = packed ? rh.pk.n_rest : nV;
        const int pbpr = blocks_of(g.pack.n_lanes, PACK_TPB), bpr = blocks_of(g.n_list, TPB);
        const unsigned reps = REP ? (unsigned)n_rep : 1u;
        const dim3 pgrid((unsigned)pbpr * reps), pblock(PACK_TPB);
        const dim3 grid((unsigned)bpr * reps), block(TPB);
        // (a kernel takes its Dev by value: the copy is made at the launch, bpr may change between them)
        DevOf<T, REP, KEYED>& gg = g;       // what the gain kernels take
        DevOf<T, REP, false>& gm = g;       // what the move kernels take
        if (packed) {
            g.bpr = pbpr;
            if (rh.pk.int8) hipLaunchKernelGGL((k_mgm_gain_pack<T, int8_t, REP, KEYED>), pgrid, pblock, 0, stream, gg, cw);
            else hipLaunchKernelGGL((k_mgm_gain_pack<T, T, REP, KEYED>), pgrid, pblock, 0, stream, gg, cw);
            MXS_TRY(hipGetLastError());
        }
        if (g.n_list > 0) {
            g.bpr = bpr;
            if (generic || max_dom > 32) hipLaunchKernelGGL((k_mgm_gain<T, REP, KEYED>), grid, block, 0, stream, gg, cw);
            else if (max_dom <= 4) hipLaunchKernelGGL((k_mgm_gain_slots<T, 4, REP, KEYED>), grid, block, 0, stream, gg, cw);
            else if (max_dom <= 8) hipLaunchKernelGGL((k_mgm_gain_slots<T, 8, REP, KEYED>), grid, block, 0, stream, gg, cw);
            else if (max_dom <= 16) hipLaunchKernelGGL((k_mgm_gain_slots<T, 16, REP, KEYED>), grid, block, 0, stream, gg, cw);
            else hipLaunchKernelGGL((k_mgm_gain_slots<T, 32, REP, KEYED>), grid, block, 0, stream, gg, cw);
            MXS_TRY(hipGetLastError());
        }
        if (packed) {
            g.bpr = pbpr;
            hipLaunchKernelGGL((k_mgm_move_pack<T, REP>), pgrid, pblock, 0, stream, gm);
            MXS_TRY(hipGetLastError());
        }
        if (g.n_list > 0) {
            g.bpr = bpr;
            if (generic) hipLaunchKernelGGL((k_mgm_move<T, REP>), grid, block, 0, stream, gm);
            else hipLaunchKernelGGL((k_mgm_move_listed<T, REP>), grid, block, 0, stream, gm);
            MXS_TRY(hipGetLastError());
        }
        return MXS_OK;
    }

    int run(int32_t n) override {
        MXS_TRY(hipSetDevice(rh.device));
        const int nV = g.n_vars;
        if (nV == 0) {
            rounds += n > 0 ? n : 0;
            return MXS_OK;
        }
        const rephost::KernelChoice k = rephost::kernel_choice(g.pack.n_lanes > 0);
        for (int32_t r = 0; r < n; ++r) {
            g.cur = cur[which].p;
            g.cost = cost[which].p;
            g.cur_out = cur[which ^ 1].p;
            g.cost_out = cost[which ^ 1].p;
            g.vcc = vcc[which].p;
            g.vcc_out = vcc[which ^ 1].p;
            g.round = rounds + 1;  // the reference's cycle_count while it handles this round's values
            int rc;
            if (!keyed) rc = launch_round<false, false>(k.packed, k.generic);
            else if (n_rep == 1) rc = launch_round<false, true>(k.packed, k.generic);
            else rc = launch_round<true, true>(k.packed, k.generic);
            if (rc) return rc;
            which ^= 1;
            rounds += 1;
        }
        MXS_TRY(hipStreamSynchronize(rh.stream));
        return MXS_OK;
    }

    int get_state(int32_t r, int32_t* idx, double* cst, uint8_t* has, double* gn, int32_t* nv) override {
        if (r < 0 || r >= n_rep) return fail(MXS_E_INVALID, "replica out of range");
        MXS_TRY(hipSetDevice(rh.device));
        const hipStream_t stream = rh.stream;
        const int nV = g.n_vars;
        if (!nV) return MXS_OK;
        std::vector<T> hc(nV);
        std::vector<GainRec<T>> hg(nV);
        std::vector<int32_t> hi(nV);
        std::vector<uint8_t> hh(nV);
        const size_t roff = (size_t)r * nV;
        MXS_TRY(hipMemcpyAsync(hi.data(), cur[which].p + roff, 4 * (size_t)nV, hipMemcpyDeviceToHost, stream));
        MXS_TRY(hipMemcpyAsync(hh.data(), has_cost.p + roff, nV, hipMemcpyDeviceToHost, stream));
        MXS_TRY(hipMemcpyAsync(hc.data(), cost[which].p + roff, sizeof(T) * (size_t)nV, hipMemcpyDeviceToHost, stream));
        MXS_TRY(hipMemcpyAsync(hg.data(), grec.p + roff, sizeof(GainRec<T>) * (size_t)nV, hipMemcpyDeviceToHost, stream));
        MXS_TRY(hipStreamSynchronize(stream));
        for (int v = 0; v < nV; ++v) {  // the state lives in packed order (Dev::q)
            const int qv = rh.h_q[v];
            if (idx) idx[v] = hi[qv];
            if (has) has[v] = hh[qv];
            if (cst) cst[v] = (double)hc[qv];
            if (gn) gn[v] = (double)hg[qv].gain;
            if (nv) nv[v] = hg[qv].newv;
        }
        return MXS_OK;
    }

    int eval_cost(const int32_t* idx, double infinity, double* cst, int64_t* viol) override {
        return rh.eval_cost(idx, infinity, cst, viol,
                            [&](int32_t* out) { return get_state(0, out, nullptr, nullptr, nullptr, nullptr); });
    }

    int replica_costs(double infinity, double* cst, int64_t* viol) override {
        return rh.replica_costs(g, cur[which].p, infinity, cst, viol);
    }

    // MGM's own sum never rises: a run's final state is its best, the final states are ranked
    int best_replica(double infinity, int32_t* replica, double* cst, int64_t* viol) override {
        return rh.best_current(g, cur[which].p, infinity, replica, cst, viol);
    }
};

}  // namespace mgm

struct mxs_mgm {
    mgm::Base* impl;
};

extern "C" {

int mxs_mgm_create(const mxs_graph* g, const mxs_params* p, const int32_t* name_rank, int32_t device, mxs_mgm** out) {
    return mxs_host::create<mxs_mgm, mgm::Engine>(g, p, out, name_rank, false, (const uint64_t*)nullptr, 1, device);
}
int mxs_mgm_create_keyed(const mxs_graph* g, const mxs_params* p, const int32_t* name_rank, const uint64_t* seeds,
                         int32_t n_replicas, int32_t device, mxs_mgm** out) {
    return mxs_host::create<mxs_mgm, mgm::Engine>(g, p, out, name_rank, true, seeds, n_replicas, device);
}
int mxs_mgm_replicas(const mxs_mgm* e, int32_t* n) {
    if (!e) return mxs_host::fail(MXS_E_INVALID, "null handle");
    if (n) *n = e->impl->n_rep;
    return MXS_OK;
}
int mxs_mgm_reset(mxs_mgm* e) { return e ? e->impl->reset() : mxs_host::fail(MXS_E_INVALID, "null handle"); }
int mxs_mgm_set_value_rank(mxs_mgm* e, const int32_t* value_rank) {
    return e ? e->impl->set_value_rank(value_rank) : mxs_host::fail(MXS_E_INVALID, "null handle");
}
int mxs_mgm_run(mxs_mgm* e, int32_t n_rounds) {
    if (!e) return mxs_host::fail(MXS_E_INVALID, "null handle");
    if (n_rounds < 0) return mxs_host::fail(MXS_E_INVALID, "negative round count");
    return e->impl->run(n_rounds);
}
int mxs_mgm_rounds(const mxs_mgm* e, int64_t* rounds) {
    if (!e) return mxs_host::fail(MXS_E_INVALID, "null handle");
    if (rounds) *rounds = e->impl->rounds;
    return MXS_OK;
}
int mxs_mgm_get_state(mxs_mgm* e, int32_t* idx, double* cost, uint8_t* has_cost, double* gain, int32_t* new_value) {
    return e ? e->impl->get_state(0, idx, cost, has_cost, gain, new_value) : mxs_host::fail(MXS_E_INVALID, "null handle");
}
int mxs_mgm_get_state_replica(mxs_mgm* e, int32_t r, int32_t* idx, double* cost, uint8_t* has_cost, double* gain,
                              int32_t* new_value) {
    return e ? e->impl->get_state(r, idx, cost, has_cost, gain, new_value) : mxs_host::fail(MXS_E_INVALID, "null handle");
}
int mxs_mgm_replica_costs(mxs_mgm* e, double infinity, double* cost, int64_t* violations) {
    return e ? e->impl->replica_costs(infinity, cost, violations) : mxs_host::fail(MXS_E_INVALID, "null handle");
}
int mxs_mgm_best_replica(mxs_mgm* e, double infinity, int32_t* replica, double* cost, int64_t* violations) {
    return e ? e->impl->best_replica(infinity, replica, cost, violations) : mxs_host::fail(MXS_E_INVALID, "null handle");
}
int mxs_mgm_eval_cost(mxs_mgm* e, const int32_t* idx, double infinity, double* cost, int64_t* violations) {
    return e ? e->impl->eval_cost(idx, infinity, cost, violations) : mxs_host::fail(MXS_E_INVALID, "null handle");
}
int mxs_mgm_destroy(mxs_mgm* e) {
    if (e) {
        delete e->impl;
        delete e;
    }
    return MXS_OK;
}

}  // extern "C"

// MGM-2 (pydcop/algorithms/mgm2.py) on the same slot view and helpers
#include "mgm2.h"

// DPOP (pydcop/algorithms/dpop.py): UTIL / VALUE over a pseudo-tree, tables in one flat pool
#include "dpop.h"

// GDBA (pydcop/algorithms/gdba.py): the two phases of MGM's round plus per-slot modifier tables
#include "gdba.h"

// DBA (pydcop/algorithms/dba.py): the satisfaction algorithm GDBA generalises, on one bit per table entry
#include "dba.h"
