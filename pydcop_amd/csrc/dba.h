// dba.h -- the reference's DBA (pydcop/algorithms/dba.py: Yokoo & Hirayama's Distributed Breakout, the algorithm
// GDBA generalises) on gfx950, #included at the end of mgm.hip (one translation unit for the gfx950 library and
// for the serial emulated build of tests/emu).  The semantics restated here, quirks included, are listed with
// the reference's line numbers in tests/dba_oracle.py, which this file follows value for value.
//
// DBA is a constraint SATISFACTION algorithm: a constraint only ever asks "is this entry >= infinity?", and an
// evaluation is the sum of the integer weights of the violated constraints.  So the cost tables never reach the
// device: per (variable, constraint) SLOT the host keeps one BIT per table entry, in a private copy with the
// variable's own axis last (the shape of HostSlots::build_rows) -- for every combination of the other scope
// variables ceil(D_v / 32) words, bit x = the entry at own value x is >= infinity.  A slot of the hard
// 3-colouring is 12 bytes where GDBA reads a 72-byte f64 table.  All arithmetic is int32: no f32 / f64 split.
//
// Both phases of DbaComputation wait for all neighbours and park early messages, so a round is
// bulk-synchronous: two launches per round, each reading what the previous one wrote.
//   k_dba_eval    eval(x) of every value, the violated constraints at the current value, the best values (from
//                 `infinity`, :436), the improvement, the keyed choice of the new value, the termination counter
//                 as it is sent                                                            (ok phase, :366-445)
//   k_dba_decide  the neighbours' records (never their live state): counter = min, can_move / quasi-local-minimum
//                 by improvement and name, consistency; then _send_ok: the stop condition, the weight increase
//                 of the slots violated at the ok phase's values, the move             (improve phase, :504-562)
// The run ends with the first round in which any variable's stop condition holds: a stopper stores the round
// number into one device word (all stoppers of a round store the same value), both kernels return at once when
// that word holds an earlier round.  run(n) queues 2 n launches and reads the word back once.
//
// REPLICAS (mxs_dba_create_replicas): R seeded runs advance with the same two launches, as in gdba.h.  The phases
// are __device__ bodies (eval_phase, eval_wide_phase, decide_phase; REP = false / true) with two sets of __global__
// entry points and ONE host engine: k_dba_* on the plain Dev -- what an engine of mxs_dba_create launches for its one
// replica, argument layout and grid as a single run has always had them -- and k_dbar_* on DevR, where the replica is
// folded into blockIdx.x (block = r * bpr + b, replica_cost.h) and the block's copy of the argument moves once to
// replica r's slices of the dynamic state and takes seeds[r] (enter_replica).  The bit rows, their offsets and
// strides, the slot view, the domains, has_nb and the ranks are stored once; cur, cost, has_cost, counter, flags, rec
// are [R][n_vars], weight and viol [R][n_slots], stop and error [R].  A stopper stores the round into stop[r]; under
// the stop policy `first` it also stores it into one engine-wide word, and every replica's lanes return once that
// word holds an earlier round: every replica completes the round in which the first one stops.  Plain stores, no
// atomics: all stoppers of a round store the same value.  The constraints violated under every replica's assignment
// (DBA's rule: the bit of the row, i.e. entry >= infinity) are counted on the device: k_dbar_viol_partial /
// k_dbar_viol_final, in the fixed shape of replica_cost.h's cost reduction.
#pragma once

namespace dba {

using mxs_host::Buf;
using mxs_host::fail;
using mxs_host::uniform;

constexpr int TPB = 64;  // one wave per block, as gdba.h
constexpr int64_t DEFAULT_MASK_BUDGET = (int64_t)4 << 30;
// draw ids (the table in engine_common.h): 8 start value (cycle 0), 9 one of the best values
enum { D_START = 8, D_BEST = 9 };
enum { F_CONSISTENT = 1, F_CAN_MOVE = 2, F_QLM = 4 };

struct alignas(16) Rec {  // the improve message (:422-426) and what the ok phase keeps for _send_ok
    int32_t improve;      // _my_improve
    int32_t eval;         // current_eval
    int32_t counter;      // _termination_counter as sent
    int32_t newv;         // _new_value (-1: still None; it stays as it is in a round without improvement)
};

struct Dev {
    int32_t n_vars, max_distance;
    int32_t inf_lim;  // the smallest int32 that is >= infinity (clamped): eval < infinity <=> eval < inf_lim
    int32_t inf_eq;   // infinity itself where it is an int32, else -1 (no eval equals it)
    uint64_t seed;
    int32_t round;    // the round being run (1, 2, ...); the computations' cycle_count is round - 1 in the ok phase
    const int32_t *dom, *var_rowptr, *has_nb, *rank;
    const int32_t *nb_rowptr, *nb_var, *row_stride;  // per slot: the other scope variables, their stride in rows
    const int32_t *conc_rowptr, *conc_var;
    const int64_t* mask_off;  // [n_slots] first word of the slot's rows (-1: the variable never plays)
    const uint32_t* masks;
    int32_t* weight;          // [n_slots] __constraints_weights__
    uint8_t* viol;            // [n_slots] violated at the ok phase's values
    int32_t* cur;
    int32_t* cost;            // the held cost (the reference's __cost__)
    uint8_t* has_cost;
    int32_t* counter;         // _termination_counter after _send_ok
    uint8_t* flags;           // F_CONSISTENT | F_CAN_MOVE | F_QLM as _send_ok saw them
    Rec* rec;
    int32_t* stop;            // 0, or the round in which a stop condition held
    int32_t* error;           // sticky: improve > 0 with no best value (the reference raises IndexError, :412)
};

// what the replica engine's kernels take: Dev plus the replicas.  The single-run kernels keep the plain Dev, i.e.
// their argument layout.  The per-replica arrays of Dev -- cur, cost, has_cost, counter, flags, rec -- are
// [replicas][n_vars], weight and viol [replicas][n_slots], stop and error [replicas]; `seed` is filled per block from
// seeds[r] (enter_replica).
struct DevR : Dev {
    int32_t bpr;            // blocks per replica of the launch being made (block = replica * bpr + b)
    int32_t n_rep;
    int32_t stop_first;     // stop policy `first`: a stopper also stores the round into *first
    int64_t n_slots;        // a replica's share of weight / viol
    const uint64_t* seeds;  // [replicas]
    int32_t* first;         // the engine-wide word: 0, or the round in which the first replica stopped (policy `first`)
};

// the replica of this block: the block's copy of DevR (kernel arguments, block-uniform) moves to the replica's slices
// of the dynamic state and takes its seed, so that nothing below knows about replicas
__device__ inline int enter_replica(DevR& g, int* b) {
    const int r = repcost::replica_of_block<true>(g, b);
    const int64_t off = (int64_t)r * g.n_vars, soff = (int64_t)r * g.n_slots;
    g.cur += off, g.cost += off, g.has_cost += off, g.counter += off, g.flags += off, g.rec += off;
    g.weight += soff, g.viol += soff;
    g.stop += r, g.error += r;
    g.seed = g.seeds[r];
    return r;
}

// nothing of a run runs after the round of its stop; REP: nor after the round in which the first replica stopped
template <bool REP, typename G>
__device__ inline bool ended(const G& g) {
    const int32_t stopped = *g.stop;
    if (stopped != 0 && stopped < g.round) return true;
    if constexpr (REP) {
        const int32_t first = *g.first;
        if (first != 0 && first < g.round) return true;
    }
    return false;
}

// the slot's row for the neighbours' current values: the index of its first word
__device__ inline int64_t row_of(const Dev& g, int s, int words) {
    int64_t r = 0;
    for (int k = g.nb_rowptr[s]; k < g.nb_rowptr[s + 1]; ++k) r += (int64_t)g.cur[g.nb_var[k]] * g.row_stride[k];
    return g.mask_off[s] + r * words;
}

// _compute_best_improvement (:428-445) one value at a time: best_eval starts at infinity, `<` then `==`
struct Best {
    int32_t best, n;
    __device__ inline void take(int32_t e, int32_t inf_eq) {
        if (e < best) {
            best = e;
            n = 1;
        } else if (e == best && (n > 0 || e == inf_eq)) {
            ++n;
        }
    }
};

// improve() (:398-420) once the evaluations are known.  n == 0: every eval is above infinity, the current one
// included: improve > 0 with an empty list.
__device__ inline void finish_eval(const Dev& g, int v, int cv, int32_t cost, const Best& b, int32_t newv) {
    Rec r;
    r.eval = cost;
    r.improve = 0;
    r.newv = g.rec[v].newv;
    if (b.n == 0) *g.error = 1;
    else {
        r.improve = cost - b.best;
        if (r.improve > 0) r.newv = newv;
    }
    r.counter = cost == 0 ? g.counter[v] : 0;
    g.cost[v] = cost;
    g.has_cost[v] = 1;
    g.rec[v] = r;
}

// domains of at most MAXD <= 32 values: one word per row, the evaluations of all values in registers
template <bool REP, int MAXD, typename G>
__device__ inline void eval_phase(const G& g, int v) {
    if (ended<REP>(g)) return;
    if (v >= g.n_vars || !g.has_nb[v]) return;
    const int D = g.dom[v], cv = g.cur[v];
    int32_t acc[MAXD];
#pragma unroll
    for (int x = 0; x < MAXD; ++x) acc[x] = 0;
    const int s0 = g.var_rowptr[v], s1 = g.var_rowptr[v + 1];
    for (int s = s0; s < s1; s += 2) {  // two slots' words in flight together
        uint32_t w[2];
        int32_t wt[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int si = s + i < s1 ? s + i : s1 - 1;
            w[i] = g.masks[row_of(g, si, 1)];
            wt[i] = g.weight[si];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
            if (s + i < s1) {
                g.viol[s + i] = (uint8_t)((w[i] >> cv) & 1u);
#pragma unroll
                for (int x = 0; x < MAXD; ++x) acc[x] += (w[i] >> x) & 1u ? wt[i] : 0;
            }
    }
    const int32_t cost = lsearch::pick<int32_t, MAXD>(acc, cv);
    Best b{g.inf_lim, 0};
#pragma unroll
    for (int x = 0; x < MAXD; ++x)
        if (x < D) b.take(acc[x], g.inf_eq);
    int newv = cv;
    if (b.n > 0 && cost - b.best > 0) {
        const int k = (int)(uniform(g.seed, v, g.round - 1, D_BEST) * b.n);
        int seen = 0;
#pragma unroll
        for (int x = 0; x < MAXD; ++x) {  // the k-th best value in domain order
            const bool hit = x < D && acc[x] == b.best;
            newv = hit && seen == k ? x : newv;
            seen += hit ? 1 : 0;
        }
    }
    finish_eval(g, v, cv, cost, b, newv);
}

// eval(x) by a walk over the slots: any domain (rows of several words)
__device__ inline int32_t eval_at(const Dev& g, int v, int x, int words, bool mark) {
    int32_t acc = 0;
    for (int s = g.var_rowptr[v]; s < g.var_rowptr[v + 1]; ++s) {
        const uint32_t bit = (g.masks[row_of(g, s, words) + (x >> 5)] >> (x & 31)) & 1u;
        acc += bit ? g.weight[s] : 0;
        if (mark) g.viol[s] = (uint8_t)bit;
    }
    return acc;
}

template <bool REP, typename G>
__device__ inline void eval_wide_phase(const G& g, int v) {
    if (ended<REP>(g)) return;
    if (v >= g.n_vars || !g.has_nb[v]) return;
    const int D = g.dom[v], cv = g.cur[v], words = (D + 31) / 32;
    const int32_t cost = eval_at(g, v, cv, words, true);
    Best b{g.inf_lim, 0};
    for (int x = 0; x < D; ++x) b.take(x == cv ? cost : eval_at(g, v, x, words, false), g.inf_eq);
    int newv = cv;
    if (b.n > 0 && cost - b.best > 0) {
        int k = (int)(uniform(g.seed, v, g.round - 1, D_BEST) * b.n);
        for (int x = 0; x < D; ++x)
            if ((x == cv ? cost : eval_at(g, v, x, words, false)) == b.best && k-- == 0) {
                newv = x;
                break;
            }
    }
    finish_eval(g, v, cv, cost, b, newv);
}

template <bool REP, typename G>
__device__ inline void decide_phase(const G& g, int v) {
    if (ended<REP>(g)) return;
    if (v >= g.n_vars || !g.has_nb[v]) return;
    const Rec me = g.rec[v];
    // what improve() left (:402-415)
    bool consistent = me.eval == 0, can_move = me.improve > 0, qlm = !can_move;
    int32_t counter = me.counter;
    const int myrank = g.rank[v];
    // _handle_improve_message per neighbour (:509-519): idempotent and commutative
    for (int k = g.conc_rowptr[v]; k < g.conc_rowptr[v + 1]; ++k) {
        const int u = g.conc_var[k];
        if (u == v) continue;
        const Rec nb = g.rec[u];
        counter = nb.counter < counter ? nb.counter : counter;
        if (nb.improve > me.improve) {
            can_move = false;
            qlm = false;
        } else if (nb.improve == me.improve && myrank > g.rank[u]) {
            can_move = false;
        }
        if (nb.eval > 0) consistent = false;
    }
    // _send_ok (:537-562)
    bool stop = false;
    if (consistent) {
        counter += 1;
        stop = counter == g.max_distance;
    }
    g.counter[v] = counter;
    g.flags[v] = (uint8_t)((consistent ? F_CONSISTENT : 0) | (can_move ? F_CAN_MOVE : 0) | (qlm ? F_QLM : 0));
    if (stop) {
        *g.stop = g.round;
        if constexpr (REP) {
            if (g.stop_first) *g.first = g.round;
        }
        return;
    }
    if (qlm)
        for (int s = g.var_rowptr[v]; s < g.var_rowptr[v + 1]; ++s)
            if (g.viol[s]) g.weight[s] += 1;
    if (can_move) {  // value_selection(_new_value, __cost__ - _my_improve)
        g.cur[v] = me.newv;
        g.cost[v] = me.eval - me.improve;
    }
}

// ---- the entry points.  The single-run kernels: the plain Dev, the thread's index from blockIdx.x alone -- what
// mxs_dba_create has always launched.
template <int MAXD>
__global__ void __launch_bounds__(TPB) k_dba_eval(Dev g) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    eval_phase<false, MAXD>(g, v);
}
__global__ void __launch_bounds__(TPB) k_dba_eval_wide(Dev g) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    eval_wide_phase<false>(g, v);
}
__global__ void __launch_bounds__(TPB) k_dba_decide(Dev g) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    decide_phase<false>(g, v);
}

// The replica kernels (mxs_dba_create_replicas): R runs per launch, whole blocks (one wave each) belong to one
// replica (block = r * bpr + b); below enter_replica the phase code is the single run's, but for the engine-wide word.
template <int MAXD>
__global__ void __launch_bounds__(TPB) k_dbar_eval(DevR g) {
    int b;
    enter_replica(g, &b);
    eval_phase<true, MAXD>(g, b * (int)blockDim.x + (int)threadIdx.x);
}
__global__ void __launch_bounds__(TPB) k_dbar_eval_wide(DevR g) {
    int b;
    enter_replica(g, &b);
    eval_wide_phase<true>(g, b * (int)blockDim.x + (int)threadIdx.x);
}
__global__ void __launch_bounds__(TPB) k_dbar_decide(DevR g) {
    int b;
    enter_replica(g, &b);
    decide_phase<true>(g, b * (int)blockDim.x + (int)threadIdx.x);
}

// the start state of every replica (on_start, :341-349), thread per (replica, index): random.choice(domain) for every
// variable -- draw D_START of cycle 0 under seeds[r]; initial values are not looked at --, cost None, no new value;
// every weight 1
constexpr int AUX_TPB = rephost::AUX_TPB;
__global__ void __launch_bounds__(AUX_TPB) k_dbar_init(DevR g) {
    int b;
    enter_replica(g, &b);
    const int64_t i = (int64_t)b * (int)blockDim.x + (int)threadIdx.x;
    if (i < g.n_vars) {
        const int v = (int)i;
        g.cur[v] = (int)(uniform(g.seed, v, 0, D_START) * g.dom[v]);
        g.cost[v] = 0;
        g.has_cost[v] = 0;
        g.counter[v] = 0;
        g.flags[v] = 0;
        g.rec[v] = Rec{0, 0, 0, -1};
    }
    if (i < g.n_slots) {
        g.weight[i] = 1;
        g.viol[i] = 0;
    }
}

// ---- the constraints violated under every replica's current assignment, DBA's rule: the entry is >= infinity,
// compared as Plan::fill compares it (NaN: not violated) -- the bit of the row, read through one slot of a playing
// scope variable (ref_slot / ref_var; -1: no variable of the scope plays, the constraint is in `base`).  FIXED
// SHAPE, as repcost::k_cost_partial / k_cost_final: a thread folds VIOL_RUN consecutive constraints, the block's
// VIOL_TPB counts are combined by one tree in LDS, the block's partial goes to part[r][b]; k_dbar_viol_final adds a
// replica's partials in index order to base[r].  No atomics.
constexpr int VIOL_TPB = 256, VIOL_RUN = 4;
struct ViolArgs {
    const int32_t *ref_slot, *ref_var;  // [n_factors]
    int32_t n_factors;
    long long* part;                    // [n_rep][bpr]
};
__global__ void __launch_bounds__(VIOL_TPB) k_dbar_viol_partial(DevR g, ViolArgs a) {
    __shared__ long long s_viol[VIOL_TPB];
    int b;
    const int r = enter_replica(g, &b);
    const int t = (int)threadIdx.x;
    const int64_t i0 = ((int64_t)b * VIOL_TPB + t) * VIOL_RUN;
    long long n = 0;
    for (int64_t i = i0; i < i0 + VIOL_RUN && i < a.n_factors; ++i) {
        const int s = a.ref_slot[i];
        if (s < 0) continue;
        const int v = a.ref_var[i], x = g.cur[v];
        n += (g.masks[row_of(g, s, (g.dom[v] + 31) / 32) + (x >> 5)] >> (x & 31)) & 1u;
    }
    s_viol[t] = n;
    __syncthreads();
    for (int s = VIOL_TPB / 2; s > 0; s >>= 1) {
        if (t < s) s_viol[t] += s_viol[t + s];
        __syncthreads();
    }
    if (t == 0) a.part[(int64_t)r * g.bpr + b] = s_viol[0];
}
// thread per replica: base[r] (the constraints of variables that never play, constant after reset) plus the partials
// in index order
__global__ void __launch_bounds__(64) k_dbar_viol_final(int n_rep, int n_blocks, const long long* part,
                                                        const long long* base, long long* viol) {
    const int r = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (r >= n_rep) return;
    long long n = base[r];
    for (int b = 0; b < n_blocks; ++b) n += part[(int64_t)r * n_blocks + b];
    viol[r] = n;
}

// The host plan of the bit rows: where each playing variable's slots start, how many words there are
struct Plan {
    std::vector<int64_t> mask_off;     // per slot, in words; -1: none
    std::vector<int32_t> row_stride;   // per entry of nb_var: that variable's stride among the others, in rows
    int64_t words = 0;
    void build(const std::vector<int32_t>& dom, const std::vector<int32_t>& vrow, const std::vector<int32_t>& has_nb,
               const lsearch::HostSlots& hs) {
        const int nV = (int)dom.size();
        mask_off.assign(hs.base.size(), -1);
        row_stride.assign(hs.nb_var.size(), 0);
        words = 0;
        for (int v = 0; v < nV; ++v) {
            if (!has_nb[v]) continue;  // never plays
            const int64_t W = (dom[v] + 31) / 32;
            for (int s = vrow[v]; s < vrow[v + 1]; ++s) {
                // nb_var lists the others from the last scope position to the first: first listed = fastest
                int64_t R = 1;
                for (int k = hs.nb_rowptr[s]; k < hs.nb_rowptr[s + 1]; ++k) {
                    row_stride[k] = (int32_t)R;
                    R *= dom[hs.nb_var[k]];
                }
                mask_off[s] = words;
                words += R * W;
            }
        }
    }
    // bit x of a row = the table entry at own value x is >= infinity, compared in double (NaN: not violated)
    std::vector<uint32_t> fill(const std::vector<int32_t>& dom, const std::vector<int32_t>& vrow,
                               const lsearch::HostSlots& hs, const std::vector<double>& tables, double infinity) const {
        std::vector<uint32_t> m((size_t)words, 0u);
        std::vector<int> digit;
        for (int v = 0; v < (int)dom.size(); ++v)
            for (int s = vrow[v]; s < vrow[v + 1]; ++s) {
                if (mask_off[s] < 0) continue;
                const int D = dom[v], W = (D + 31) / 32;
                const int k0 = hs.nb_rowptr[s], no = hs.nb_rowptr[s + 1] - k0;
                int64_t R = 1;
                for (int k = 0; k < no; ++k) R *= dom[hs.nb_var[k0 + k]];
                digit.assign(no, 0);
                int64_t src = hs.base[s];
                uint32_t* dst = m.data() + mask_off[s];
                for (int64_t r = 0; r < R; ++r, dst += W) {
                    for (int x = 0; x < D; ++x)
                        if (tables[src + (int64_t)x * hs.stride_v[s]] >= infinity) dst[x >> 5] |= 1u << (x & 31);
                    for (int k = 0; k < no; ++k) {  // next combination of the others
                        src += hs.nb_stride[k0 + k];
                        if (++digit[k] < dom[hs.nb_var[k0 + k]]) break;
                        src -= (int64_t)hs.nb_stride[k0 + k] * digit[k];
                        digit[k] = 0;
                    }
                }
            }
        return m;
    }
};

struct Base {
    virtual ~Base() = default;
    virtual int init(const mxs_graph& g, const mxs_params& p, const int32_t* rank, double infinity, int32_t max_distance,
                     const uint64_t* seeds, int32_t n_replicas, int32_t stop_policy, bool single, int64_t budget,
                     int device) = 0;
    virtual int reset() = 0;
    virtual int run(int32_t n) = 0;
    virtual int get_state(int32_t r, int32_t* idx, int32_t* cost, uint8_t* has_cost, int32_t* eval, int32_t* improve,
                          int32_t* newv, int32_t* counter, uint8_t* consistent) = 0;
    virtual int get_weights(int32_t r, int32_t* out) = 0;
    virtual int eval_cost(const int32_t* idx, double infinity, double* cost, int64_t* viol) = 0;
    virtual int stop_rounds(int64_t* stop_round, int64_t* rounds_of) = 0;
    virtual int replica_violations(int64_t* viol) = 0;
    virtual int best_replica(int32_t* replica, int64_t* stop_round, int64_t* viol) = 0;
    int64_t rounds = 0, stop_round = 0, mask_bytes = 0;  // stop_round 0: the engine has not ended
    int32_t n_rep = 1;
};

enum { STOP_EACH = 0, STOP_FIRST = 1 };

// (violations, stop round with running = +infinity, index): the lexicographic minimum.  A stop does not imply a
// solution when max_distance is below the graph's diameter, so the violations come first.
inline int best_of(int n_rep, const long long* viol, const int32_t* stop) {
    int best = 0;
    for (int r = 1; r < n_rep; ++r) {
        const int64_t a = stop[r] ? stop[r] : INT64_MAX, b = stop[best] ? stop[best] : INT64_MAX;
        if (viol[r] < viol[best] || (viol[r] == viol[best] && a < b)) best = r;
    }
    return best;
}

// The one host engine: R >= 1 seeded runs of the instance with the launches one run needs.  The bit rows, their
// offsets and strides, the slot view, dom, has_nb and rank are stored once; cur, cost, counter, has_cost, flags, rec are
// [R][n_vars], weight and viol [R][n_slots], stop and error [R] (words: stop[R], error[R], then the engine-wide word);
// the seeds are a device array.  The engine ENDS when every replica has stopped (policy `each`) or with the round in
// which the first one stops (`first`); nothing runs after its end.
// `single` (mxs_dba_create): one replica under seeds = {seed} whose rounds are launched through the plain entry
// points on the Dev base of g -- replica 0's slices are the buffers' bases.
// (T, the table type of mxs_host::create<>, has no part in DBA: nothing here is floating point)
template <typename T>
struct Engine : Base {
    int device = 0;
    hipStream_t stream = nullptr;
    DevR g{};
    bool single = false;
    int32_t policy = STOP_EACH;
    Plan plan;
    mxs_host::HostGraph hg;
    std::vector<int32_t> h_nb, h_stop;  // h_stop [R]: the round in which the replica stopped (0: running)
    std::vector<uint64_t> h_seeds;
    lsearch::HostSlots hs;
    mxs_host::DevSlots sl;
    Buf<int32_t> dom, var_rowptr, has_nb, rank, row_stride, weight, cur, cost, counter, words, ref_slot, ref_var;
    Buf<int64_t> mask_off;
    Buf<uint32_t> masks;
    Buf<uint8_t> viol, has_cost, flags;
    Buf<Rec> rec;
    Buf<uint64_t> seeds;
    Buf<long long> viol_part, viol_base, rep_viol;
    int max_dom = 1, viol_blocks = 1;
    int64_t max_rounds = INT32_MAX;

    ~Engine() override {
        if (stream) (void)hipStreamDestroy(stream);
    }

    // the blocks of one replica in the launches: thread per variable, the start state, the violation count
    int var_blocks() const { return rephost::blocks_of(hg.nV, TPB); }
    int init_blocks() const { return rephost::blocks_of(std::max<int64_t>(hg.nV, (int64_t)hs.base.size()), AUX_TPB); }

    int init(const mxs_graph& G, const mxs_params& p, const int32_t* rk, double infinity, int32_t max_distance,
             const uint64_t* sds, int32_t n_replicas, int32_t stop_policy, bool one_run, int64_t budget, int dev) override {
        device = dev;
        single = one_run;
        if (n_replicas < 1 || n_replicas > repcost::MAX_REPLICAS)
            return fail(MXS_E_INVALID, "the number of replicas must be in 1 .. 4096");
        if (!sds) return fail(MXS_E_INVALID, "null seeds");
        if (stop_policy != STOP_EACH && stop_policy != STOP_FIRST)
            return fail(MXS_E_INVALID, "dba: the stop policy must be 0 (each) or 1 (first)");
        n_rep = n_replicas;
        policy = stop_policy;
        h_seeds.assign(sds, sds + n_replicas);
        if (int rc = mxs_host::open_device(dev, &stream)) return rc;
        if (p.mode == MXS_MODE_MAX)  // the constructor's ValueError (:295-298)
            return fail(MXS_E_INVALID, "DBA is a constraint **satisfaction** algorithm and only support minimization objective");
        if (!std::isfinite(infinity)) return fail(MXS_E_INVALID, "dba: infinity must be finite");
        if (budget < 0) return fail(MXS_E_INVALID, "dba: negative mask budget");
        if (budget == 0) budget = DEFAULT_MASK_BUDGET;
        if (int rc = hg.load(G, p)) return rc;
        const int nV = hg.nV, nF = hg.nF;
        for (int f = 0; f < nF; ++f)
            if (hg.toff[f + 1] <= hg.toff[f]) return fail(MXS_E_INVALID, "empty table");
        const std::string bad = hs.build(nV, nF, hg.dom, hg.frow, hg.evar, hg.toff, hg.vrow, hg.vedges);
        if (!bad.empty()) return fail(MXS_E_INVALID, bad);
        // a variable whose constraints hold no other variable never plays (:341-349, :373)
        h_nb.assign(nV, 0);
        int max_deg = 0;
        max_dom = 1;
        for (int v = 0; v < nV; ++v) {
            h_nb[v] = hs.conc_rowptr[v + 1] - hs.conc_rowptr[v] > 1;
            if (!h_nb[v]) continue;
            max_deg = std::max(max_deg, hg.vrow[v + 1] - hg.vrow[v]);
            max_dom = std::max(max_dom, hg.dom[v]);
        }
        // an eval is at most (slots of the variable) x (largest weight), a weight at most 1 + rounds: int32
        max_rounds = max_deg ? (int64_t)(INT32_MAX - 1) / max_deg - 1 : (int64_t)INT32_MAX;
        // the plan of the bit rows, checked against the budget before anything is allocated
        plan.build(hg.dom, hg.vrow, h_nb, hs);
        mask_bytes = plan.words * (int64_t)sizeof(uint32_t);
        if (plan.words > budget / (int64_t)sizeof(uint32_t))
            return fail(MXS_E_INVALID, "dba: the violation bit rows take " + std::to_string(mask_bytes) +
                                           " bytes, more than the budget of " + std::to_string(budget));
        // every launch folds the replica into blockIdx.x: the largest grid must fit
        viol_blocks = std::max(1, rephost::blocks_of(nF, VIOL_TPB * VIOL_RUN));
        const int64_t most = std::max<int64_t>({var_blocks(), init_blocks(), viol_blocks});
        if (most * (int64_t)n_rep > INT32_MAX) return fail(MXS_E_INVALID, "too many replicas for an instance of this size");
        std::vector<int32_t> h_rank(nV);
        for (int v = 0; v < nV; ++v) h_rank[v] = rk ? rk[v] : v;
        // per constraint, one slot of a playing scope variable (the violation count reads the constraint's bit there)
        std::vector<int32_t> h_ref_slot(nF, -1), h_ref_var(nF, -1);
        for (int v = 0; v < nV; ++v)
            for (int s = hg.vrow[v]; s < hg.vrow[v + 1]; ++s) {
                const int f = hg.efac[hg.vedges[s]];
                if (plan.mask_off[s] >= 0 && h_ref_slot[f] < 0) h_ref_slot[f] = s, h_ref_var[f] = v;
            }
        // the others hold no playing variable: their variables keep the start draw, their entry is constant after reset
        std::vector<long long> h_base(n_rep, 0);
        for (int f = 0; f < nF; ++f) {
            if (h_ref_slot[f] >= 0) continue;
            for (int r = 0; r < n_rep; ++r) {
                int64_t lin = 0;
                for (int e = hg.frow[f]; e < hg.frow[f + 1]; ++e) {
                    const int u = hg.evar[e];
                    lin = lin * hg.dom[u] + (int)(uniform(h_seeds[r], u, 0, D_START) * hg.dom[u]);
                }
                h_base[r] += hg.tables[hg.toff[f] + lin] >= infinity ? 1 : 0;
            }
        }
        if (int rc = sl.upload(hs, stream, nullptr, false)) return rc;
        MXS_TRY(masks.upload(plan.fill(hg.dom, hg.vrow, hs, hg.tables, infinity), stream));
        MXS_TRY(mask_off.upload(plan.mask_off, stream));
        MXS_TRY(row_stride.upload(plan.row_stride, stream));
        MXS_TRY(dom.upload(hg.dom, stream));
        MXS_TRY(var_rowptr.upload(hg.vrow, stream));
        MXS_TRY(has_nb.upload(h_nb, stream));
        MXS_TRY(rank.upload(h_rank, stream));
        MXS_TRY(ref_slot.upload(h_ref_slot, stream));
        MXS_TRY(ref_var.upload(h_ref_var, stream));
        MXS_TRY(seeds.upload(h_seeds, stream));
        MXS_TRY(viol_base.upload(h_base, stream));
        const size_t nS = hs.base.size(), R = (size_t)n_rep;
        if (int rc = rephost::alloc_rep(weight, R * nS, "weights")) return rc;
        if (int rc = rephost::alloc_rep(viol, R * nS, "violation flags")) return rc;
        if (int rc = rephost::alloc_rep(cur, R * nV, "values")) return rc;
        if (int rc = rephost::alloc_rep(cost, R * nV, "held costs")) return rc;
        if (int rc = rephost::alloc_rep(counter, R * nV, "termination counters")) return rc;
        if (int rc = rephost::alloc_rep(has_cost, R * nV, "cost flags")) return rc;
        if (int rc = rephost::alloc_rep(flags, R * nV, "flags")) return rc;
        if (int rc = rephost::alloc_rep(rec, R * nV, "improvement records")) return rc;
        if (int rc = rephost::alloc_rep(words, 2 * R + 1, "stop words")) return rc;
        if (int rc = rephost::alloc_rep(viol_part, R * viol_blocks, "violation partials")) return rc;
        if (int rc = rephost::alloc_rep(rep_viol, R, "violation counts")) return rc;
        const lsearch::Slots view = sl.view();
        g.n_vars = nV;
        g.max_distance = max_distance;
        const double up = std::ceil(infinity);
        g.inf_lim = up >= (double)INT32_MAX ? INT32_MAX : (up <= (double)INT32_MIN ? INT32_MIN : (int32_t)up);
        g.inf_eq = up == infinity && up >= 0.0 && up < (double)INT32_MAX ? (int32_t)up : -1;
        g.seed = single ? h_seeds[0] : 0;  // the replica kernels: seeds[r], per block
        g.bpr = 1, g.n_rep = n_rep, g.stop_first = policy == STOP_FIRST, g.n_slots = (int64_t)nS, g.seeds = seeds.p;
        g.dom = dom.p;
        g.var_rowptr = var_rowptr.p;
        g.has_nb = has_nb.p;
        g.rank = rank.p;
        g.nb_rowptr = view.nb_rowptr;
        g.nb_var = view.nb_var;
        g.row_stride = row_stride.p;
        g.conc_rowptr = view.conc_rowptr;
        g.conc_var = view.conc_var;
        g.mask_off = mask_off.p;
        g.masks = masks.p;
        g.weight = weight.p;
        g.viol = viol.p;
        g.cur = cur.p;
        g.cost = cost.p;
        g.has_cost = has_cost.p;
        g.counter = counter.p;
        g.flags = flags.p;
        g.rec = rec.p;
        g.stop = words.p;
        g.error = words.p + n_rep;
        g.first = words.p + 2 * n_rep;
        return reset();
    }

    // on_start (:341-349), every replica (k_dbar_init): random.choice(domain) for every variable, initial values are
    // not looked at; cost None; the weights 1; the stop words cleared
    int reset() override {
        MXS_TRY(hipSetDevice(device));
        if (g.n_vars) {
            g.bpr = init_blocks();
            hipLaunchKernelGGL(k_dbar_init, dim3((unsigned)(g.bpr * n_rep)), dim3(AUX_TPB), 0, stream, g);
            MXS_TRY(hipGetLastError());
        }
        MXS_TRY(hipMemsetAsync(words.p, 0, 4 * (2 * (size_t)n_rep + 1), stream));
        MXS_TRY(hipStreamSynchronize(stream));
        h_stop.assign(n_rep, 0);
        rounds = 0;
        stop_round = 0;
        return MXS_OK;
    }

    // the ok phase of all replicas; the single run: the plain entry points on the Dev part of g
    template <int MAXD>
    void launch_eval(const dim3& grid, const dim3& block) {
        if (single) hipLaunchKernelGGL((k_dba_eval<MAXD>), grid, block, 0, stream, (const Dev&)g);
        else hipLaunchKernelGGL((k_dbar_eval<MAXD>), grid, block, 0, stream, g);
    }

    int run(int32_t n) override {
        MXS_TRY(hipSetDevice(device));
        if (stop_round) return MXS_OK;  // the engine has ended: nothing after its end runs
        if (rounds + (int64_t)n > max_rounds)
            return fail(MXS_E_INVALID, "dba: weights and evals are int32, at most " + std::to_string(max_rounds) +
                                           " rounds on this instance");
        const int nV = g.n_vars;
        if (nV == 0) {
            rounds += n;
            return MXS_OK;
        }
        const int vbpr = var_blocks();
        const dim3 grid((unsigned)vbpr * (unsigned)n_rep), block(TPB);
        g.bpr = vbpr;  // (a kernel takes its argument by value: the copy is made at the launch)
        for (int32_t r = 0; r < n; ++r) {  // no read-back per round: the kernels of the rounds after a stop return at once
            g.round = (int32_t)(rounds + 1 + r);
            if (max_dom <= 4) launch_eval<4>(grid, block);
            else if (max_dom <= 8) launch_eval<8>(grid, block);
            else if (max_dom <= 32) launch_eval<32>(grid, block);
            else if (single) hipLaunchKernelGGL(k_dba_eval_wide, grid, block, 0, stream, (const Dev&)g);
            else hipLaunchKernelGGL(k_dbar_eval_wide, grid, block, 0, stream, g);
            MXS_TRY(hipGetLastError());
            if (single) hipLaunchKernelGGL(k_dba_decide, grid, block, 0, stream, (const Dev&)g);
            else hipLaunchKernelGGL(k_dbar_decide, grid, block, 0, stream, g);
            MXS_TRY(hipGetLastError());
        }
        const size_t R = (size_t)n_rep;
        std::vector<int32_t> w(2 * R + 1, 0);  // stop[R], error[R], the engine-wide word
        MXS_TRY(hipMemcpyAsync(w.data(), words.p, 4 * w.size(), hipMemcpyDeviceToHost, stream));
        MXS_TRY(hipStreamSynchronize(stream));
        for (size_t r = 0; r < R; ++r)
            if (w[R + r])
                return fail(MXS_E_STATE,
                            "dba: a variable improves with no best value: every eval of it is above infinity "
                            "(the reference raises IndexError there); infinity is too small for the weights" +
                                (single ? std::string() : " (replica " + std::to_string(r) + ")"));
        // a replica that stopped in the engine's last round or before it (policy `first`: the others never ran theirs)
        int64_t end = policy == STOP_FIRST ? w[2 * R] : 0;
        bool all = true;
        for (size_t r = 0; r < R; ++r) {
            h_stop[r] = w[r];
            all = all && w[r] != 0;
            if (policy == STOP_EACH) end = std::max<int64_t>(end, w[r]);
        }
        if (policy == STOP_EACH && !all) end = 0;
        if (end) rounds = stop_round = end;
        else rounds += n;
        return MXS_OK;
    }

    // per replica: the round in which it stopped (0: running) and the rounds it ran
    int stop_rounds(int64_t* stop_of, int64_t* rounds_of) override {
        for (int r = 0; r < n_rep; ++r) {
            if (stop_of) stop_of[r] = h_stop[r];
            if (rounds_of) rounds_of[r] = h_stop[r] ? h_stop[r] : rounds;
        }
        return MXS_OK;
    }

    // the violated constraints of every replica's current assignment into rep_viol, fetched
    int violations(std::vector<long long>& hv) {
        MXS_TRY(hipSetDevice(device));
        g.bpr = viol_blocks;
        const ViolArgs a{ref_slot.p, ref_var.p, hg.nF, viol_part.p};
        hipLaunchKernelGGL(k_dbar_viol_partial, dim3((unsigned)(viol_blocks * n_rep)), dim3(VIOL_TPB), 0, stream, g, a);
        MXS_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_dbar_viol_final, dim3((unsigned)rephost::blocks_of(n_rep, 64)), dim3(64), 0, stream, (int)n_rep,
                           viol_blocks, (const long long*)viol_part.p, (const long long*)viol_base.p, rep_viol.p);
        MXS_TRY(hipGetLastError());
        hv.resize(n_rep);
        MXS_TRY(hipMemcpyAsync(hv.data(), rep_viol.p, 8 * (size_t)n_rep, hipMemcpyDeviceToHost, stream));
        MXS_TRY(hipStreamSynchronize(stream));
        return MXS_OK;
    }

    int replica_violations(int64_t* out) override {
        std::vector<long long> hv;
        if (int rc = violations(hv)) return rc;
        for (int r = 0; r < n_rep; ++r)
            if (out) out[r] = (int64_t)hv[r];
        return MXS_OK;
    }

    int best_replica(int32_t* replica, int64_t* stop_of, int64_t* viol_out) override {
        std::vector<long long> hv;
        if (int rc = violations(hv)) return rc;
        const int r = best_of(n_rep, hv.data(), h_stop.data());
        if (replica) *replica = r;
        if (stop_of) *stop_of = h_stop[r];
        if (viol_out) *viol_out = (int64_t)hv[r];
        return MXS_OK;
    }

    int get_state(int32_t r, int32_t* idx, int32_t* cst, uint8_t* has, int32_t* ev, int32_t* imp, int32_t* nv, int32_t* cnt,
                  uint8_t* cons) override {
        if (r < 0 || r >= n_rep) return fail(MXS_E_INVALID, "replica out of range");
        MXS_TRY(hipSetDevice(device));
        const int nV = g.n_vars;
        if (!nV) return MXS_OK;
        std::vector<Rec> hr(nV);
        std::vector<uint8_t> hf(nV);
        const size_t roff = (size_t)r * nV;
        if (idx) MXS_TRY(hipMemcpyAsync(idx, cur.p + roff, 4 * (size_t)nV, hipMemcpyDeviceToHost, stream));
        if (cst) MXS_TRY(hipMemcpyAsync(cst, cost.p + roff, 4 * (size_t)nV, hipMemcpyDeviceToHost, stream));
        if (has) MXS_TRY(hipMemcpyAsync(has, has_cost.p + roff, (size_t)nV, hipMemcpyDeviceToHost, stream));
        if (cnt) MXS_TRY(hipMemcpyAsync(cnt, counter.p + roff, 4 * (size_t)nV, hipMemcpyDeviceToHost, stream));
        MXS_TRY(hipMemcpyAsync(hr.data(), rec.p + roff, sizeof(Rec) * (size_t)nV, hipMemcpyDeviceToHost, stream));
        MXS_TRY(hipMemcpyAsync(hf.data(), flags.p + roff, (size_t)nV, hipMemcpyDeviceToHost, stream));
        MXS_TRY(hipStreamSynchronize(stream));
        for (int v = 0; v < nV; ++v) {
            if (ev) ev[v] = hr[v].eval;
            if (imp) imp[v] = hr[v].improve;
            if (nv) nv[v] = hr[v].newv;
            if (cons) cons[v] = hf[v] & F_CONSISTENT ? 1 : 0;
        }
        return MXS_OK;
    }

    int get_weights(int32_t r, int32_t* out) override {
        if (r < 0 || r >= n_rep) return fail(MXS_E_INVALID, "replica out of range");
        MXS_TRY(hipSetDevice(device));
        const size_t nS = hs.base.size();
        if (!out || !nS) return MXS_OK;
        MXS_TRY(hipMemcpyAsync(out, weight.p + (size_t)r * nS, 4 * nS, hipMemcpyDeviceToHost, stream));
        MXS_TRY(hipStreamSynchronize(stream));
        return MXS_OK;
    }

    // DCOP.solution_cost of an assignment (constraints and the variables' own costs); NULL: replica 0's
    int eval_cost(const int32_t* idx, double infinity, double* cst, int64_t* viol_out) override {
        std::vector<int32_t> c;
        if (!idx) {
            c.resize(g.n_vars);
            int rc = get_state(0, c.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
            if (rc) return rc;
            idx = c.data();
        }
        return hg.eval_cost(idx, infinity, cst, viol_out);
    }
};

}  // namespace dba

struct mxs_dba {
    dba::Base* impl;
};

extern "C" {

int mxs_dba_create(const mxs_graph* g, const mxs_params* p, const int32_t* name_rank, double infinity, int32_t max_distance,
                   uint64_t seed, int64_t mask_budget_bytes, int32_t device, mxs_dba** out) {
    return mxs_host::create<mxs_dba, dba::Engine>(g, p, out, name_rank, infinity, max_distance, (const uint64_t*)&seed, 1,
                                                  (int32_t)dba::STOP_EACH, true, mask_budget_bytes, device);
}
int mxs_dba_create_replicas(const mxs_graph* g, const mxs_params* p, const int32_t* name_rank, double infinity,
                            int32_t max_distance, const uint64_t* seeds, int32_t n_replicas, int32_t stop_policy,
                            int64_t mask_budget_bytes, int32_t device, mxs_dba** out) {
    return mxs_host::create<mxs_dba, dba::Engine>(g, p, out, name_rank, infinity, max_distance, seeds, n_replicas, stop_policy,
                                                  false, mask_budget_bytes, device);
}
int mxs_dba_replicas(const mxs_dba* e, int32_t* n) {
    if (!e) return mxs_host::fail(MXS_E_INVALID, "null handle");
    if (n) *n = e->impl->n_rep;
    return MXS_OK;
}
int mxs_dba_reset(mxs_dba* e) { return e ? e->impl->reset() : mxs_host::fail(MXS_E_INVALID, "null handle"); }
int mxs_dba_run(mxs_dba* e, int32_t n_rounds) {
    if (!e) return mxs_host::fail(MXS_E_INVALID, "null handle");
    if (n_rounds < 0) return mxs_host::fail(MXS_E_INVALID, "negative round count");
    return e->impl->run(n_rounds);
}
int mxs_dba_rounds(const mxs_dba* e, int64_t* rounds) {
    if (!e) return mxs_host::fail(MXS_E_INVALID, "null handle");
    if (rounds) *rounds = e->impl->rounds;
    return MXS_OK;
}
int mxs_dba_finished(const mxs_dba* e, int32_t* stopped, int64_t* stop_round) {
    if (!e) return mxs_host::fail(MXS_E_INVALID, "null handle");
    if (stopped) *stopped = e->impl->stop_round != 0;
    if (stop_round) *stop_round = e->impl->stop_round;
    return MXS_OK;
}
int mxs_dba_get_state(mxs_dba* e, int32_t* idx, int32_t* cost, uint8_t* has_cost, int32_t* eval, int32_t* improve,
                      int32_t* new_value, int32_t* counter, uint8_t* consistent) {
    return e ? e->impl->get_state(0, idx, cost, has_cost, eval, improve, new_value, counter, consistent)
             : mxs_host::fail(MXS_E_INVALID, "null handle");
}
int mxs_dba_get_state_replica(mxs_dba* e, int32_t replica, int32_t* idx, int32_t* cost, uint8_t* has_cost, int32_t* eval,
                              int32_t* improve, int32_t* new_value, int32_t* counter, uint8_t* consistent) {
    return e ? e->impl->get_state(replica, idx, cost, has_cost, eval, improve, new_value, counter, consistent)
             : mxs_host::fail(MXS_E_INVALID, "null handle");
}
int mxs_dba_get_weights(mxs_dba* e, int32_t* out) {
    return e ? e->impl->get_weights(0, out) : mxs_host::fail(MXS_E_INVALID, "null handle");
}
int mxs_dba_get_weights_replica(mxs_dba* e, int32_t replica, int32_t* out) {
    return e ? e->impl->get_weights(replica, out) : mxs_host::fail(MXS_E_INVALID, "null handle");
}
int mxs_dba_stop_rounds(mxs_dba* e, int64_t* stop_round, int64_t* rounds) {
    return e ? e->impl->stop_rounds(stop_round, rounds) : mxs_host::fail(MXS_E_INVALID, "null handle");
}
int mxs_dba_replica_violations(mxs_dba* e, int64_t* violations) {
    return e ? e->impl->replica_violations(violations) : mxs_host::fail(MXS_E_INVALID, "null handle");
}
int mxs_dba_best_replica(mxs_dba* e, int32_t* replica, int64_t* stop_round, int64_t* violations) {
    return e ? e->impl->best_replica(replica, stop_round, violations) : mxs_host::fail(MXS_E_INVALID, "null handle");
}
int mxs_dba_mask_bytes(const mxs_dba* e, int64_t* bytes) {
    if (!e) return mxs_host::fail(MXS_E_INVALID, "null handle");
    if (bytes) *bytes = e->impl->mask_bytes;
    return MXS_OK;
}
int mxs_dba_eval_cost(mxs_dba* e, const int32_t* idx, double infinity, double* cost, int64_t* violations) {
    return e ? e->impl->eval_cost(idx, infinity, cost, violations) : mxs_host::fail(MXS_E_INVALID, "null handle");
}
int mxs_dba_destroy(mxs_dba* e) {
    if (e) {
        delete e->impl;
        delete e;
    }
    return MXS_OK;
}

}  // extern "C"
