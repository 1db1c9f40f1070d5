// mgm2.h -- the reference's MGM-2 (pydcop/algorithms/mgm2.py: Maheswaran, Pearce, Tambe 2004) on gfx950,
// #included at the end of mgm.hip (one translation unit for the gfx950 library and for the serial emulated
// build of tests/emu).  The semantics restated here expression by expression, quirks included, are listed
// with the reference's line numbers in tests/mgm2_oracle.py, which this file follows bit for bit.
//
// Every phase of Mgm2Computation waits for all its neighbours and parks early messages (_enter_state), so a
// round is bulk-synchronous: five launches per round, each reading what the previous one wrote.
//   k_mgm2_value    local cost at the current values (-> the held cost), offerer test, partner, best
//                   unilateral move and its gain                                   (value phase, :742-786)
//   k_mgm2_offers   one lane per (x, y) entry of an offerer's joint-move table: the cost over all its
//                   constraints with itself at x, the partner at y; kept when it strictly improves
//                                                                        (_compute_offers_to_send, :521-554)
//   k_mgm2_receive  a non-offerer evaluates the offers aimed at it, best global gain, ties, commit rule,
//                   the accepted offer; writes only its own record               (offer phase, :787-856)
//   k_mgm2_resolve  an offerer whose partner accepted takes the accepted value and gain (answer, :858-890)
//   k_mgm2_decide   gain comparison over the neighbourhood (name ranks for ties) and, for a committed pair,
//                   both go decisions computed on the fly                  (gain :892-972, go :974-1001)
// Every draw of the reference's unseeded `random` comes from the counter-based generator of engine_common.h keyed on
// (seed, variable, round, draw); the sequences a draw picks from are in canonical order (tests/mgm2_oracle.py).
// All cost sums run over the variable's constraints in the reference's order, starting from 0
// (assignment_cost, relations.py:1513-1531), through the slot view of local_search.h.
//
// REPLICAS (mxs_mgm2_create_replicas): R seeded runs advance with the same five launches, as in mgm.hip.  The five
// phases are __device__ bodies (value_phase .. decide_phase) with two sets of __global__ entry points and ONE host
// engine: k_mgm2_* on the plain Dev -- what an engine of mxs_mgm2_create launches for its one replica, argument layout
// and grid as a single run has always had them -- and k_mgm2r_* on DevR, where
// the replica is folded into blockIdx.x (block = r * bpr + b, replica_cost.h) and the block's copy of the argument
// moves once to replica r's slice of the dynamic state and takes seeds[r] (enter_replica).  Everything static is
// stored once; the state is [R][n_vars] / [R][n_entries] in GRAPH order (there is no packed order here).  The start
// state is drawn on the device (k_mgm2r_init), the solution costs are reduced by replica_cost.h's kernels, the
// refusals, the allocations that grow with R and the cost launches are replica_host.h's.
#pragma once

namespace mgm2 {

using mxs_host::Buf;
using mxs_host::fail;
using mxs_host::uniform;

constexpr int TPB = 64;    // thread-per-variable launches: one wave per block (latency-bound gathers)
constexpr int OTPB = 256;  // the offer-entry launch

// the draw ids (tests/mgm2_oracle.py): 0 start, 1 offerer test, 2 partner, 3 best unilateral value,
// 4 the `favor: no` coin, 5 the accepted offer among the tied best ones
enum { D_START = 0, D_OFFERER = 1, D_PARTNER = 2, D_BEST = 3, D_COIN = 4, D_OFFER = 5 };
enum { F_OFFERER = 1, F_COMMITTED = 2 };

template <typename T>
struct alignas(8) Rec {    // a variable's intended move of the round
    T gain;                // potential gain
    int32_t value;         // potential value
    int32_t partner;       // -1: none
    int32_t partner_value; // k_mgm2_receive: the value of the accepted offer for the offerer
    int32_t flags;         // F_OFFERER | F_COMMITTED
};

template <typename T>
struct Dev {
    int32_t n_vars, is_max, favor;  // favor: 0 unilateral, 1 no, 2 coordinated
    double threshold;
    uint64_t seed;
    int64_t round;                  // the reference's cycle_count during the round (1, 2, ...)
    const int32_t *dom, *var_rowptr, *has_nb, *rank;
    const int64_t* off_off;         // [n_vars + 1] offer table of v: off_off[v] .. off_off[v + 1]
    const int32_t* off_w;           // [n_vars] its row width P_v = the largest domain among v's neighbours
    const int32_t* ent_var;         // [n_entries] the variable an entry belongs to
    int64_t n_entries;
    const T* tables;
    lsearch::Slots slots;           // base, stride_v, nb_rowptr / nb_var / nb_stride, conc_rowptr / conc_var
    int32_t* cur;
    T* cost;                        // the held cost (current_cost); the local cost during a round
    uint8_t* has_cost;
    Rec<T>* uni;                    // value phase -> (resolve) -> the final move of the round
    Rec<T>* recv;                   // what a receiver decided
    T* offer;                       // [n_entries] offerer's gain of entry x * P_v + y
    uint8_t* offer_ok;              // the entry improves on the local cost
};

// what the replica engine's kernels take: Dev plus the replicas.  The single-run kernels keep the plain Dev, i.e.
// their argument layout.  The per-replica arrays of Dev -- cur, cost, has_cost, uni, recv -- are [replicas][n_vars],
// offer and offer_ok [replicas][n_entries]; `seed` is filled per block from seeds[r] (enter_replica).
template <typename T>
struct DevR : Dev<T> {
    int32_t bpr;               // blocks per replica of the launch being made (block = replica * bpr + b)
    int32_t n_rep;
    const uint64_t* seeds;     // [replicas]
    // what k_cost_partial (replica_cost.h) reads of its G: the constraints' CSR and q, here the identity -- the
    // state is in graph order
    const int32_t *dom_size, *factor_rowptr, *edge_var, *q;
    const int64_t* table_off;
};

// the replica of this block: the block's copy of DevR (kernel arguments, block-uniform) moves to the replica's slice
// of the dynamic state and takes its seed, so that nothing below knows about replicas
template <typename T>
__device__ inline int enter_replica(DevR<T>& g, int* b) {
    const int r = repcost::replica_of_block<true>(g, b);
    const int64_t off = (int64_t)r * g.n_vars, eoff = (int64_t)r * g.n_entries;
    g.cur += off, g.cost += off, g.has_cost += off, g.uni += off, g.recv += off;
    g.offer += eoff, g.offer_ok += eoff;
    g.seed = g.seeds[r];
    return r;
}

// assignment_cost over v's constraints in the reference's order, from 0: v at x, variable u at y (u < 0:
// none), every other variable at its current value; skip_u: only the constraints WITHOUT u
// (_find_best_offer's `concerned`, :575-582)
template <typename T>
__device__ inline T slot_sum(const Dev<T>& g, int v, int x, int u, int y, bool skip_u) {
    T acc = (T)0;
    for (int s = g.var_rowptr[v]; s < g.var_rowptr[v + 1]; ++s) {
        int64_t off = g.slots.base[s] + (int64_t)x * g.slots.stride_v[s];
        bool has_u = false;
        for (int k = g.slots.nb_rowptr[s]; k < g.slots.nb_rowptr[s + 1]; ++k) {
            const int w = g.slots.nb_var[k];
            const bool is_u = w == u;
            has_u |= is_u;
            off += (int64_t)(is_u ? y : g.cur[w]) * g.slots.nb_stride[k];
        }
        if (!(skip_u && has_u)) acc += g.tables[off];
    }
    return acc;
}

template <typename T>
__device__ __forceinline__ void value_phase(const Dev<T>& g, const int v) {
    if (v >= g.n_vars || !g.has_nb[v]) return;
    const int D = g.dom[v], cv = g.cur[v];
    const T lcost = slot_sum(g, v, cv, -1, 0, false);  // _current_local_cost -> __cost__
    g.cost[v] = lcost;
    g.has_cost[v] = 1;
    Rec<T> r;
    r.partner = -1;
    r.partner_value = -1;
    r.flags = 0;
    if (uniform(g.seed, v, g.round, D_OFFERER) < g.threshold) {  // partner: uniform among the distinct
        const int c0 = g.slots.conc_rowptr[v];                   // neighbours, ascending index (the
        const int n = g.slots.conc_rowptr[v + 1] - c0 - 1;       // list holds v itself once)
        const int k = (int)(uniform(g.seed, v, g.round, D_PARTNER) * n);
        const int p = g.slots.conc_var[c0 + k] < v ? c0 + k : c0 + k + 1;
        r.partner = g.slots.conc_var[p];
        r.flags = F_OFFERER;
    }
    // _compute_best_value: strictly better starts a new list, equal joins it (domain order)
    T best = (T)0;
    int n_best = 0;
    for (int x = 0; x < D; ++x) {
        const T c = x == cv ? lcost : slot_sum(g, v, x, -1, 0, false);
        if (n_best == 0 || (g.is_max ? best < c : best > c)) {
            best = c;
            n_best = 1;
        } else if (best == c) {
            ++n_best;
        }
    }
    const T pg = lcost - best;
    int pv = cv;
    if (g.is_max ? pg < (T)0 : pg > (T)0) {
        int k = (int)(uniform(g.seed, v, g.round, D_BEST) * n_best);
        for (int x = 0; x < D; ++x) {
            const T c = x == cv ? lcost : slot_sum(g, v, x, -1, 0, false);
            if (c == best && k-- == 0) {
                pv = x;
                break;
            }
        }
    }
    r.gain = pg;
    r.value = pv;
    g.uni[v] = r;
}

// one lane per entry of every variable's table; the lanes of non-offerers and the rows beyond the partner's
// domain write nothing (nobody reads them this round)
template <typename T>
__device__ __forceinline__ void offers_phase(const Dev<T>& g, const int64_t t) {
    if (t >= g.n_entries) return;
    const int v = g.ent_var[t];
    const Rec<T> r = g.uni[v];
    if (!(r.flags & F_OFFERER)) return;
    const int P = g.off_w[v];
    const int e = (int)(t - g.off_off[v]), x = e / P, y = e % P;
    if (y >= g.dom[r.partner]) return;
    const T c = slot_sum(g, v, x, r.partner, y, false);
    const T lc = g.cost[v];
    const bool ok = g.is_max ? lc < c : lc > c;
    g.offer[t] = ok ? lc - c : (T)0;
    g.offer_ok[t] = ok ? 1 : 0;
}

template <typename T>
__device__ __forceinline__ void receive_phase(const Dev<T>& g, const int v) {
    if (v >= g.n_vars || !g.has_nb[v]) return;
    const Rec<T> me = g.uni[v];
    Rec<T> out;
    out.gain = (T)0;
    out.value = -1;
    out.partner = -1;
    out.partner_value = -1;
    out.flags = 0;
    if (!(me.flags & F_OFFERER)) {
        const T lcost = g.cost[v];
        const int D = g.dom[v];
        const int c0 = g.slots.conc_rowptr[v], c1 = g.slots.conc_rowptr[v + 1];
        // best global gain and its ties (the count does not depend on the scan order: the running best only
        // improves, so every entry equal to the final best comes at or after the one that set it)
        T best = (T)0;
        int64_t n_best = 0;
        for (int k = c0; k < c1; ++k) {
            const int u = g.slots.conc_var[k];
            if (u == v) continue;
            const Rec<T> ru = g.uni[u];
            if (!(ru.flags & F_OFFERER) || ru.partner != v) continue;
            const int Du = g.dom[u], P = g.off_w[u];
            const int64_t b = g.off_off[u];
            for (int yr = 0; yr < D; ++yr) {
                const T d = lcost - slot_sum(g, v, yr, u, 0, true);
                for (int xo = 0; xo < Du; ++xo) {
                    const int64_t i = b + (int64_t)xo * P + yr;
                    if (!g.offer_ok[i]) continue;
                    const T gg = d + g.offer[i];
                    if (g.is_max ? gg < best : gg > best) {
                        best = gg;
                        n_best = 1;
                    } else if (gg == best) {
                        ++n_best;
                    }
                }
            }
        }
        bool commit = false;
        if (best != (T)0 && n_best > 0) {
            if (g.is_max ? best < me.gain : best > me.gain) commit = true;
            else if (best == me.gain)
                commit = g.favor == 2 || (g.favor == 1 && uniform(g.seed, v, g.round, D_COIN) > 0.5);
        }
        if (commit) {  // the k-th tied offer in (offerer index, offerer value, own value) order
            int64_t kk = (int64_t)(uniform(g.seed, v, g.round, D_OFFER) * (double)n_best);
            for (int k = c0; k < c1 && out.flags == 0; ++k) {
                const int u = g.slots.conc_var[k];
                if (u == v) continue;
                const Rec<T> ru = g.uni[u];
                if (!(ru.flags & F_OFFERER) || ru.partner != v) continue;
                const int Du = g.dom[u], P = g.off_w[u];
                const int64_t b = g.off_off[u];
                for (int xo = 0; xo < Du && out.flags == 0; ++xo)
                    for (int yr = 0; yr < D; ++yr) {
                        const int64_t i = b + (int64_t)xo * P + yr;
                        if (!g.offer_ok[i]) continue;
                        const T gg = (lcost - slot_sum(g, v, yr, u, 0, true)) + g.offer[i];
                        if (gg == best && kk-- == 0) {
                            out.gain = best;
                            out.value = yr;
                            out.partner = u;
                            out.partner_value = xo;
                            out.flags = F_COMMITTED;
                            break;
                        }
                    }
            }
        }
    }
    g.recv[v] = out;
}

template <typename T>
__device__ __forceinline__ void resolve_phase(const Dev<T>& g, const int v) {
    if (v >= g.n_vars || !g.has_nb[v]) return;
    Rec<T> me = g.uni[v];
    if (me.flags & F_OFFERER) {
        const Rec<T> rp = g.recv[me.partner];
        if ((rp.flags & F_COMMITTED) && rp.partner == v) {
            me.gain = rp.gain;
            me.value = rp.partner_value;
            me.flags |= F_COMMITTED;
        }
    } else {
        const Rec<T> rr = g.recv[v];
        if (rr.flags & F_COMMITTED) {
            me.gain = rr.gain;
            me.value = rr.value;
            me.partner = rr.partner;
            me.flags |= F_COMMITTED;
        }
    }
    g.uni[v] = me;
}

// a committed variable's can_move: its gain beats every neighbour's but its partner's (or there is none)
template <typename T>
__device__ inline bool can_move(const Dev<T>& g, int a, int partner, T gain) {
    bool any = false;
    T mx = (T)0;
    for (int k = g.slots.conc_rowptr[a]; k < g.slots.conc_rowptr[a + 1]; ++k) {
        const int u = g.slots.conc_var[k];
        if (u == a || u == partner) continue;
        const T gu = g.uni[u].gain;
        if (!any || gu > mx) mx = gu;
        any = true;
    }
    return !any || gain > mx;
}

template <typename T>
__device__ __forceinline__ void decide_phase(const Dev<T>& g, const int v) {
    if (v >= g.n_vars || !g.has_nb[v]) return;
    const Rec<T> me = g.uni[v];
    if (me.gain == (T)0) return;  // nothing to do this round; the held cost stays the local cost
    bool move;
    if (me.flags & F_COMMITTED) {  // go from the partner and its own can_move (both sides the same gain)
        move = can_move(g, v, me.partner, me.gain) && can_move(g, me.partner, v, me.gain);
    } else {  // max() and > in both modes (:950-970), ties: the first name of sorted(tied + itself)
        const int myrank = g.rank[v];
        T mx = (T)0;
        bool first = true, wins = true;
        for (int k = g.slots.conc_rowptr[v]; k < g.slots.conc_rowptr[v + 1]; ++k) {
            const int u = g.slots.conc_var[k];
            if (u == v) continue;
            const T gu = g.uni[u].gain;
            const bool lower = g.rank[u] < myrank;
            if (first || gu > mx) {
                mx = gu;
                wins = !lower;
            } else if (gu == mx && lower) {
                wins = false;
            }
            first = false;
        }
        move = me.gain > mx || (me.gain == mx && wins);
    }
    if (move) {  // value_selection(potential_value, current_cost - potential_gain)
        g.cur[v] = me.value;
        g.cost[v] = g.cost[v] - me.gain;
    }
}

// ---- the entry points.  The single-run kernels: the plain Dev, the thread's index from blockIdx.x alone -- what
// mxs_mgm2_create has always launched.
template <typename T>
__global__ void __launch_bounds__(TPB) k_mgm2_value(Dev<T> g) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    value_phase(g, v);
}
template <typename T>
__global__ void __launch_bounds__(OTPB) k_mgm2_offers(Dev<T> g) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    offers_phase(g, t);
}
template <typename T>
__global__ void __launch_bounds__(TPB) k_mgm2_receive(Dev<T> g) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    receive_phase(g, v);
}
template <typename T>
__global__ void __launch_bounds__(TPB) k_mgm2_resolve(Dev<T> g) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    resolve_phase(g, v);
}
template <typename T>
__global__ void __launch_bounds__(TPB) k_mgm2_decide(Dev<T> g) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    decide_phase(g, v);
}

// The replica kernels (mxs_mgm2_create_replicas): R runs per launch, whole blocks belong to one replica
// (block = r * bpr + b); below enter_replica the phase code is the single run's.
template <typename T>
__global__ void __launch_bounds__(TPB) k_mgm2r_value(DevR<T> g) {
    int b;
    enter_replica(g, &b);
    value_phase<T>(g, b * (int)blockDim.x + (int)threadIdx.x);
}
template <typename T>
__global__ void __launch_bounds__(OTPB) k_mgm2r_offers(DevR<T> g) {
    int b;
    enter_replica(g, &b);
    offers_phase<T>(g, (int64_t)b * blockDim.x + threadIdx.x);
}
template <typename T>
__global__ void __launch_bounds__(TPB) k_mgm2r_receive(DevR<T> g) {
    int b;
    enter_replica(g, &b);
    receive_phase<T>(g, b * (int)blockDim.x + (int)threadIdx.x);
}
template <typename T>
__global__ void __launch_bounds__(TPB) k_mgm2r_resolve(DevR<T> g) {
    int b;
    enter_replica(g, &b);
    resolve_phase<T>(g, b * (int)blockDim.x + (int)threadIdx.x);
}
template <typename T>
__global__ void __launch_bounds__(TPB) k_mgm2r_decide(DevR<T> g) {
    int b;
    enter_replica(g, &b);
    decide_phase<T>(g, b * (int)blockDim.x + (int)threadIdx.x);
}

// the start state of every replica (on_start, :460-495), thread per (replica, variable): a variable with neighbours
// keeps its initial value (the same in every replica) or takes int(u * D_v); one without neighbours takes the k-th of
// its best own-constraint values (best_val[best_off[v] ..], uploaded once) and holds their cost.  u: draw 0 of
// cycle 0 under seeds[r].
constexpr int AUX_TPB = rephost::AUX_TPB;
template <typename T>
__global__ void __launch_bounds__(AUX_TPB) k_mgm2r_init(DevR<T> g, const int32_t* init, const int64_t* best_off,
                                                        const int32_t* best_val, const T* best_cost) {
    int b;
    enter_replica(g, &b);
    const int v = b * (int)blockDim.x + (int)threadIdx.x;
    if (v >= g.n_vars) return;
    const double u = uniform(g.seed, v, 0, D_START);
    int x;
    if (g.has_nb[v]) {
        x = init[v] >= 0 ? init[v] : (int)(u * g.dom[v]);
    } else {
        const int64_t b0 = best_off[v];
        x = best_val[b0 + (int64_t)(u * (double)(best_off[v + 1] - b0))];
    }
    g.cur[v] = x;
    g.cost[v] = g.has_nb[v] ? (T)0 : best_cost[v];
    g.has_cost[v] = g.has_nb[v] ? 0 : 1;
}

// ---- the host side
inline int check_params(double threshold, int32_t favor) {
    if (!(threshold >= 0.0 && threshold <= 1.0)) return fail(MXS_E_INVALID, "threshold must be in [0, 1]");
    if (favor < 0 || favor > 2) return fail(MXS_E_INVALID, "favor must be 0 (unilateral), 1 (no) or 2 (coordinated)");
    return MXS_OK;
}

// max() over NaN gains depends on message arrival in the reference: no defined result
inline int check_tables(const mxs_host::HostGraph& hg) {
    for (double t : hg.tables)
        if (!std::isfinite(t)) return fail(MXS_E_INVALID, "mgm2: constraint tables must be finite (no inf / NaN entries)");
    return MXS_OK;
}

// who has neighbours (the other variables of v's constraints: the concerned list holds v itself once) and the
// offer tables: D_v rows of P_v = the largest domain among v's neighbours
struct Layout {
    std::vector<int32_t> has_nb, width, ent_var;
    std::vector<int64_t> off;
    int build(const mxs_host::HostGraph& hg, const lsearch::HostSlots& hs) {
        const int nV = hg.nV;
        has_nb.assign(nV, 0);
        width.assign(nV, 0);
        off.assign(nV + 1, 0);
        for (int v = 0; v < nV; ++v) {
            int P = 0;
            for (int k = hs.conc_rowptr[v]; k < hs.conc_rowptr[v + 1]; ++k)
                if (hs.conc_var[k] != v) P = std::max(P, hg.dom[hs.conc_var[k]]);
            has_nb[v] = P > 0;
            width[v] = P;
            off[v + 1] = off[v] + (int64_t)hg.dom[v] * P;
        }
        if (off[nV] > INT32_MAX) return fail(MXS_E_INVALID, "mgm2: offer tables larger than 2^31 entries");
        ent_var.resize((size_t)off[nV]);
        for (int v = 0; v < nV; ++v)
            for (int64_t i = off[v]; i < off[v + 1]; ++i) ent_var[(size_t)i] = v;
        return MXS_OK;
    }
};

// on_start of a variable without neighbours (:460-470): the best values of its own constraints, in domain order
// (strictly better starts a new list, equal joins it), and their cost
template <typename T>
T best_own_values(const mxs_host::HostGraph& hg, const lsearch::HostSlots& hs, int v, std::vector<int32_t>& vals) {
    T best = (T)0;
    vals.clear();
    for (int x = 0; x < hg.dom[v]; ++x) {
        T acc = (T)0;
        for (int s = hg.vrow[v]; s < hg.vrow[v + 1]; ++s) acc += (T)hg.tables[hs.base[s] + (int64_t)x * hs.stride_v[s]];
        if (vals.empty() || (hg.is_max ? best < acc : best > acc)) {
            best = acc;
            vals.assign(1, x);
        } else if (best == acc) {
            vals.push_back(x);
        }
    }
    return best;
}

inline std::vector<int32_t> ranks_or_index(const int32_t* rk, int nV) {
    std::vector<int32_t> h(nV);
    for (int v = 0; v < nV; ++v) h[v] = rk ? rk[v] : v;
    return h;
}

// Engine<T> behind struct mxs_mgm2, whatever its T
struct Base {
    virtual ~Base() = default;
    virtual int init(const mxs_graph& G, const mxs_params& p, const int32_t* name_rank, double threshold, int32_t favor,
                     const uint64_t* seeds, int32_t n_replicas, bool single, int dev) = 0;
    virtual int reset() = 0;
    virtual int run(int32_t n) = 0;
    virtual int get_state(int32_t r, int32_t* idx, double* cost, uint8_t* has_cost) = 0;
    virtual int eval_cost(const int32_t* idx, double infinity, double* cost, int64_t* viol) = 0;
    virtual int replica_costs(double infinity, double* cost, int64_t* viol) = 0;
    virtual int best_replica(double infinity, int32_t* replica, double* cost, int64_t* viol) = 0;
    int64_t rounds = 0;
    int32_t n_rep = 1;
};

// The one host engine: R >= 1 seeded runs of the instance with the launches one run needs.  The slot view, the
// tables, dom, rank and the offer tables' layout are stored once; cur, cost, has_cost, uni, recv are [R][n_vars],
// offer and offer_ok [R][n_entries]; the seeds are a device array.  The refusals, the allocations that grow with R
// and the cost launches are rephost::Host's (replica_host.h, shared with dsa.hip and mgm.hip); MGM-2 keeps its
// variables in graph order, so Host's q is the identity (graph_order).  MGM-2's sum stops improving at a local
// optimum and is not tracked: the CURRENT states are ranked (Host::best_current).
// `single` (mxs_mgm2_create): one replica under seeds = {seed} whose rounds are launched through the plain entry
// points on the Dev base of g -- replica 0's slices are the buffers' bases.  It keeps the single run's API: its
// replica cost, and the best replica's, is the host's eval_cost.
template <typename T>
struct Engine : Base {
    rephost::Host<T> rh;
    DevR<T> g{};
    bool single = false;
    mxs_host::DevSlots sl;
    Buf<int32_t> rank, off_w, ent_var, init_idx, best_val;
    Buf<int64_t> off_off, best_off;
    Buf<T> best_cost;
    Buf<int32_t> cur;                 // the dynamic state: [R][n_vars], graph order
    Buf<T> cost, offer;
    Buf<uint8_t> has_cost, offer_ok;
    Buf<Rec<T>> uni, recv;

    int init(const mxs_graph& G, const mxs_params& p, const int32_t* rk, double threshold, int32_t favor,
             const uint64_t* sds, int32_t n_replicas, bool one_run, int dev) override {
        single = one_run;
        if (int rc = rh.open(sds, n_replicas, dev, true)) return rc;
        n_rep = rh.n_rep;
        if (int rc = check_params(threshold, favor)) return rc;
        if (int rc = rh.hg.load(G, p)) return rc;
        if (int rc = check_tables(rh.hg)) return rc;
        if (int rc = rh.hg.load_init(G)) return rc;
        const mxs_host::HostGraph& hg = rh.hg;
        const hipStream_t stream = rh.stream;
        const int nV = hg.nV;
        lsearch::HostSlots hs;
        const std::string bad = hs.build(nV, hg.nF, hg.dom, hg.frow, hg.evar, hg.toff, hg.vrow, hg.vedges);
        if (!bad.empty()) return fail(MXS_E_INVALID, bad);
        Layout lay;
        if (int rc = lay.build(hg, hs)) return rc;
        const int64_t nE = lay.off[nV];
        if (int rc = rh.graph_order(lay.has_nb, std::max<int64_t>(rephost::blocks_of(nV, TPB), rephost::blocks_of(nE, OTPB))))
            return rc;
        // the start of the variables without neighbours: their best values and the cost, whatever the replicas
        std::vector<int64_t> b_off(nV + 1, 0);
        std::vector<int32_t> b_val, vals;
        std::vector<T> b_cost(nV, (T)0);
        for (int v = 0; v < nV; ++v) {
            if (!lay.has_nb[v]) {
                b_cost[v] = best_own_values<T>(hg, hs, v, vals);
                b_val.insert(b_val.end(), vals.begin(), vals.end());
            }
            b_off[v + 1] = (int64_t)b_val.size();
        }
        if (int rc = sl.upload(hs, stream, nullptr, false)) return rc;  // no first-neighbour arrays, no rows
        if (int rc = rh.upload_order()) return rc;
        if (int rc = rh.upload_graph()) return rc;
        MXS_TRY(rank.upload(ranks_or_index(rk, nV), stream));
        MXS_TRY(off_w.upload(lay.width, stream));
        MXS_TRY(off_off.upload(lay.off, stream));
        MXS_TRY(ent_var.upload(lay.ent_var, stream));
        MXS_TRY(init_idx.upload(hg.init, stream));
        MXS_TRY(best_off.upload(b_off, stream));
        MXS_TRY(best_val.upload(b_val, stream));
        MXS_TRY(best_cost.upload(b_cost, stream));
        const size_t R = (size_t)n_rep;
        if (int rc = rephost::alloc_rep(cur, R * nV, "values")) return rc;
        if (int rc = rephost::alloc_rep(cost, R * nV, "held costs")) return rc;
        if (int rc = rephost::alloc_rep(has_cost, R * nV, "cost flags")) return rc;
        if (int rc = rephost::alloc_rep(uni, R * nV, "move records")) return rc;
        if (int rc = rephost::alloc_rep(recv, R * nV, "receiver records")) return rc;
        if (int rc = rephost::alloc_rep(offer, R * (size_t)nE, "offer tables")) return rc;
        if (int rc = rephost::alloc_rep(offer_ok, R * (size_t)nE, "offer tables")) return rc;
        g.favor = favor;
        g.threshold = threshold;
        g.n_entries = nE;
        bind();
        return reset();
    }

    // the kernels' argument: the Dev part, the per-replica arrays at their bases (replica 0's slices), then DevR's
    void bind() {
        g.slots = sl.view();
        g.n_vars = rh.hg.nV, g.is_max = rh.hg.is_max;
        g.seed = single ? rh.h_seeds[0] : 0;  // the replica kernels: seeds[r], per block
        g.dom = rh.dom_size.p, g.var_rowptr = rh.var_rowptr.p, g.has_nb = rh.n_neigh.p, g.rank = rank.p;
        g.off_off = off_off.p, g.off_w = off_w.p, g.ent_var = ent_var.p, g.tables = rh.tables.p;
        g.cur = cur.p, g.cost = cost.p, g.has_cost = has_cost.p, g.uni = uni.p, g.recv = recv.p;
        g.offer = offer.p, g.offer_ok = offer_ok.p;
        g.bpr = 1, g.n_rep = n_rep, g.seeds = rh.seeds.p;
        g.dom_size = rh.dom_size.p, g.factor_rowptr = rh.factor_rowptr.p, g.edge_var = rh.edge_var.p;
        g.q = rh.qmap.p, g.table_off = rh.table_off.p;
    }

    // every replica back to its start state (k_mgm2r_init): nothing is uploaded
    int reset() override {
        MXS_TRY(hipSetDevice(rh.device));
        rounds = 0;
        if (g.n_vars) {
            g.bpr = rephost::blocks_of(g.n_vars, AUX_TPB);
            hipLaunchKernelGGL((k_mgm2r_init<T>), dim3((unsigned)(g.bpr * n_rep)), dim3(AUX_TPB), 0, rh.stream, g,
                               (const int32_t*)init_idx.p, (const int64_t*)best_off.p, (const int32_t*)best_val.p,
                               (const T*)best_cost.p);
            MXS_TRY(hipGetLastError());
            MXS_TRY(hipStreamSynchronize(rh.stream));
        }
        return MXS_OK;
    }

    int run(int32_t n) override {
        MXS_TRY(hipSetDevice(rh.device));
        const hipStream_t stream = rh.stream;
        const int nV = g.n_vars;
        if (nV == 0) {
            rounds += n > 0 ? n : 0;
            return MXS_OK;
        }
        const int vbpr = rephost::blocks_of(nV, TPB), obpr = rephost::blocks_of(g.n_entries, OTPB);
        const dim3 grid((unsigned)vbpr * (unsigned)n_rep), block(TPB);
        const dim3 ogrid((unsigned)obpr * (unsigned)n_rep), oblock(OTPB);
        const Dev<T>& one = g;  // what a single run's launches copy: the Dev part
        for (int32_t r = 0; r < n; ++r) {
            g.round = rounds + 1;
            if (single) {
                hipLaunchKernelGGL((k_mgm2_value<T>), grid, block, 0, stream, one);
                MXS_TRY(hipGetLastError());
                if (g.n_entries > 0) {
                    hipLaunchKernelGGL((k_mgm2_offers<T>), ogrid, oblock, 0, stream, one);
                    MXS_TRY(hipGetLastError());
                }
                hipLaunchKernelGGL((k_mgm2_receive<T>), grid, block, 0, stream, one);
                MXS_TRY(hipGetLastError());
                hipLaunchKernelGGL((k_mgm2_resolve<T>), grid, block, 0, stream, one);
                MXS_TRY(hipGetLastError());
                hipLaunchKernelGGL((k_mgm2_decide<T>), grid, block, 0, stream, one);
                MXS_TRY(hipGetLastError());
            } else {
                g.bpr = vbpr;  // (a kernel takes its DevR by value: the copy is made at the launch)
                hipLaunchKernelGGL((k_mgm2r_value<T>), grid, block, 0, stream, g);
                MXS_TRY(hipGetLastError());
                if (g.n_entries > 0) {
                    g.bpr = obpr;
                    hipLaunchKernelGGL((k_mgm2r_offers<T>), ogrid, oblock, 0, stream, g);
                    MXS_TRY(hipGetLastError());
                    g.bpr = vbpr;
                }
                hipLaunchKernelGGL((k_mgm2r_receive<T>), grid, block, 0, stream, g);
                MXS_TRY(hipGetLastError());
                hipLaunchKernelGGL((k_mgm2r_resolve<T>), grid, block, 0, stream, g);
                MXS_TRY(hipGetLastError());
                hipLaunchKernelGGL((k_mgm2r_decide<T>), grid, block, 0, stream, g);
                MXS_TRY(hipGetLastError());
            }
            rounds += 1;
        }
        MXS_TRY(hipStreamSynchronize(stream));
        return MXS_OK;
    }

    int get_state(int32_t r, int32_t* idx, double* cst, uint8_t* has) override {
        if (r < 0 || r >= n_rep) return fail(MXS_E_INVALID, "replica out of range");
        MXS_TRY(hipSetDevice(rh.device));
        const hipStream_t stream = rh.stream;
        const int nV = g.n_vars;
        if (!nV) return MXS_OK;
        std::vector<T> hc(nV);
        std::vector<uint8_t> hh(nV);
        const size_t roff = (size_t)r * nV;
        if (idx) MXS_TRY(hipMemcpyAsync(idx, cur.p + roff, 4 * (size_t)nV, hipMemcpyDeviceToHost, stream));
        if (has) MXS_TRY(hipMemcpyAsync(has, has_cost.p + roff, nV, hipMemcpyDeviceToHost, stream));
        if (cst) MXS_TRY(hipMemcpyAsync(hc.data(), cost.p + roff, sizeof(T) * (size_t)nV, hipMemcpyDeviceToHost, stream));
        MXS_TRY(hipStreamSynchronize(stream));
        for (int v = 0; cst && v < nV; ++v) cst[v] = (double)hc[v];
        return MXS_OK;
    }

    int eval_cost(const int32_t* idx, double infinity, double* cst, int64_t* viol) override {
        return rh.eval_cost(idx, infinity, cst, viol, [&](int32_t* out) { return get_state(0, out, nullptr, nullptr); });
    }

    // the device's reduction; a single run's cost is eval_cost's (the host's summation order), and it is the best replica
    int replica_costs(double infinity, double* cst, int64_t* viol) override {
        if (single) return eval_cost(nullptr, infinity, cst, viol);
        return rh.replica_costs(g, cur.p, infinity, cst, viol);
    }

    int best_replica(double infinity, int32_t* replica, double* cst, int64_t* viol) override {
        if (single) {
            if (replica) *replica = 0;
            return eval_cost(nullptr, infinity, cst, viol);
        }
        return rh.best_current(g, cur.p, infinity, replica, cst, viol);
    }
};

}  // namespace mgm2

struct mxs_mgm2 {
    mgm2::Base* impl;
};

extern "C" {

int mxs_mgm2_create(const mxs_graph* g, const mxs_params* p, const int32_t* name_rank, double threshold, int32_t favor,
                    uint64_t seed, int32_t device, mxs_mgm2** out) {
    return mxs_host::create<mxs_mgm2, mgm2::Engine>(g, p, out, name_rank, threshold, favor, (const uint64_t*)&seed, 1, true,
                                                    device);
}
int mxs_mgm2_create_replicas(const mxs_graph* g, const mxs_params* p, const int32_t* name_rank, double threshold,
                             int32_t favor, const uint64_t* seeds, int32_t n_replicas, int32_t device, mxs_mgm2** out) {
    return mxs_host::create<mxs_mgm2, mgm2::Engine>(g, p, out, name_rank, threshold, favor, seeds, n_replicas, false, device);
}
int mxs_mgm2_replicas(const mxs_mgm2* e, int32_t* n) {
    if (!e) return mxs_host::fail(MXS_E_INVALID, "null handle");
    if (n) *n = e->impl->n_rep;
    return MXS_OK;
}
int mxs_mgm2_reset(mxs_mgm2* e) { return e ? e->impl->reset() : mxs_host::fail(MXS_E_INVALID, "null handle"); }
int mxs_mgm2_run(mxs_mgm2* e, int32_t n_rounds) {
    if (!e) return mxs_host::fail(MXS_E_INVALID, "null handle");
    if (n_rounds < 0) return mxs_host::fail(MXS_E_INVALID, "negative round count");
    return e->impl->run(n_rounds);
}
int mxs_mgm2_rounds(const mxs_mgm2* e, int64_t* rounds) {
    if (!e) return mxs_host::fail(MXS_E_INVALID, "null handle");
    if (rounds) *rounds = e->impl->rounds;
    return MXS_OK;
}
int mxs_mgm2_get_state(mxs_mgm2* e, int32_t* idx, double* cost, uint8_t* has_cost) {
    return e ? e->impl->get_state(0, idx, cost, has_cost) : mxs_host::fail(MXS_E_INVALID, "null handle");
}
int mxs_mgm2_get_state_replica(mxs_mgm2* e, int32_t replica, int32_t* idx, double* cost, uint8_t* has_cost) {
    return e ? e->impl->get_state(replica, idx, cost, has_cost) : mxs_host::fail(MXS_E_INVALID, "null handle");
}
int mxs_mgm2_replica_costs(mxs_mgm2* e, double infinity, double* cost, int64_t* violations) {
    return e ? e->impl->replica_costs(infinity, cost, violations) : mxs_host::fail(MXS_E_INVALID, "null handle");
}
int mxs_mgm2_best_replica(mxs_mgm2* e, double infinity, int32_t* replica, double* cost, int64_t* violations) {
    return e ? e->impl->best_replica(infinity, replica, cost, violations) : mxs_host::fail(MXS_E_INVALID, "null handle");
}
int mxs_mgm2_eval_cost(mxs_mgm2* e, const int32_t* idx, double infinity, double* cost, int64_t* violations) {
    return e ? e->impl->eval_cost(idx, infinity, cost, violations) : mxs_host::fail(MXS_E_INVALID, "null handle");
}
int mxs_mgm2_destroy(mxs_mgm2* e) {
    if (e) {
        delete e->impl;
        delete e;
    }
    return MXS_OK;
}

}  // extern "C"
