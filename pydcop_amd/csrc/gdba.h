// gdba.h -- the reference's GDBA (pydcop/algorithms/gdba.py: Okamoto, Zivan, Nahon 2016) on gfx950, #included at
// the end of mgm.hip (one translation unit for the gfx950 library and for the serial emulated build of
// tests/emu).  The semantics restated here expression by expression, quirks included, are listed with the
// reference's line numbers in tests/gdba_oracle.py, which this file follows bit for bit.
//
// Both phases of GdbaComputation wait for all neighbours and park early messages, so a round is
// bulk-synchronous: two launches per round, each reading what the previous one wrote.
//   k_gdba_eval    the modified cost of every value in the reference's constraint order (compute_eval_value,
//                  :428-461), the cost and the violated constraints at the current value, the best values, the
//                  improvement and the keyed choice of the new value                      (ok phase, :352-387)
//   k_gdba_decide  maxi / max_list over the neighbourhood by name rank, the move -- or, where nobody can
//                  improve, the increase of the violated constraints' modifiers      (improve phase, :493-541)
// The modifiers are the new traffic: one table per (variable, constraint) SLOT, integer counters above a base of
// 0 (`modifier: A`, cost + m) or 1 (`M`, cost * m).  The reference looks a modifier up under the assignment
// filtered to the constraint's scope but, in modes E, R and C, writes it under the assignment of ALL neighbours:
// an increase is read back only where the scope is {v} + neighbours(v).  The host plan marks those slots LIVE and
// stores tables (in the layout of the constraint's table) for them alone; mode T adds 1 to every entry of the
// constraint's own table, always live: one counter per slot.  The increase runs a wave at a time: the lanes of a
// wave take the entries of one stuck variable's row (R) or slab (C) side by side.
// Counters are 16 bits wide: a counter grows by at most 1 per round, and run() refuses to go past 65535 rounds.
//
// REPLICAS (mxs_gdba_create_replicas): R seeded runs advance with the same two launches, as in mgm2.h.  The two
// phases are __device__ bodies (eval_phase, decide_phase) with two sets of __global__ entry points and ONE host
// engine: k_gdba_* on the plain Dev -- what an engine of mxs_gdba_create launches for its one replica, argument layout
// and grid as a single run has always had them -- and k_gdbar_* on DevR, where the replica is folded into blockIdx.x
// (block = r * bpr + b, replica_cost.h) and the block's copy of the argument moves
// once to replica r's slices of the dynamic state and takes seeds[r] (enter_replica).  A block is one wave of ONE
// replica, so the ballot / shuffle loop of the decide phase never mixes replicas.  Everything static is stored once;
// the state is [R][n_vars] in GRAPH order, viol / slot_vc [R][n_slots], the modifier pool [R][plan.entries] (mod_off
// stays per slot).  The start state is drawn on the device (k_gdbar_init).  A GDBA run is not monotone -- the breakout
// makes the assignment wander -- so the best state every replica has shown is kept on the device: the solution costs
// are reduced by replica_cost.h's kernels and its k_best_copy takes the snapshot; the refusals, the allocations that
// grow with R, the cost launches and the records of the best state (rephost::BestTracker) are replica_host.h's.
#pragma once

namespace gdba {

using mxs_host::Buf;
using mxs_host::fail;
using mxs_host::uniform;

constexpr int TPB = 64;  // one wave per block, as mgm2.h: 100k variables spread over every CU
constexpr int64_t MAX_ROUNDS = 65535;
constexpr int64_t DEFAULT_POOL_BUDGET = (int64_t)4 << 30;
// draw ids (the table in engine_common.h): 6 start value (cycle 0), 7 one of the best values
enum { D_START = 6, D_BEST = 7 };
enum { MOD_A = 0, MOD_M = 1 };
enum { VIO_NZ = 0, VIO_NM = 1, VIO_MX = 2 };
enum { INC_E = 0, INC_R = 1, INC_C = 2, INC_T = 3 };

typedef uint16_t counter_t;

template <typename T>
struct alignas(8) Rec {  // what the ok phase leaves for the improve phase
    T improve;           // _my_improve
    int32_t newv;        // _new_value
};

template <typename T>
struct Dev {
    int32_t n_vars, is_max, modifier, violation, increase_mode, has_var_cost;
    uint64_t seed;
    int64_t round;                  // the reference's cycle_count during the round (1, 2, ...)
    const int32_t *dom, *var_rowptr, *has_nb, *rank;
    const T* tables;
    const T* vref;                  // [n_slots] what a raw entry is compared with: 0 (NZ), the table's min (NM), max (MX)
    const int64_t* mod_off;         // [n_slots] the slot's counters in the pool, -1: none stored (dead in E, R, C)
    counter_t* pool;
    const int32_t* conc_first;      // per entry of conc_var: the first slot (position in v's list) that holds it
    const int64_t* cost_off;
    const T* var_cost;
    lsearch::Slots slots;           // base, stride_v, nb_rowptr / nb_var / nb_stride, conc_rowptr / conc_var
    int32_t* cur;
    T* cost;                        // __cost__
    uint8_t* has_cost;
    Rec<T>* rec;
    uint8_t* viol;                  // [n_slots] violated at the current value (round r's ok phase)
    T* slot_vc;                     // [n_slots] vars_cost after the slot, this round (written and read by the owner only)
};

// what the replica engine's kernels take: Dev plus the replicas.  The single-run kernels keep the plain Dev, i.e.
// their argument layout.  The per-replica arrays of Dev -- cur, cost, has_cost, rec -- are [replicas][n_vars], viol and
// slot_vc [replicas][n_slots], pool [replicas][n_pool]; `seed` is filled per block from seeds[r] (enter_replica).
template <typename T>
struct DevR : Dev<T> {
    int32_t bpr;               // blocks per replica of the launch being made (block = replica * bpr + b)
    int32_t n_rep;
    int64_t n_slots, n_pool;   // a replica's share of viol / slot_vc and of the pool
    const uint64_t* seeds;     // [replicas]
    // what k_cost_partial (replica_cost.h) reads of its G: the constraints' CSR and q, here the identity -- the
    // state is in graph order
    const int32_t *dom_size, *factor_rowptr, *edge_var, *q;
    const int64_t* table_off;
};

// the replica of this block: the block's copy of DevR (kernel arguments, block-uniform) moves to the replica's slices
// of the dynamic state and takes its seed, so that nothing below knows about replicas
template <typename T>
__device__ inline int enter_replica(DevR<T>& g, int* b) {
    const int r = repcost::replica_of_block<true>(g, b);
    const int64_t off = (int64_t)r * g.n_vars, soff = (int64_t)r * g.n_slots;
    g.cur += off, g.cost += off, g.has_cost += off, g.rec += off;
    g.viol += soff;
    if (g.has_var_cost) g.slot_vc += soff;
    g.pool += (int64_t)r * g.n_pool;
    g.seed = g.seeds[r];
    return r;
}

// the offset the OTHER scope variables' current values contribute to the slot's table index
template <typename T>
__device__ inline int64_t others_offset(const Dev<T>& g, int s) {
    int64_t off = 0;
    for (int k = g.slots.nb_rowptr[s]; k < g.slots.nb_rowptr[s + 1]; ++k)
        off += (int64_t)g.cur[g.slots.nb_var[k]] * g.slots.nb_stride[k];
    return off;
}

// vars_cost after slot position `pos` of v (:443-459): cost_for_val, from 0, of the owner and of every variable
// of the constraints seen so far, each at its current value, in ascending index
template <typename T>
__device__ inline T vars_cost(const Dev<T>& g, int v, int pos) {
    T acc = (T)0;
    for (int k = g.slots.conc_rowptr[v]; k < g.slots.conc_rowptr[v + 1]; ++k)
        if (g.conc_first[k] <= pos) {
            const int u = g.slots.conc_var[k];
            acc += g.var_cost[g.cost_off[u] + g.cur[u]];
        }
    return acc;
}

// compute_eval_value(x): from 0, over v's constraints in order, += eff_cost, += vars_cost.  mark: also write
// the violated bit of every slot (the caller passes the current value)
template <typename T>
__device__ inline T eval_at(const Dev<T>& g, int v, int x, bool mark) {
    T acc = (T)0;
    const int s0 = g.var_rowptr[v], s1 = g.var_rowptr[v + 1];
    for (int s = s0; s < s1; ++s) {
        const int64_t idx = (int64_t)x * g.slots.stride_v[s] + others_offset(g, s);
        const T tv = g.tables[g.slots.base[s] + idx];
        const int64_t mo = g.mod_off[s];
        int m = g.modifier;  // the base: 0 (A), 1 (M)
        if (mo >= 0) m += (int)g.pool[g.increase_mode == INC_T ? mo : mo + idx];
        acc += g.modifier == MOD_M ? tv * (T)m : tv + (T)m;
        if (g.has_var_cost) acc += g.slot_vc[s];
        if (mark) g.viol[s] = g.violation == VIO_MX ? tv == g.vref[s] : tv != g.vref[s];
    }
    return acc;
}

template <typename T>
__device__ __forceinline__ void eval_phase(const Dev<T>& g, const int v) {
    if (v >= g.n_vars || !g.has_nb[v]) return;
    const int D = g.dom[v], cv = g.cur[v];
    // vars_cost does not depend on the candidate value: once per slot and round, not once per (value, slot)
    if (g.has_var_cost)
        for (int s = g.var_rowptr[v]; s < g.var_rowptr[v + 1]; ++s) g.slot_vc[s] = vars_cost(g, v, s - g.var_rowptr[v]);
    const T cost = eval_at(g, v, cv, true);
    // _compute_best_improvement: strictly better starts a new list, equal joins it (domain order)
    T best = (T)0;
    int n_best = 0;
    for (int x = 0; x < D; ++x) {
        const T c = x == cv ? cost : eval_at(g, v, x, false);
        if (n_best == 0 || (g.is_max ? c > best : c < best)) {
            best = c;
            n_best = 1;
        } else if (c == best) {
            ++n_best;
        }
    }
    Rec<T> r;
    r.improve = cost - best;
    r.newv = cv;
    if (g.is_max ? r.improve < (T)0 : r.improve > (T)0) {
        int k = (int)(uniform(g.seed, v, g.round, D_BEST) * n_best);
        for (int x = 0; x < D; ++x) {
            const T c = x == cv ? cost : eval_at(g, v, x, false);
            if (c == best && k-- == 0) {
                r.newv = x;
                break;
            }
        }
    }
    g.cost[v] = cost;
    g.has_cost[v] = 1;
    g.rec[v] = r;
}

// _increase_cost of every violated constraint of variable w (at value cw), by the 64 lanes of a wave together.
// Every lane reads the same slot records (one broadcast request each); the entries are spread over the lanes.
template <typename T>
__device__ inline void increase_violated(const Dev<T>& g, int w, int cw, int lane) {
    const int Dw = g.dom[w];
    for (int s = g.var_rowptr[w]; s < g.var_rowptr[w + 1]; ++s) {
        if (!g.viol[s]) continue;
        const int64_t mo = g.mod_off[s];
        if (mo < 0) continue;  // no look-up ever reads what the reference writes here
        if (g.increase_mode == INC_T) {
            if (lane == 0) g.pool[mo] = (counter_t)(g.pool[mo] + 1);
            continue;
        }
        const int64_t sv = g.slots.stride_v[s];
        if (g.increase_mode == INC_E) {
            const int64_t i = mo + (int64_t)cw * sv + others_offset(g, s);
            if (lane == 0) g.pool[i] = (counter_t)(g.pool[i] + 1);
        } else if (g.increase_mode == INC_R) {  // every value of w, the neighbours as they are: one strided row
            const int64_t b = mo + others_offset(g, s);
            for (int x = lane; x < Dw; x += 64) g.pool[b + x * sv] = (counter_t)(g.pool[b + x * sv] + 1);
        } else {  // C: every assignment of the neighbours, w as it is: a slab of size / D_w entries
            const int k0 = g.slots.nb_rowptr[s], k1 = g.slots.nb_rowptr[s + 1];
            int64_t n = 1;
            for (int k = k0; k < k1; ++k) n *= g.dom[g.slots.nb_var[k]];
            const int64_t b = mo + (int64_t)cw * sv;
            for (int64_t e = lane; e < n; e += 64) {
                int64_t rest = e, i = b;
                for (int k = k0; k < k1; ++k) {
                    const int d = g.dom[g.slots.nb_var[k]];
                    i += (rest % d) * g.slots.nb_stride[k];
                    rest /= d;
                }
                g.pool[i] = (counter_t)(g.pool[i] + 1);
            }
        }
    }
}

// (every lane of the wave comes here, the ones past n_vars too: the ballot below is the wave's)
template <typename T>
__device__ __forceinline__ void decide_phase(const Dev<T>& g, const int v) {
    const int lane = threadIdx.x & 63;
    const bool plays = v < g.n_vars && g.has_nb[v];
    bool stuck = false;
    int cv = 0;
    if (plays) {
        const Rec<T> me = g.rec[v];
        cv = g.cur[v];
        // maxi and max_list with > and == in both modes (:506-513); sorted(max_list)[0] is v's own name iff no
        // neighbour improves more and none that improves as much has a smaller name
        const int myrank = g.rank[v];
        T maxi = me.improve;
        bool wins = true;
        for (int k = g.slots.conc_rowptr[v]; k < g.slots.conc_rowptr[v + 1]; ++k) {
            const int u = g.slots.conc_var[k];
            if (u == v) continue;
            const T gu = g.rec[u].improve;
            if (gu > maxi) {
                maxi = gu;
                wins = false;
            } else if (gu == maxi && g.rank[u] < myrank) {
                wins = false;
            }
        }
        if (g.is_max ? me.improve < (T)0 : me.improve > (T)0) {
            if (wins) {  // value_selection(_new_value, current_cost + _my_improve), as written (:521-523)
                g.cur[v] = me.newv;
                g.cost[v] = g.cost[v] + me.improve;
            }
        } else if (maxi == (T)0) {
            stuck = true;
        }
    }
    // A stuck variable's neighbours improve by at most 0 where they would need more (min) or improve less than
    // it where the least improving one moves (max): none of them moves this round, so the values read below are
    // those of the round's ok phase, as in the reference.
    unsigned long long todo = __ballot(stuck);
    while (todo) {
        const int src = __builtin_ctzll(todo);
        todo &= todo - 1;
        const int w = __shfl(v, src, 64), cw = __shfl(cv, src, 64);
        increase_violated(g, w, cw, lane);
    }
}

// ---- the entry points.  The single-run kernels: the plain Dev, the thread's index from blockIdx.x alone -- what
// mxs_gdba_create has always launched.
template <typename T>
__global__ void __launch_bounds__(TPB) k_gdba_eval(Dev<T> g) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    eval_phase(g, v);
}
template <typename T>
__global__ void __launch_bounds__(TPB) k_gdba_decide(Dev<T> g) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    decide_phase(g, v);
}

// The replica kernels (mxs_gdba_create_replicas): R runs per launch, whole blocks (one wave each) belong to one
// replica (block = r * bpr + b); below enter_replica the phase code is the single run's.
template <typename T>
__global__ void __launch_bounds__(TPB) k_gdbar_eval(DevR<T> g) {
    int b;
    enter_replica(g, &b);
    eval_phase<T>(g, b * (int)blockDim.x + (int)threadIdx.x);
}
template <typename T>
__global__ void __launch_bounds__(TPB) k_gdbar_decide(DevR<T> g) {
    int b;
    enter_replica(g, &b);
    decide_phase<T>(g, b * (int)blockDim.x + (int)threadIdx.x);
}

// the start state of every replica (on_start, :302-333), thread per (replica, variable): a variable with neighbours
// keeps its initial value (the same in every replica) or takes int(u * D_v), u: draw D_START of cycle 0 under
// seeds[r]; one without takes iso_val / iso_cost (optimal_cost_value, replica_host.h's start_values) and holds
// that cost.  The pool and viol are cleared by the host's memsets.
constexpr int AUX_TPB = rephost::AUX_TPB;
template <typename T>
__global__ void __launch_bounds__(AUX_TPB) k_gdbar_init(DevR<T> g, const int32_t* init, const int32_t* iso_val,
                                                        const T* iso_cost) {
    int b;
    enter_replica(g, &b);
    const int v = b * (int)blockDim.x + (int)threadIdx.x;
    if (v >= g.n_vars) return;
    const int iso = iso_val[v];
    int x = iso;
    if (iso < 0) x = init[v] >= 0 ? init[v] : (int)(uniform(g.seed, v, 0, D_START) * g.dom[v]);
    g.cur[v] = x;
    g.cost[v] = iso >= 0 ? iso_cost[v] : (T)0;
    g.has_cost[v] = iso >= 0 ? 1 : 0;
    Rec<T> r;
    r.improve = (T)0;
    r.newv = x;
    g.rec[v] = r;
}

// The host plan of the modifier pool: which slots are live, where their counters start, how many there are
struct Plan {
    std::vector<int64_t> mod_off, size;  // per slot: offset (-1: none) and number of counters
    int64_t entries = 0;
    void build(int increase_mode, const std::vector<int32_t>& dom, const std::vector<int32_t>& vrow,
               const std::vector<int32_t>& has_nb, const lsearch::HostSlots& hs) {
        const int nV = (int)dom.size();
        const size_t nS = hs.base.size();
        mod_off.assign(nS, -1);
        size.assign(nS, 0);
        entries = 0;
        std::vector<int32_t> seen;
        for (int v = 0; v < nV; ++v) {
            if (!has_nb[v]) continue;  // never plays
            const int n_conc = hs.conc_rowptr[v + 1] - hs.conc_rowptr[v];
            for (int s = vrow[v]; s < vrow[v + 1]; ++s) {
                int64_t n = 1;
                if (increase_mode != INC_T) {  // live: the scope is {v} + every neighbour of v
                    seen.assign(hs.nb_var.begin() + hs.nb_rowptr[s], hs.nb_var.begin() + hs.nb_rowptr[s + 1]);
                    std::sort(seen.begin(), seen.end());
                    seen.erase(std::unique(seen.begin(), seen.end()), seen.end());
                    if ((int)seen.size() != n_conc - 1) continue;
                    // the size of the constraint's table (v may hold several positions of the scope)
                    n = (int64_t)hs.stride_v[s] * (dom[v] - 1) + 1;
                    for (int k = hs.nb_rowptr[s]; k < hs.nb_rowptr[s + 1]; ++k)
                        n += (int64_t)hs.nb_stride[k] * (dom[hs.nb_var[k]] - 1);
                }
                mod_off[s] = entries;
                size[s] = n;
                entries += n;
            }
        }
    }
};

// ---- the host side
inline int check_params(int32_t modifier, int32_t violation, int32_t increase_mode, int64_t* budget) {
    if (modifier < 0 || modifier > 1) return fail(MXS_E_INVALID, "gdba: modifier must be 0 (A) or 1 (M)");
    if (violation < 0 || violation > 2) return fail(MXS_E_INVALID, "gdba: violation must be 0 (NZ), 1 (NM) or 2 (MX)");
    if (increase_mode < 0 || increase_mode > 3)
        return fail(MXS_E_INVALID, "gdba: increase_mode must be 0 (E), 1 (R), 2 (C) or 3 (T)");
    if (*budget < 0) return fail(MXS_E_INVALID, "gdba: negative pool budget");
    if (*budget == 0) *budget = DEFAULT_POOL_BUDGET;
    return MXS_OK;
}

// after hg.load: no empty table, finite tables and variable costs; any_vc: some variable cost is non-zero
inline int check_graph(const mxs_host::HostGraph& hg, bool* any_vc) {
    for (int f = 0; f < hg.nF; ++f)
        if (hg.toff[f + 1] <= hg.toff[f]) return fail(MXS_E_INVALID, "empty table");
    // maxi over NaN improvements depends on message arrival in the reference: no defined result
    for (double t : hg.tables)
        if (!std::isfinite(t)) return fail(MXS_E_INVALID, "gdba: constraint tables must be finite (no inf / NaN entries)");
    *any_vc = false;
    for (double c : hg.var_cost) {
        if (!std::isfinite(c)) return fail(MXS_E_INVALID, "gdba: variable costs must be finite (no inf / NaN entries)");
        *any_vc |= c != 0.0;
    }
    return MXS_OK;
}

// neighbours: the other variables of v's constraints (the concerned list holds v itself once); the first slot of
// v's list that holds each concerned variable (v itself: slot 0, every scope holds it)
inline void neighbourhood(const mxs_host::HostGraph& hg, const lsearch::HostSlots& hs, std::vector<int32_t>& h_nb,
                          std::vector<int32_t>& h_first) {
    const int nV = hg.nV;
    h_nb.assign(nV, 0);
    h_first.assign(hs.conc_var.size(), 0);
    for (int v = 0; v < nV; ++v) {
        const int c0 = hs.conc_rowptr[v], c1 = hs.conc_rowptr[v + 1];
        h_nb[v] = c1 - c0 > 1;
        for (int k = c0; k < c1; ++k) {
            const int u = hs.conc_var[k];
            int first = 0;
            if (u != v)
                for (int s = hg.vrow[v]; s < hg.vrow[v + 1]; ++s) {
                    bool in = false;
                    for (int q = hs.nb_rowptr[s]; q < hs.nb_rowptr[s + 1]; ++q) in |= hs.nb_var[q] == u;
                    if (in) {
                        first = s - hg.vrow[v];
                        break;
                    }
                }
            h_first[k] = first;
        }
    }
}

// what a raw entry is compared with (_is_violated, :552-572), per slot: 0 (NZ), min / max over the flattened table
template <typename T>
std::vector<T> violation_refs(const mxs_host::HostGraph& hg, size_t n_slots, int32_t violation) {
    std::vector<T> h_vref(n_slots, (T)0);
    if (violation == VIO_NZ) return h_vref;
    std::vector<T> fref(hg.nF);
    for (int f = 0; f < hg.nF; ++f) {
        T r = (T)hg.tables[hg.toff[f]];
        for (int64_t i = hg.toff[f]; i < hg.toff[f + 1]; ++i) {
            const T t = (T)hg.tables[i];
            if (violation == VIO_NM ? t < r : t > r) r = t;
        }
        fref[f] = r;
    }
    for (size_t s = 0; s < n_slots; ++s) h_vref[s] = fref[hg.efac[hg.vedges[s]]];
    return h_vref;
}

// Engine<T> behind struct mxs_gdba, whatever its T
struct Base {
    virtual ~Base() = default;
    virtual int init(const mxs_graph& G, const mxs_params& p, const int32_t* name_rank, const int32_t* value_rank,
                     int32_t modifier, int32_t violation, int32_t increase_mode, const uint64_t* seeds, int32_t n_replicas,
                     bool single, int64_t budget, int dev) = 0;
    virtual int reset() = 0;
    virtual int run(int32_t n) = 0;
    virtual int get_state(int32_t r, int32_t* idx, double* cost, uint8_t* has_cost, double* improve, int32_t* newv) = 0;
    virtual int get_modifiers(int32_t r, int32_t slot, int32_t* out, int64_t capacity, int64_t* n) = 0;
    virtual int eval_cost(const int32_t* idx, double infinity, double* cost, int64_t* viol) = 0;
    virtual int replica_costs(double infinity, double* cost, int64_t* viol) = 0;
    virtual int track_best(int32_t every, double infinity) = 0;
    virtual int get_best(int32_t r, int32_t* replica, int64_t* round, double* cost, int64_t* viol, int32_t* idx) = 0;
    int64_t rounds = 0;
    int32_t n_rep = 1;
};

// The one host engine: R >= 1 seeded runs of the instance with the launches one run needs.  The slot view, the
// tables, vref, mod_off, conc_first, dom, rank and the variable costs are stored once; cur, cost, has_cost, rec are
// [R][n_vars], viol (and slot_vc where some variable cost is non-zero) [R][n_slots], the pool [R][plan.entries]; the
// seeds are a device array.  The refusals, the allocations that grow with R, the start values of the variables
// without neighbours and the cost launches are rephost::Host's (replica_host.h, shared with dsa.hip, mgm.hip and
// mgm2.h); GDBA keeps its variables in graph order, so Host's q is the identity (graph_order).  A run's final state
// is usually not its best: track_best keeps every replica's best state on the device, as DSA's does.
// `single` (mxs_gdba_create): one replica under seeds = {seed} whose rounds are launched through the plain entry
// points on the Dev base of g -- replica 0's slices are the buffers' bases.  It keeps the single run's API: its
// replica cost is the host's eval_cost, it tracks no best state, and its budget refusal names no replicas.
template <typename T>
struct Engine : Base {
    rephost::Host<T> rh;
    DevR<T> g{};
    bool single = false;
    Plan plan;
    mxs_host::DevSlots sl;
    size_t n_slots = 0;
    Buf<int32_t> rank, conc_first, init_idx;
    Buf<int64_t> mod_off;
    Buf<T> vref, var_cost;
    Buf<int32_t> cur;                 // the dynamic state: [R][n_vars], graph order
    Buf<T> cost, slot_vc;
    Buf<counter_t> pool;
    Buf<uint8_t> has_cost, viol;
    Buf<Rec<T>> rec;
    rephost::BestTracker<T> bt;       // the best state every replica has shown (track_best, get_best)

    int init(const mxs_graph& G, const mxs_params& p, const int32_t* rk, const int32_t* vrk, int32_t modifier,
             int32_t violation, int32_t increase_mode, const uint64_t* sds, int32_t n_replicas, bool one_run,
             int64_t budget, int dev) override {
        single = one_run;
        if (int rc = rh.open(sds, n_replicas, dev, true)) return rc;
        n_rep = rh.n_rep;
        if (int rc = check_params(modifier, violation, increase_mode, &budget)) return rc;
        if (int rc = rh.hg.load(G, p)) return rc;
        bool any_vc = false;
        if (int rc = check_graph(rh.hg, &any_vc)) return rc;
        if (int rc = rh.hg.load_init(G)) return rc;
        rh.set_value_rank(vrk);
        const mxs_host::HostGraph& hg = rh.hg;
        const hipStream_t stream = rh.stream;
        const int nV = hg.nV;
        lsearch::HostSlots hs;
        const std::string bad = hs.build(nV, hg.nF, hg.dom, hg.frow, hg.evar, hg.toff, hg.vrow, hg.vedges);
        if (!bad.empty()) return fail(MXS_E_INVALID, bad);
        std::vector<int32_t> h_nb, h_first;
        neighbourhood(hg, hs, h_nb, h_first);
        // the plan of ONE replica's pool; all of them against the budget before anything is allocated
        plan.build(increase_mode, hg.dom, hg.vrow, h_nb, hs);
        const int64_t one = plan.entries * (int64_t)sizeof(counter_t);
        if (plan.entries > budget / (int64_t)sizeof(counter_t) / n_rep)
            return fail(MXS_E_INVALID,
                        (single ? "gdba: the modifier tables take " + std::to_string(one) + " bytes"
                                : "gdba: the modifier tables of " + std::to_string(n_rep) + " replicas take " +
                                      std::to_string(one * n_rep) + " bytes (" + std::to_string(one) + " per replica)") +
                            ", more than the budget of " + std::to_string(budget));
        if (int rc = rh.graph_order(h_nb, rephost::blocks_of(nV, TPB))) return rc;
        n_slots = hs.base.size();
        if (int rc = sl.upload(hs, stream, nullptr, false)) return rc;  // no first-neighbour arrays, no rows
        if (int rc = rh.upload_order()) return rc;
        if (int rc = rh.upload_graph()) return rc;
        MXS_TRY(conc_first.upload(h_first, stream));
        MXS_TRY(rank.upload(mgm2::ranks_or_index(rk, nV), stream));
        MXS_TRY(vref.upload(violation_refs<T>(hg, n_slots, violation), stream));
        MXS_TRY(var_cost.upload(mxs_host::narrowed<T>(hg.var_cost), stream));
        MXS_TRY(mod_off.upload(plan.mod_off, stream));
        MXS_TRY(init_idx.upload(hg.init, stream));
        const size_t R = (size_t)n_rep;
        if (int rc = rephost::alloc_rep(pool, R * (size_t)plan.entries, "modifier tables")) return rc;
        if (int rc = rephost::alloc_rep(cur, R * nV, "values")) return rc;
        if (int rc = rephost::alloc_rep(cost, R * nV, "held costs")) return rc;
        if (int rc = rephost::alloc_rep(has_cost, R * nV, "cost flags")) return rc;
        if (int rc = rephost::alloc_rep(rec, R * nV, "improvement records")) return rc;
        if (int rc = rephost::alloc_rep(viol, R * n_slots, "violation flags")) return rc;
        if (int rc = rephost::alloc_rep(slot_vc, any_vc ? R * n_slots : 0, "variable-cost sums")) return rc;
        g.modifier = modifier;
        g.violation = violation;
        g.increase_mode = increase_mode;
        g.has_var_cost = any_vc;
        bind();
        return reset();
    }

    // the kernels' argument: the Dev part, the per-replica arrays at their bases (replica 0's slices), then DevR's
    void bind() {
        g.slots = sl.view();
        g.n_vars = rh.hg.nV, g.is_max = rh.hg.is_max;
        g.seed = single ? rh.h_seeds[0] : 0;  // the replica kernels: seeds[r], per block
        g.dom = rh.dom_size.p, g.var_rowptr = rh.var_rowptr.p, g.has_nb = rh.n_neigh.p, g.rank = rank.p;
        g.tables = rh.tables.p, g.vref = vref.p, g.mod_off = mod_off.p, g.pool = pool.p;
        g.conc_first = conc_first.p, g.cost_off = rh.cost_off.p, g.var_cost = var_cost.p;
        g.cur = cur.p, g.cost = cost.p, g.has_cost = has_cost.p, g.rec = rec.p, g.viol = viol.p, g.slot_vc = slot_vc.p;
        g.bpr = 1, g.n_rep = n_rep, g.n_slots = (int64_t)n_slots, g.n_pool = plan.entries, g.seeds = rh.seeds.p;
        g.dom_size = rh.dom_size.p, g.factor_rowptr = rh.factor_rowptr.p, g.edge_var = rh.edge_var.p;
        g.q = rh.qmap.p, g.table_off = rh.table_off.p;
    }

    // every replica back to its start state (k_gdbar_init), the pools and the violation flags cleared; the records
    // of track_best start again
    int reset() override {
        if (int rc = rh.start_values()) return rc;  // optimal_cost_value of the variables without neighbours
        const hipStream_t stream = rh.stream;
        const size_t R = (size_t)n_rep;
        rounds = 0;
        if (g.n_vars) {
            g.bpr = rephost::blocks_of(g.n_vars, AUX_TPB);
            hipLaunchKernelGGL((k_gdbar_init<T>), dim3((unsigned)(g.bpr * n_rep)), dim3(AUX_TPB), 0, stream, g,
                               (const int32_t*)init_idx.p, (const int32_t*)rh.iso_val.p, (const T*)rh.iso_cost.p);
            MXS_TRY(hipGetLastError());
        }
        if (plan.entries) MXS_TRY(hipMemsetAsync(pool.p, 0, sizeof(counter_t) * R * (size_t)plan.entries, stream));
        if (n_slots) MXS_TRY(hipMemsetAsync(viol.p, 0, R * n_slots, stream));
        const int rc = bt.on_reset(rh, g, cur.p);
        MXS_TRY(hipStreamSynchronize(stream));  // (also when the record failed)
        return rc;
    }

    int run(int32_t n) override {
        MXS_TRY(hipSetDevice(rh.device));
        if (rounds + (int64_t)n > MAX_ROUNDS)
            return fail(MXS_E_INVALID, "gdba: the modifier counters are 16 bits wide, at most 65535 rounds");
        const hipStream_t stream = rh.stream;
        const int nV = g.n_vars;
        if (nV == 0) {
            rounds += n;
            return MXS_OK;
        }
        const int vbpr = rephost::blocks_of(nV, TPB);
        const dim3 grid((unsigned)vbpr * (unsigned)n_rep), block(TPB);
        const Dev<T>& one = g;  // what a single run's launches copy: the Dev part
        for (int32_t r = 0; r < n; ++r) {
            g.round = rounds + 1;
            g.bpr = vbpr;  // (a kernel takes its argument by value: the copy is made at the launch; the record sets its own)
            if (single) {
                hipLaunchKernelGGL((k_gdba_eval<T>), grid, block, 0, stream, one);
                MXS_TRY(hipGetLastError());
                hipLaunchKernelGGL((k_gdba_decide<T>), grid, block, 0, stream, one);
                MXS_TRY(hipGetLastError());
            } else {
                hipLaunchKernelGGL((k_gdbar_eval<T>), grid, block, 0, stream, g);
                MXS_TRY(hipGetLastError());
                hipLaunchKernelGGL((k_gdbar_decide<T>), grid, block, 0, stream, g);
                MXS_TRY(hipGetLastError());
            }
            rounds += 1;
            if (int rc = bt.after_step(rh, g, cur.p, rounds)) return rc;
        }
        MXS_TRY(hipStreamSynchronize(stream));
        return MXS_OK;
    }

    int get_state(int32_t r, int32_t* idx, double* cst, uint8_t* has, double* imp, int32_t* nv) override {
        if (r < 0 || r >= n_rep) return fail(MXS_E_INVALID, "replica out of range");
        MXS_TRY(hipSetDevice(rh.device));
        const hipStream_t stream = rh.stream;
        const int nV = g.n_vars;
        if (!nV) return MXS_OK;
        std::vector<T> hc(nV);
        std::vector<Rec<T>> hr(nV);
        const size_t roff = (size_t)r * nV;
        if (idx) MXS_TRY(hipMemcpyAsync(idx, cur.p + roff, 4 * (size_t)nV, hipMemcpyDeviceToHost, stream));
        if (has) MXS_TRY(hipMemcpyAsync(has, has_cost.p + roff, nV, hipMemcpyDeviceToHost, stream));
        if (cst) MXS_TRY(hipMemcpyAsync(hc.data(), cost.p + roff, sizeof(T) * (size_t)nV, hipMemcpyDeviceToHost, stream));
        if (imp || nv) MXS_TRY(hipMemcpyAsync(hr.data(), rec.p + roff, sizeof(Rec<T>) * (size_t)nV, hipMemcpyDeviceToHost, stream));
        MXS_TRY(hipStreamSynchronize(stream));
        for (int v = 0; v < nV; ++v) {
            if (cst) cst[v] = (double)hc[v];
            if (imp) imp[v] = (double)hr[v].improve;
            if (nv) nv[v] = hr[v].newv;
        }
        return MXS_OK;
    }

    // slot -1: *n = the bytes of the whole pool, all replicas.  Otherwise *n = the number of modifiers stored for the
    // slot (0: none); with `out`, those of replica r are copied (base + counter) -- capacity must hold them
    int get_modifiers(int32_t r, int32_t slot, int32_t* out, int64_t capacity, int64_t* n) override {
        if (r < 0 || r >= n_rep) return fail(MXS_E_INVALID, "replica out of range");
        if (slot == -1) {
            if (n) *n = plan.entries * (int64_t)sizeof(counter_t) * n_rep;
            return MXS_OK;
        }
        if (slot < 0 || (size_t)slot >= plan.size.size()) return fail(MXS_E_INVALID, "gdba: slot out of range");
        const int64_t cnt = plan.size[slot];
        if (n) *n = cnt;
        if (!out || cnt == 0) return MXS_OK;
        if (capacity < cnt) return fail(MXS_E_INVALID, "gdba: buffer too small for the slot's modifiers");
        MXS_TRY(hipSetDevice(rh.device));
        std::vector<counter_t> h((size_t)cnt);
        MXS_TRY(hipMemcpyAsync(h.data(), pool.p + (size_t)r * (size_t)plan.entries + plan.mod_off[slot],
                               sizeof(counter_t) * (size_t)cnt, hipMemcpyDeviceToHost, rh.stream));
        MXS_TRY(hipStreamSynchronize(rh.stream));
        for (int64_t i = 0; i < cnt; ++i) out[i] = g.modifier + (int32_t)h[(size_t)i];
        return MXS_OK;
    }

    int eval_cost(const int32_t* idx, double infinity, double* cst, int64_t* viol_out) override {
        return rh.eval_cost(idx, infinity, cst, viol_out,
                            [&](int32_t* out) { return get_state(0, out, nullptr, nullptr, nullptr, nullptr); });
    }

    // the device's reduction; a single run's cost is eval_cost's (the host's summation order)
    int replica_costs(double infinity, double* cst, int64_t* viol_out) override {
        if (single) return eval_cost(nullptr, infinity, cst, viol_out);
        return rh.replica_costs(g, cur.p, infinity, cst, viol_out);
    }

    // (the best state is kept for mxs_gdba_create_replicas, one replica included)
    int track_best(int32_t ev, double infinity) override {
        if (single) return fail(MXS_E_STATE, "gdba: the best state is tracked by the replica engine");
        return bt.track(rh, g, cur.p, rounds, ev, infinity);
    }

    int get_best(int32_t r, int32_t* replica, int64_t* round, double* cst, int64_t* viol_out, int32_t* idx) override {
        if (single) r = -1;  // (a single run is never tracked -- track_best refuses it -- and answers so whatever r)
        return bt.get(rh, g, cur.p, rounds, r, replica, round, cst, viol_out, idx,
                      [&](int32_t rep, int32_t* out) { return get_state(rep, out, nullptr, nullptr, nullptr, nullptr); },
                      "mxs_gdba");
    }
};

}  // namespace gdba

struct mxs_gdba {
    gdba::Base* impl;
};

extern "C" {

int mxs_gdba_create(const mxs_graph* g, const mxs_params* p, const int32_t* name_rank, const int32_t* value_rank,
                    int32_t modifier, int32_t violation, int32_t increase_mode, uint64_t seed, int64_t pool_budget_bytes,
                    int32_t device, mxs_gdba** out) {
    return mxs_host::create<mxs_gdba, gdba::Engine>(g, p, out, name_rank, value_rank, modifier, violation, increase_mode,
                                                    (const uint64_t*)&seed, 1, true, pool_budget_bytes, device);
}
int mxs_gdba_create_replicas(const mxs_graph* g, const mxs_params* p, const int32_t* name_rank, const int32_t* value_rank,
                             int32_t modifier, int32_t violation, int32_t increase_mode, const uint64_t* seeds,
                             int32_t n_replicas, int64_t pool_budget_bytes, int32_t device, mxs_gdba** out) {
    return mxs_host::create<mxs_gdba, gdba::Engine>(g, p, out, name_rank, value_rank, modifier, violation, increase_mode, seeds,
                                                    n_replicas, false, pool_budget_bytes, device);
}
int mxs_gdba_replicas(const mxs_gdba* e, int32_t* n) {
    if (!e) return mxs_host::fail(MXS_E_INVALID, "null handle");
    if (n) *n = e->impl->n_rep;
    return MXS_OK;
}
int mxs_gdba_reset(mxs_gdba* e) { return e ? e->impl->reset() : mxs_host::fail(MXS_E_INVALID, "null handle"); }
int mxs_gdba_run(mxs_gdba* e, int32_t n_rounds) {
    if (!e) return mxs_host::fail(MXS_E_INVALID, "null handle");
    if (n_rounds < 0) return mxs_host::fail(MXS_E_INVALID, "negative round count");
    return e->impl->run(n_rounds);
}
int mxs_gdba_rounds(const mxs_gdba* e, int64_t* rounds) {
    if (!e) return mxs_host::fail(MXS_E_INVALID, "null handle");
    if (rounds) *rounds = e->impl->rounds;
    return MXS_OK;
}
int mxs_gdba_get_state(mxs_gdba* e, int32_t* idx, double* cost, uint8_t* has_cost, double* improve, int32_t* new_value) {
    return e ? e->impl->get_state(0, idx, cost, has_cost, improve, new_value) : mxs_host::fail(MXS_E_INVALID, "null handle");
}
int mxs_gdba_get_state_replica(mxs_gdba* e, int32_t replica, int32_t* idx, double* cost, uint8_t* has_cost, double* improve,
                               int32_t* new_value) {
    return e ? e->impl->get_state(replica, idx, cost, has_cost, improve, new_value) : mxs_host::fail(MXS_E_INVALID, "null handle");
}
int mxs_gdba_get_modifiers(mxs_gdba* e, int32_t slot, int32_t* out, int64_t capacity, int64_t* n_entries) {
    return e ? e->impl->get_modifiers(0, slot, out, capacity, n_entries) : mxs_host::fail(MXS_E_INVALID, "null handle");
}
int mxs_gdba_get_modifiers_replica(mxs_gdba* e, int32_t replica, int32_t slot, int32_t* out, int64_t capacity,
                                   int64_t* n_entries) {
    return e ? e->impl->get_modifiers(replica, slot, out, capacity, n_entries) : mxs_host::fail(MXS_E_INVALID, "null handle");
}
int mxs_gdba_replica_costs(mxs_gdba* e, double infinity, double* cost, int64_t* violations) {
    return e ? e->impl->replica_costs(infinity, cost, violations) : mxs_host::fail(MXS_E_INVALID, "null handle");
}
int mxs_gdba_track_best(mxs_gdba* e, int32_t every, double infinity) {
    return e ? e->impl->track_best(every, infinity) : mxs_host::fail(MXS_E_INVALID, "null handle");
}
int mxs_gdba_get_best(mxs_gdba* e, int32_t r, int32_t* replica, int64_t* round, double* cost, int64_t* violations,
                      int32_t* idx) {
    return e ? e->impl->get_best(r, replica, round, cost, violations, idx) : mxs_host::fail(MXS_E_INVALID, "null handle");
}
int mxs_gdba_eval_cost(mxs_gdba* e, const int32_t* idx, double infinity, double* cost, int64_t* violations) {
    return e ? e->impl->eval_cost(idx, infinity, cost, violations) : mxs_host::fail(MXS_E_INVALID, "null handle");
}
int mxs_gdba_destroy(mxs_gdba* e) {
    if (e) {
        delete e->impl;
        delete e;
    }
    return MXS_OK;
}

}  // extern "C"
