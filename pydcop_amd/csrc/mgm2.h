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
__global__ void __launch_bounds__(TPB) k_mgm2_value(Dev<T> g) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
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
__global__ void __launch_bounds__(OTPB) k_mgm2_offers(Dev<T> g) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
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
__global__ void __launch_bounds__(TPB) k_mgm2_receive(Dev<T> g) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
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
__global__ void __launch_bounds__(TPB) k_mgm2_resolve(Dev<T> g) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
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
__global__ void __launch_bounds__(TPB) k_mgm2_decide(Dev<T> g) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
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

struct Base {
    virtual ~Base() = default;
    virtual int init(const mxs_graph& g, const mxs_params& p, const int32_t* rank, double threshold, int32_t favor,
                     uint64_t seed, int device) = 0;
    virtual int reset() = 0;
    virtual int run(int32_t n) = 0;
    virtual int get_state(int32_t* idx, double* cost, uint8_t* has_cost) = 0;
    virtual int eval_cost(const int32_t* idx, double infinity, double* cost, int64_t* viol) = 0;
    int64_t rounds = 0;
};

template <typename T>
struct Engine : Base {
    int device = 0;
    hipStream_t stream = nullptr;
    Dev<T> g{};
    mxs_host::HostGraph hg;
    std::vector<int32_t> h_nb;
    lsearch::HostSlots hs;
    Buf<int32_t> dom, var_rowptr, has_nb, rank, off_w, ent_var, cur;
    Buf<int64_t> off_off;
    mxs_host::DevSlots sl;
    Buf<T> tables, cost, offer;
    Buf<uint8_t> has_cost, offer_ok;
    Buf<Rec<T>> uni, recv;

    ~Engine() override {
        if (stream) (void)hipStreamDestroy(stream);
    }

    int init(const mxs_graph& G, const mxs_params& p, const int32_t* rk, double threshold, int32_t favor, uint64_t seed,
             int dev) override {
        device = dev;
        if (int rc = mxs_host::open_device(dev, &stream)) return rc;
        if (!(threshold >= 0.0 && threshold <= 1.0)) return fail(MXS_E_INVALID, "threshold must be in [0, 1]");
        if (favor < 0 || favor > 2) return fail(MXS_E_INVALID, "favor must be 0 (unilateral), 1 (no) or 2 (coordinated)");
        if (int rc = hg.load(G, p)) return rc;
        const int nV = hg.nV, nF = hg.nF;
        // max() over NaN gains depends on message arrival in the reference: no defined result
        for (double t : hg.tables)
            if (!std::isfinite(t)) return fail(MXS_E_INVALID, "mgm2: constraint tables must be finite (no inf / NaN entries)");
        if (int rc = hg.load_init(G)) return rc;
        const std::string bad = hs.build(nV, nF, hg.dom, hg.frow, hg.evar, hg.toff, hg.vrow, hg.vedges);
        if (!bad.empty()) return fail(MXS_E_INVALID, bad);
        // neighbours: the other variables of v's constraints (the concerned list holds v itself once)
        h_nb.assign(nV, 0);
        std::vector<int32_t> h_w(nV, 0), h_ent;
        std::vector<int64_t> h_off(nV + 1, 0);
        for (int v = 0; v < nV; ++v) {
            int P = 0;
            for (int k = hs.conc_rowptr[v]; k < hs.conc_rowptr[v + 1]; ++k)
                if (hs.conc_var[k] != v) P = std::max(P, hg.dom[hs.conc_var[k]]);
            h_nb[v] = P > 0;
            h_w[v] = P;
            h_off[v + 1] = h_off[v] + (int64_t)hg.dom[v] * P;
        }
        if (h_off[nV] > INT32_MAX) return fail(MXS_E_INVALID, "mgm2: offer tables larger than 2^31 entries");
        h_ent.resize((size_t)h_off[nV]);
        for (int v = 0; v < nV; ++v)
            for (int64_t i = h_off[v]; i < h_off[v + 1]; ++i) h_ent[(size_t)i] = v;
        std::vector<int32_t> h_rank(nV);
        for (int v = 0; v < nV; ++v) h_rank[v] = rk ? rk[v] : v;
        if (int rc = sl.upload(hs, stream, nullptr, false)) return rc;  // no first-neighbour arrays, no rows
        MXS_TRY(dom.upload(hg.dom, stream));
        MXS_TRY(var_rowptr.upload(hg.vrow, stream));
        MXS_TRY(has_nb.upload(h_nb, stream));
        MXS_TRY(rank.upload(h_rank, stream));
        MXS_TRY(off_w.upload(h_w, stream));
        MXS_TRY(off_off.upload(h_off, stream));
        MXS_TRY(ent_var.upload(h_ent, stream));
        MXS_TRY(tables.upload(mxs_host::narrowed<T>(hg.tables), stream));
        MXS_TRY(cur.alloc(nV));
        MXS_TRY(cost.alloc(nV));
        MXS_TRY(has_cost.alloc(nV));
        MXS_TRY(uni.alloc(nV));
        MXS_TRY(recv.alloc(nV));
        MXS_TRY(offer.alloc((size_t)h_off[nV]));
        MXS_TRY(offer_ok.alloc((size_t)h_off[nV]));
        g.slots = sl.view();
        g.n_vars = nV;
        g.is_max = p.mode == MXS_MODE_MAX;
        g.favor = favor;
        g.threshold = threshold;
        g.seed = seed;
        g.dom = dom.p;
        g.var_rowptr = var_rowptr.p;
        g.has_nb = has_nb.p;
        g.rank = rank.p;
        g.off_off = off_off.p;
        g.off_w = off_w.p;
        g.ent_var = ent_var.p;
        g.n_entries = h_off[nV];
        g.tables = tables.p;
        g.cur = cur.p;
        g.cost = cost.p;
        g.has_cost = has_cost.p;
        g.uni = uni.p;
        g.recv = recv.p;
        g.offer = offer.p;
        g.offer_ok = offer_ok.p;
        return reset();
    }

    // on_start (:460-495): a variable with neighbours takes its initial value or a random one (held cost None);
    // one without neighbours takes a random best value of its own constraints and is finished
    int reset() override {
        MXS_TRY(hipSetDevice(device));
        const int nV = g.n_vars;
        std::vector<int32_t> c0(nV);
        std::vector<T> k0(nV, (T)0);
        std::vector<uint8_t> h0(nV, 0);
        for (int v = 0; v < nV; ++v) {
            const double u = uniform(g.seed, v, 0, D_START);
            if (h_nb[v]) {
                c0[v] = hg.init[v] >= 0 ? hg.init[v] : (int)(u * hg.dom[v]);
                continue;
            }
            std::vector<T> c(hg.dom[v]);
            T best = (T)0;
            int n_best = 0;
            for (int x = 0; x < hg.dom[v]; ++x) {
                T acc = (T)0;
                for (int s = hg.vrow[v]; s < hg.vrow[v + 1]; ++s) acc += (T)hg.tables[hs.base[s] + (int64_t)x * hs.stride_v[s]];
                c[x] = acc;
                if (n_best == 0 || (g.is_max ? best < acc : best > acc)) {
                    best = acc;
                    n_best = 1;
                } else if (best == acc) {
                    ++n_best;
                }
            }
            int k = (int)(u * n_best);
            for (int x = 0; x < hg.dom[v]; ++x)
                if (c[x] == best && k-- == 0) {
                    c0[v] = x;
                    break;
                }
            k0[v] = best;
            h0[v] = 1;
        }
        if (nV) {
            MXS_TRY(hipMemcpyAsync(cur.p, c0.data(), 4 * (size_t)nV, hipMemcpyHostToDevice, stream));
            MXS_TRY(hipMemcpyAsync(cost.p, k0.data(), sizeof(T) * nV, hipMemcpyHostToDevice, stream));
            MXS_TRY(hipMemcpyAsync(has_cost.p, h0.data(), nV, hipMemcpyHostToDevice, stream));
            MXS_TRY(hipStreamSynchronize(stream));
        }
        rounds = 0;
        return MXS_OK;
    }

    int run(int32_t n) override {
        MXS_TRY(hipSetDevice(device));
        const int nV = g.n_vars;
        if (nV == 0) {
            rounds += n > 0 ? n : 0;
            return MXS_OK;
        }
        const dim3 grid((unsigned)((nV + TPB - 1) / TPB)), block(TPB);
        const dim3 ogrid((unsigned)((g.n_entries + OTPB - 1) / OTPB)), oblock(OTPB);
        for (int32_t r = 0; r < n; ++r) {
            g.round = rounds + 1;
            hipLaunchKernelGGL((k_mgm2_value<T>), grid, block, 0, stream, g);
            MXS_TRY(hipGetLastError());
            if (g.n_entries > 0) {
                hipLaunchKernelGGL((k_mgm2_offers<T>), ogrid, oblock, 0, stream, g);
                MXS_TRY(hipGetLastError());
            }
            hipLaunchKernelGGL((k_mgm2_receive<T>), grid, block, 0, stream, g);
            MXS_TRY(hipGetLastError());
            hipLaunchKernelGGL((k_mgm2_resolve<T>), grid, block, 0, stream, g);
            MXS_TRY(hipGetLastError());
            hipLaunchKernelGGL((k_mgm2_decide<T>), grid, block, 0, stream, g);
            MXS_TRY(hipGetLastError());
            rounds += 1;
        }
        MXS_TRY(hipStreamSynchronize(stream));
        return MXS_OK;
    }

    int get_state(int32_t* idx, double* cst, uint8_t* has) override {
        MXS_TRY(hipSetDevice(device));
        const int nV = g.n_vars;
        if (!nV) return MXS_OK;
        std::vector<T> hc(nV);
        std::vector<int32_t> hi(nV);
        std::vector<uint8_t> hh(nV);
        MXS_TRY(hipMemcpyAsync(hi.data(), cur.p, 4 * (size_t)nV, hipMemcpyDeviceToHost, stream));
        MXS_TRY(hipMemcpyAsync(hh.data(), has_cost.p, nV, hipMemcpyDeviceToHost, stream));
        MXS_TRY(hipMemcpyAsync(hc.data(), cost.p, sizeof(T) * nV, hipMemcpyDeviceToHost, stream));
        MXS_TRY(hipStreamSynchronize(stream));
        for (int v = 0; v < nV; ++v) {
            if (idx) idx[v] = hi[v];
            if (has) has[v] = hh[v];
            if (cst) cst[v] = (double)hc[v];
        }
        return MXS_OK;
    }

    // DCOP.solution_cost of an assignment (the variables' own costs included, unlike the search itself)
    int eval_cost(const int32_t* idx, double infinity, double* cst, int64_t* viol) override {
        std::vector<int32_t> c;
        if (!idx) {
            c.resize(g.n_vars);
            int rc = get_state(c.data(), nullptr, nullptr);
            if (rc) return rc;
            idx = c.data();
        }
        return hg.eval_cost(idx, infinity, cst, viol);
    }
};

}  // namespace mgm2

struct mxs_mgm2 {
    mgm2::Base* impl;
};

extern "C" {

int mxs_mgm2_create(const mxs_graph* g, const mxs_params* p, const int32_t* name_rank, double threshold, int32_t favor,
                    uint64_t seed, int32_t device, mxs_mgm2** out) {
    return mxs_host::create<mxs_mgm2, mgm2::Engine>(g, p, out, name_rank, threshold, favor, seed, device);
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
    return e ? e->impl->get_state(idx, cost, has_cost) : mxs_host::fail(MXS_E_INVALID, "null handle");
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
