// replica_host.h -- the host side of an engine that advances R seeded runs of one instance with the same launches
// (dsa.hip, mgm.hip, mgm2.h, gdba.h; the device side is replica_cost.h): what such an engine owns whatever its
// algorithm, and the steps of its life that do not depend on the algorithm.  Host code only: no kernel, no
// kernel-argument layout.  Every one of the four algorithms has ONE host engine on it, a single run being the case
// R = 1.  An engine HOLDS a Host<T> and supplies its Dev (the kernels' argument), its per-lane extras (built from the
// host views between build_views and upload_views), its init kernel (after start_values) and the launches of a cycle.
// It takes from Host the device costs of the current states and their ranking (replica_costs, best_current: what
// MGM's and MGM-2's best_replica is).  An engine whose runs are not monotone (DSA, GDBA) also HOLDS a BestTracker<T>:
// the records of the best state every replica has shown, their allocation, the launches that compare and copy, and
// get_best -- the engine calls it after reset, after every step and from track_best / get_best, passing its live
// values and its step count, and keeps only the refusals that are its own.
// MGM-2 and GDBA bring their own view and keep their state in graph order: they take open, graph_order /
// upload_order in place of build_views / upload_views, upload_graph, alloc_rep and the cost launches, and bind their
// DevR themselves; their mxs_*_create engine launches its one replica through the plain-Dev entry points.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "engine_common.h"
#include "replica_cost.h"

namespace rephost {

using mxs_host::Buf;
using mxs_host::fail;

// the block sizes of the launches that fold the replica into blockIdx.x (the engines assert theirs against these):
// thread per variable, lane per (variable, constraint), init and copy kernels
constexpr int VAR_TPB = 64, PACK_TPB = 256, AUX_TPB = 256;
static_assert(AUX_TPB == repcost::BEST_TPB, "k_best_copy is launched with blocks of AUX_TPB threads");

inline int blocks_of(int64_t n, int per_block) { return (int)((n + per_block - 1) / per_block); }

// an allocation that grows with the number of replicas: its failure is MXS_E_NOMEM (the owner's destructor frees
// what was allocated before)
template <typename U>
int alloc_rep(Buf<U>& b, size_t count, const char* what) {
    if (b.alloc(count) != hipSuccess) {
        (void)hipGetLastError();
        b.p = nullptr;
        b.n = 0;
        return fail(MXS_E_NOMEM, std::string("out of device memory for the replicas' ") + what);
    }
    return MXS_OK;
}

// $MAXSUM_LOCAL_SEARCH_GENERIC (A/B runs, tests) =1: the CSR-walk kernels, =2: the slot kernels for every variable;
// else the packed kernels where the instance has packed lanes
struct KernelChoice {
    bool generic, packed;
};
inline KernelChoice kernel_choice(bool have_pack) {
    const char* env = std::getenv("MAXSUM_LOCAL_SEARCH_GENERIC");
    const bool generic = env && env[0] == '1';
    return {generic, !generic && !(env && env[0] == '2') && have_pack};
}

template <typename T>
struct Host {
    int device = 0;
    hipStream_t stream = nullptr;
    int32_t n_rep = 1;
    std::vector<uint64_t> h_seeds;  // [replicas]; one 0 where the engine draws nothing
    mxs_host::HostGraph hg;
    std::vector<int32_t> h_nn, h_q, h_vrank;  // has neighbours; graph index -> packed position; order of the domains' values
    int max_dom = 0;
    Buf<int32_t> dom_size, factor_rowptr, edge_var, edge_factor, var_rowptr, var_edges, n_neigh, qmap;
    Buf<int64_t> table_off, cost_off;
    Buf<T> tables;
    Buf<uint64_t> seeds;
    mxs_host::DevSlots sl;
    mxs_host::DevPack<T> pk;
    // the start state of the variables without neighbours (the engine's init kernel reads iso_val / iso_cost)
    std::vector<int32_t> h_iso_val;
    std::vector<T> h_iso_cost;
    Buf<int32_t> iso_val;
    Buf<T> iso_cost;
    // the device cost (k_cost_partial / k_cost_final, replica_cost.h)
    Buf<double> evc, part_cost, rep_cost;
    Buf<long long> part_viol, rep_viol;
    int cost_blocks = 1;

    ~Host() {
        if (stream) (void)hipStreamDestroy(stream);
    }

    // the refusals every replica engine makes first, then the device; the engine's own checks and hg.load follow
    int open(const uint64_t* sds, int n_replicas, int dev, bool seeds_required) {
        device = dev;
        if (n_replicas < 1 || n_replicas > repcost::MAX_REPLICAS)
            return fail(MXS_E_INVALID, "the number of replicas must be in 1 .. 4096");
        if (seeds_required && !sds) return fail(MXS_E_INVALID, "null seeds");
        n_rep = n_replicas;
        h_seeds = seeds_required ? std::vector<uint64_t>(sds, sds + n_replicas) : std::vector<uint64_t>(1, 0);
        return mxs_host::open_device(dev, &stream);
    }

    // the host side of the views (after hg.load): who has neighbours, the slot view, the packed view of the variables
    // it can take (local_search.h; the others -- constraints of arity > 2, larger domains, degrees above 64 -- stay
    // on the thread-per-variable kernels), the packed order, and the one refusal of a grid that does not fit
    int build_views(lsearch::HostSlots& hs, lsearch::HostPack& hp) {
        const int nV = hg.nV, nF = hg.nF;
        h_nn.assign(nV, 0);
        for (int f = 0; f < nF; ++f)
            if (hg.frow[f + 1] - hg.frow[f] > 1)
                for (int e = hg.frow[f]; e < hg.frow[f + 1]; ++e) h_nn[hg.evar[e]] = 1;
        const std::string bad = hs.build(nV, nF, hg.dom, hg.frow, hg.evar, hg.toff, hg.vrow, hg.vedges);
        if (!bad.empty()) return fail(MXS_E_INVALID, bad);
        max_dom = 0;
        for (int v = 0; v < nV; ++v) max_dom = hg.dom[v] > max_dom ? hg.dom[v] : max_dom;
        hp.build(nV, hg.dom, hg.vrow, h_nn, hs, hg.tables);
        h_q = mxs_host::packed_order(hp, nV);
        return fit_grids(std::max<int64_t>(blocks_of((int64_t)hp.nb.size(), PACK_TPB), blocks_of(nV, VAR_TPB)));
    }

    // the same step of an engine that brings its own view and keeps its state in GRAPH order (mgm2.h): who has
    // neighbours is the engine's, q is the identity, there is no packed view; most_blocks: the blocks of its largest
    // launch for ONE replica
    int graph_order(const std::vector<int32_t>& has_neighbours, int64_t most_blocks) {
        const int nV = hg.nV;
        h_nn = has_neighbours;
        h_q.resize(nV);
        for (int v = 0; v < nV; ++v) h_q[v] = v;
        max_dom = 0;
        for (int v = 0; v < nV; ++v) max_dom = hg.dom[v] > max_dom ? hg.dom[v] : max_dom;
        return fit_grids(most_blocks);
    }

    // the grid of the cost reduction, and the one refusal: every launch folds the replica into blockIdx.x, the
    // largest grid must fit
    int fit_grids(int64_t most_blocks) {
        cost_blocks = std::max(1, blocks_of((int64_t)hg.nF + hg.nV, repcost::COST_TPB * repcost::COST_RUN));
        const int64_t most = std::max<int64_t>({most_blocks, blocks_of(hg.nV, AUX_TPB), cost_blocks});
        if (most * (int64_t)n_rep > INT32_MAX) return fail(MXS_E_INVALID, "too many replicas for an instance of this size");
        return MXS_OK;
    }

    // graph index -> position in the dynamic state (k_cost_partial reads the values through it)
    int upload_order() {
        MXS_TRY(qmap.upload(h_q, stream));
        return MXS_OK;
    }

    // the views on the device, their variable references as packed positions (the engine has built its per-lane
    // extras from hs / hp / h_q by now: upload_rows releases hs.rows)
    int upload_views(lsearch::HostSlots& hs, const lsearch::HostPack& hp) {
        if (int rc = upload_order()) return rc;
        if (int rc = sl.upload(hs, stream, &h_q, true)) return rc;
        if (int rc = pk.upload(hp, h_q, hg.dom, stream)) return rc;
        sl.upload_rows(hs, hp.rest, hg, max_dom, (int)sizeof(T), stream);
        return MXS_OK;
    }

    // the CSR arrays and the tables (in T), the seeds, eval_var_cost; what holds the start values and the device cost
    int upload_graph() {
        MXS_TRY(dom_size.upload(hg.dom, stream));
        MXS_TRY(factor_rowptr.upload(hg.frow, stream));
        MXS_TRY(edge_var.upload(hg.evar, stream));
        MXS_TRY(edge_factor.upload(hg.efac, stream));
        MXS_TRY(var_rowptr.upload(hg.vrow, stream));
        MXS_TRY(var_edges.upload(hg.vedges, stream));
        MXS_TRY(n_neigh.upload(h_nn, stream));
        MXS_TRY(table_off.upload(hg.toff, stream));
        MXS_TRY(cost_off.upload(hg.coff, stream));
        MXS_TRY(tables.upload(mxs_host::narrowed<T>(hg.tables), stream));
        MXS_TRY(seeds.upload(h_seeds, stream));
        MXS_TRY(evc.upload(hg.eval_var_cost, stream));
        MXS_TRY(iso_val.alloc(hg.nV));
        MXS_TRY(iso_cost.alloc(hg.nV));
        const size_t R = (size_t)n_rep;
        if (int rc = alloc_rep(part_cost, R * cost_blocks, "cost partials")) return rc;
        if (int rc = alloc_rep(part_viol, R * cost_blocks, "cost partials")) return rc;
        if (int rc = alloc_rep(rep_cost, R, "costs")) return rc;
        return alloc_rep(rep_viol, R, "costs");
    }

    // what every engine's Dev G has of the above, under the same names
    template <typename G>
    void bind(G& g) const {
        g.n_vars = hg.nV; g.is_max = hg.is_max; g.seeds = seeds.p;
        g.dom_size = dom_size.p; g.factor_rowptr = factor_rowptr.p; g.edge_var = edge_var.p;
        g.edge_factor = edge_factor.p; g.var_rowptr = var_rowptr.p; g.var_edges = var_edges.p;
        g.n_neigh = n_neigh.p; g.table_off = table_off.p; g.tables = tables.p;
        g.q = qmap.p; g.slots = sl.view(); g.pack = pk.view(); g.pack_dom = pk.dom.p;
    }

    // the order of every variable's domain values (include/maxsum_gpu.h): cost ties of a variable without
    // neighbours break on the value, as the reference's optimal_cost_value does.  The engine resets after it.
    void set_value_rank(const int32_t* rank) {
        if (rank) h_vrank.assign(rank, rank + hg.coff[hg.nV]);
        else h_vrank.clear();
    }

    // the optimal_cost_value of the variables without neighbours and its cost into iso_val / iso_cost (-1: has
    // neighbours), copied on the stream: the engine launches its init kernel after it and synchronises before it returns
    int start_values() {
        MXS_TRY(hipSetDevice(device));
        const int nV = hg.nV;
        h_iso_val.assign(nV, -1);
        h_iso_cost.assign(nV, (T)0);
        for (int v = 0; v < nV; ++v)
            if (h_nn[v] == 0) {
                h_iso_val[v] = hg.optimal_cost_value<T>(v, hg.is_max, h_vrank);
                h_iso_cost[v] = (T)hg.var_cost[hg.coff[v] + h_iso_val[v]];
            }
        if (nV) {
            MXS_TRY(hipMemcpyAsync(iso_val.p, h_iso_val.data(), 4 * (size_t)nV, hipMemcpyHostToDevice, stream));
            MXS_TRY(hipMemcpyAsync(iso_cost.p, h_iso_cost.data(), sizeof(T) * (size_t)nV, hipMemcpyHostToDevice, stream));
        }
        return MXS_OK;
    }

    // packed order (Dev::q) -> graph order
    void unpack(const std::vector<int32_t>& hi, int32_t* idx) const {
        for (int v = 0; v < hg.nV; ++v) idx[v] = hi[h_q[v]];
    }

    // DCOP.solution_cost of `idx`; NULL: of replica 0's current values, which `values_of_replica0(int32_t*)` fetches
    template <typename F>
    int eval_cost(const int32_t* idx, double infinity, double* cst, int64_t* viol, F values_of_replica0) {
        std::vector<int32_t> c;
        if (!idx) {
            c.resize(hg.nV);
            if (int rc = values_of_replica0(c.data())) return rc;
            idx = c.data();
        }
        return hg.eval_cost(idx, infinity, cst, viol);
    }

    // the costs of the replicas' assignments `cur` ([R][n_vars], packed order) into rep_cost / rep_viol, on the
    // stream; g: the engine's Dev (k_cost_partial takes it as the engine's kernels do); mode, best: k_cost_final
    template <typename G>
    int launch_costs(G& g, const int32_t* cur, double infinity, int mode, const repcost::BestRec& best) {
        g.bpr = cost_blocks;
        const repcost::CostArgs a{cur, cost_off.p, evc.p, hg.nF, infinity, part_cost.p, part_viol.p};
        hipLaunchKernelGGL((repcost::k_cost_partial<G>), dim3((unsigned)(cost_blocks * n_rep)), dim3(repcost::COST_TPB), 0,
                           stream, g, a);
        MXS_TRY(hipGetLastError());
        hipLaunchKernelGGL((repcost::k_cost_final<repcost::BestRec>), dim3((unsigned)blocks_of(n_rep, 64)), dim3(64), 0, stream,
                           (int)n_rep, cost_blocks, (int)g.is_max, (const double*)part_cost.p, (const long long*)part_viol.p,
                           rep_cost.p, rep_viol.p, mode, best);
        MXS_TRY(hipGetLastError());
        return MXS_OK;
    }

    int fetch_costs(std::vector<double>& hc, std::vector<long long>& hv, const double* dc, const long long* dv) {
        hc.resize(n_rep), hv.resize(n_rep);
        MXS_TRY(hipMemcpyAsync(hc.data(), dc, 8 * (size_t)n_rep, hipMemcpyDeviceToHost, stream));
        MXS_TRY(hipMemcpyAsync(hv.data(), dv, 8 * (size_t)n_rep, hipMemcpyDeviceToHost, stream));
        MXS_TRY(hipStreamSynchronize(stream));
        return MXS_OK;
    }

    // the costs alone (mode 0), fetched
    template <typename G>
    int current_costs(G& g, const int32_t* cur, double infinity, std::vector<double>& hc, std::vector<long long>& hv) {
        MXS_TRY(hipSetDevice(device));
        if (int rc = launch_costs(g, cur, infinity, 0, repcost::BestRec{})) return rc;
        return fetch_costs(hc, hv, rep_cost.p, rep_viol.p);
    }

    template <typename G>
    int replica_costs(G& g, const int32_t* cur, double infinity, double* cst, int64_t* viol) {
        std::vector<double> hc;
        std::vector<long long> hv;
        if (int rc = current_costs(g, cur, infinity, hc, hv)) return rc;
        for (int r = 0; r < n_rep; ++r) {
            if (cst) cst[r] = hc[r];
            if (viol) viol[r] = (int64_t)hv[r];
        }
        return MXS_OK;
    }

    // the CURRENT states ranked (repcost::best_replica): the best replica, its cost and its violations
    template <typename G>
    int best_current(G& g, const int32_t* cur, double infinity, int32_t* replica, double* cst, int64_t* viol) {
        std::vector<double> hc;
        std::vector<long long> hv;
        if (int rc = current_costs(g, cur, infinity, hc, hv)) return rc;
        const int r = repcost::best_replica(n_rep, g.is_max, hc.data(), hv.data());
        if (replica) *replica = r;
        if (cst) *cst = hc[r];
        if (viol) *viol = (int64_t)hv[r];
        return MXS_OK;
    }
};

// The best state every replica has shown, kept on the device (mxs_dsa_track_best, mxs_gdba_track_best): what an engine
// whose runs are not monotone holds beside its Host.  The engine passes what is its own with every call: rh, its Dev
// g, the live values `cur` ([R][n_vars], in the order of rh.h_q) and `step`, its count of cycles or rounds.
template <typename T>
struct BestTracker {
    bool tracked = false;  // track() was called
    int32_t every = 0;     // > 0: records are kept
    double best_infinity = INFINITY;
    Buf<double> best_cost;
    Buf<long long> best_viol, best_step;
    Buf<int32_t> best_improved, best_idx;

    repcost::BestRec rec() const {
        return repcost::BestRec{best_cost.p, best_viol.p, best_step.p, best_improved.p, best_idx.p};
    }

    void drop() {
        best_cost.release(), best_viol.release(), best_step.release(), best_improved.release(), best_idx.release();
        every = 0;
    }

    // the current states against the records (mode 1; 2: the first record), three launches in stream order
    template <typename G>
    int record(Host<T>& rh, G& g, const int32_t* cur, int64_t step, int mode) {
        if (int rc = rh.launch_costs(g, cur, best_infinity, mode, rec())) return rc;
        const int bpr = std::max(1, blocks_of(g.n_vars, AUX_TPB));
        hipLaunchKernelGGL((repcost::k_best_copy<repcost::BestRec>), dim3((unsigned)(bpr * rh.n_rep)), dim3(AUX_TPB), 0,
                           rh.stream, (int)g.n_vars, bpr, cur, (const double*)rh.rep_cost.p,
                           (const long long*)rh.rep_viol.p, (long long)step, rec());
        MXS_TRY(hipGetLastError());
        return MXS_OK;
    }

    // after the launches of step `step` (counted from 1)
    template <typename G>
    int after_step(Host<T>& rh, G& g, const int32_t* cur, int64_t step) {
        return every > 0 && step % every == 0 ? record(rh, g, cur, step, 1) : MXS_OK;
    }

    // after the engine's init kernel: the records start again (the engine synchronises, also when this failed)
    template <typename G>
    int on_reset(Host<T>& rh, G& g, const int32_t* cur) {
        return every > 0 ? record(rh, g, cur, 0, 2) : MXS_OK;
    }

    // ev > 0: a record per replica, compared after every ev-th step, the first one the state as it is now (step 0 of
    // a fresh engine); ev == 0: none, get() ranks the current states under `infinity`.  Clears the records.
    template <typename G>
    int track(Host<T>& rh, G& g, const int32_t* cur, int64_t step, int32_t ev, double infinity) {
        if (ev < 0) return fail(MXS_E_INVALID, "every must be 0 (off) or positive");
        MXS_TRY(hipSetDevice(rh.device));
        drop();
        if (ev > 0) {
            const size_t R = (size_t)rh.n_rep;
            int rc = alloc_rep(best_cost, R, "records");
            if (!rc) rc = alloc_rep(best_viol, R, "records");
            if (!rc) rc = alloc_rep(best_step, R, "records");
            if (!rc) rc = alloc_rep(best_improved, R, "records");
            if (!rc) rc = alloc_rep(best_idx, R * g.n_vars, "best states");
            if (rc) {  // no records, and get keeps what the last successful call set (tracked, best_infinity)
                drop();
                return rc;
            }
        }
        tracked = true;
        best_infinity = infinity;
        every = ev;
        if (ev == 0) return MXS_OK;
        if (int rc = record(rh, g, cur, step, 2)) return rc;
        MXS_TRY(hipStreamSynchronize(rh.stream));
        return MXS_OK;
    }

    // the record of replica r (-1: of the best one) where records are kept, else its current state at `step`;
    // current_idx_of(r, idx): the engine's get_state; prefix: the engine's, for the refusal ("mxs_dsa")
    template <typename G, typename F>
    int get(Host<T>& rh, G& g, const int32_t* cur, int64_t step, int32_t r, int32_t* replica, int64_t* step_out, double* cst,
            int64_t* viol, int32_t* idx, F current_idx_of, const char* prefix) {
        const int32_t n_rep = rh.n_rep;
        if (r < -1 || r >= n_rep) return fail(MXS_E_INVALID, "replica out of range");
        if (!tracked) return fail(MXS_E_STATE, std::string(prefix) + "_get_best before " + prefix + "_track_best");
        MXS_TRY(hipSetDevice(rh.device));
        std::vector<double> hc;
        std::vector<long long> hv, hy(n_rep, (long long)step);
        if (every > 0) {  // the records
            if (int rc = rh.fetch_costs(hc, hv, best_cost.p, best_viol.p)) return rc;
            MXS_TRY(hipMemcpyAsync(hy.data(), best_step.p, 8 * (size_t)n_rep, hipMemcpyDeviceToHost, rh.stream));
            MXS_TRY(hipStreamSynchronize(rh.stream));
        } else {          // the current states
            if (int rc = rh.current_costs(g, cur, best_infinity, hc, hv)) return rc;
        }
        if (r < 0) r = repcost::best_replica(n_rep, g.is_max, hc.data(), hv.data());
        if (replica) *replica = r;
        if (step_out) *step_out = (int64_t)hy[r];
        if (cst) *cst = hc[r];
        if (viol) *viol = (int64_t)hv[r];
        if (idx && g.n_vars) {
            if (every == 0) return current_idx_of(r, idx);
            std::vector<int32_t> hi(g.n_vars);
            MXS_TRY(hipMemcpyAsync(hi.data(), best_idx.p + (size_t)r * g.n_vars, 4 * (size_t)g.n_vars, hipMemcpyDeviceToHost,
                                   rh.stream));
            MXS_TRY(hipStreamSynchronize(rh.stream));
            rh.unpack(hi, idx);
        }
        return MXS_OK;
    }
};

}  // namespace rephost
