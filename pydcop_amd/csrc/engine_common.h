// engine_common.h -- the host scaffold the DSA / MGM / MGM-2 / GDBA / DBA / DPOP engines share (dsa.hip, mgm.hip and the
// headers mgm.hip includes): error helpers, the device buffer, the counter-based generator, the host copy of an
// mxs_graph with its checks and DCOP.solution_cost, the device side of the slot and the packed view of
// local_search.h, and the shell of the mxs_*_create entry points.  Nothing here is a kernel; what only one engine
// needs stays in that engine, what only the replica engines (dsa.hip, mgm.hip) share is replica_host.h.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <exception>
#include <string>
#include <vector>

#include "../../include/maxsum_gpu.h"
#include "local_search.h"

extern "C" __attribute__((visibility("hidden"))) void mxs_set_last_error(const char* msg);  // engine.hip

namespace mxs_host {

static int fail(int code, const std::string& msg) {
    mxs_set_last_error(msg.c_str());
    return code;
}
#define MXS_TRY(call)                                                                               \
    do {                                                                                            \
        hipError_t e__ = (call);                                                                    \
        if (e__ != hipSuccess) return ::mxs_host::fail(MXS_E_HIP, std::string(#call) + " failed");   \
    } while (0)

template <typename U>
struct Buf {
    U* p = nullptr;
    size_t n = 0;
    hipError_t upload(const std::vector<U>& h, hipStream_t st) {
        release();
        n = h.size();
        hipError_t e = hipMalloc((void**)&p, (n ? n : 1) * sizeof(U));
        if (e != hipSuccess || h.empty()) return e;
        e = hipMemcpyAsync(p, h.data(), n * sizeof(U), hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return e;
        return hipStreamSynchronize(st);
    }
    hipError_t alloc(size_t count) {
        n = count;
        return hipMalloc((void**)&p, (n ? n : 1) * sizeof(U));
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    ~Buf() {
        if (p) (void)hipFree(p);
    }
};

// ---- the generator: every draw of the reference's unseeded `random` is a function of (seed, variable, cycle, draw),
// the splitmix64 finaliser over that key -- oracle/dsa_oracle.c, tests/mgm2_oracle.py, tests/gdba_oracle.py,
// tests/mgm_keyed_oracle.py, bit for bit.
// The draw ids in use:
//   DSA    0 start value, 1 move test, 2 choice among the best values
//   MGM-2  0 start, 1 offerer test, 2 partner, 3 best unilateral value, 4 the `favor: no` coin, 5 the accepted offer
//   GDBA   6 start value (cycle 0), 7 one of the best values
//   DBA    8 start value (cycle 0), 9 one of the best values (at the computation's cycle_count: round - 1)
//   MGM    10 start value (cycle 0), 11 one of the best values (at the computation's cycle_count: round k, from 1, is k);
//          mxs_mgm_create_keyed only -- mxs_mgm_create fixes both draws to "first"
__host__ __device__ inline uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__host__ __device__ inline double uniform(uint64_t seed, int32_t variable, int64_t cycle, int32_t draw) {
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * ((uint64_t)(uint32_t)variable + 1);
    z = mix64(z) + 0x9E3779B97F4A7C15ull * ((uint64_t)cycle + 1);
    z = mix64(z) + (uint64_t)(uint32_t)draw;
    return (double)(mix64(z) >> 11) * (1.0 / 9007199254740992.0);
}
// the same generator from its first stage, mix64(seed + G * (variable + 1)): a constant of the variable,
// computed once on the host for DSA's packed kernel (two 64-bit multiplies per draw fewer)
__host__ __device__ inline uint64_t uniform_key(uint64_t seed, int32_t variable) {
    return mix64(seed + 0x9E3779B97F4A7C15ull * ((uint64_t)(uint32_t)variable + 1));
}
__host__ __device__ inline double uniform_from_key(uint64_t key, int64_t cycle, int32_t draw) {
    uint64_t z = key + 0x9E3779B97F4A7C15ull * ((uint64_t)cycle + 1);
    z = mix64(z) + (uint64_t)(uint32_t)draw;
    return (double)(mix64(z) >> 11) * (1.0 / 9007199254740992.0);
}

// ---- the device
inline int check_device(int dev) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(MXS_E_NODEVICE, "no HIP device visible: the engine has no CPU fallback");
    if (dev < 0 || dev >= count) return fail(MXS_E_INVALID, "device index out of range");
    return MXS_OK;
}
inline int open_device(int dev, hipStream_t* stream) {
    if (int rc = check_device(dev)) return rc;
    MXS_TRY(hipSetDevice(dev));
    MXS_TRY(hipStreamCreateWithFlags(stream, 0));
    return MXS_OK;
}

// ---- the host copy of an mxs_graph
struct HostGraph {
    int nV = 0, nF = 0, nE = 0;
    bool is_max = false;
    std::vector<int32_t> dom, frow, evar, efac, vrow, vedges, init;  // efac: the constraint of an edge; init: -1 = none
    std::vector<int64_t> toff, coff;                                 // coff: prefix sums of dom (offsets into var_cost)
    std::vector<double> tables, var_cost, eval_var_cost;             // eval_var_cost: what solution_cost is evaluated on

    // the copies and the checks every engine makes; an engine's own checks follow it
    int load(const mxs_graph& G, const mxs_params& p) {
        nV = G.n_vars, nF = G.n_factors, nE = G.n_edges;
        if (nV < 0 || nF < 0 || nE < 0) return fail(MXS_E_INVALID, "negative size");
        if (p.mode != MXS_MODE_MIN && p.mode != MXS_MODE_MAX) return fail(MXS_E_INVALID, "invalid mode");
        is_max = p.mode == MXS_MODE_MAX;
        dom.assign(G.dom_size, G.dom_size + nV);
        frow.assign(G.factor_rowptr, G.factor_rowptr + nF + 1);
        evar.assign(G.edge_var, G.edge_var + nE);
        toff.assign(G.table_off, G.table_off + nF + 1);
        coff.assign(nV + 1, 0);
        for (int v = 0; v < nV; ++v) {
            if (dom[v] < 1) return fail(MXS_E_INVALID, "empty domain");
            coff[v + 1] = coff[v] + dom[v];
        }
        efac.assign(nE, 0);
        for (int f = 0; f < nF; ++f) {
            if (frow[f + 1] <= frow[f]) return fail(MXS_E_INVALID, "factor without variable");
            for (int e = frow[f]; e < frow[f + 1]; ++e) {
                if (evar[e] < 0 || evar[e] >= nV) return fail(MXS_E_INVALID, "edge_var out of range");
                efac[e] = f;
            }
        }
        vrow.assign(G.var_rowptr, G.var_rowptr + nV + 1);
        vedges.assign(G.var_edges, G.var_edges + nE);
        tables.assign(G.tables, G.tables + toff[nF]);
        var_cost.assign(G.var_cost, G.var_cost + coff[nV]);
        const double* ev = G.eval_var_cost ? G.eval_var_cost : G.var_cost;
        eval_var_cost.assign(ev, ev + coff[nV]);
        return MXS_OK;
    }

    // the initial values, for the engines that start from them (after load)
    int load_init(const mxs_graph& G) {
        init.assign(nV, -1);
        if (G.init_idx)
            for (int v = 0; v < nV; ++v) {
                if (G.init_idx[v] >= dom[v]) return fail(MXS_E_INVALID, "init_idx out of the domain");
                init[v] = G.init_idx[v];
            }
        return MXS_OK;
    }

    // DCOP.solution_cost of an assignment: every constraint and every variable's own cost; an entry equal to
    // `infinity` counts as a violation instead
    int eval_cost(const int32_t* idx, double infinity, double* cost, int64_t* viol) const {
        for (int v = 0; v < nV; ++v)
            if (idx[v] < 0 || idx[v] >= dom[v]) return fail(MXS_E_INVALID, "assignment index out of the domain");
        double soft = 0;
        int64_t hard = 0;
        for (int f = 0; f < nF; ++f) {
            int64_t lin = 0;
            for (int e = frow[f]; e < frow[f + 1]; ++e) lin = lin * dom[evar[e]] + idx[evar[e]];
            const double r = tables[toff[f] + lin];
            if (r != infinity) soft += r; else hard += 1;
        }
        for (int v = 0; v < nV; ++v) {
            const double x = eval_var_cost[coff[v] + idx[v]];
            if (x != infinity) soft += x; else hard += 1;
        }
        if (cost) *cost = soft;
        if (viol) *viol = hard;
        return MXS_OK;
    }

    // the reference's optimal_cost_value of a variable without neighbours: min / max over (cost, value) tuples
    // (relations.py:1661-1665), the costs compared in T; value_rank: the order of the domain's values (empty: index order)
    template <typename T>
    int optimal_cost_value(int v, bool max_mode, const std::vector<int32_t>& value_rank) const {
        const int32_t* rk = value_rank.empty() ? nullptr : value_rank.data() + coff[v];
        int best = 0;
        for (int d = 1; d < dom[v]; ++d) {
            const T a = (T)var_cost[coff[v] + d], b = (T)var_cost[coff[v] + best];
            const int rd = rk ? rk[d] : d, rb = rk ? rk[best] : best;
            if (max_mode ? (a > b || (a == b && rd > rb)) : (a < b || (a == b && rd < rb))) best = d;
        }
        return best;
    }
};

template <typename T>
std::vector<T> narrowed(const std::vector<double>& a) {  // the host's doubles in the engine's type
    return std::vector<T>(a.begin(), a.end());
}

// graph indices -> positions in `q` (negative entries, "none", stay)
inline std::vector<int32_t> remap(std::vector<int32_t> a, const std::vector<int32_t>& q) {
    for (auto& x : a)
        if (x >= 0) x = q[x];
    return a;
}

// ---- the device side of the slot view (local_search.h)
struct DevSlots {
    Buf<int64_t> base, row_base;
    Buf<int32_t> stride_v, nb_rowptr, nb_var, nb_stride, nb0_var, nb0_stride, conc_rowptr, conc_var, row_nb_stride, row_nb0_stride;
    Buf<uint8_t> rows;  // the row view of the variables the pack cannot take (Slots::rows)
    bool have_rows = false;
    int32_t rows_int8 = 0;

    // q: the positions the variable references (nb_var, nb0_var, conc_var) are uploaded as (NULL: graph indices);
    // nb0: also the first-neighbour arrays (the views of MGM-2 and GDBA carry null pointers for them)
    int upload(const lsearch::HostSlots& hs, hipStream_t st, const std::vector<int32_t>* q, bool nb0) {
        auto ref = [&](const std::vector<int32_t>& a) { return q ? remap(a, *q) : a; };
        MXS_TRY(base.upload(hs.base, st));
        MXS_TRY(stride_v.upload(hs.stride_v, st));
        MXS_TRY(nb_rowptr.upload(hs.nb_rowptr, st));
        MXS_TRY(nb_var.upload(ref(hs.nb_var), st));
        MXS_TRY(nb_stride.upload(hs.nb_stride, st));
        if (nb0) {
            MXS_TRY(nb0_var.upload(ref(hs.nb0_var), st));
            MXS_TRY(nb0_stride.upload(hs.nb0_stride, st));
        }
        MXS_TRY(conc_rowptr.upload(hs.conc_rowptr, st));
        MXS_TRY(conc_var.upload(ref(hs.conc_var), st));
        return MXS_OK;
    }

    // the row view for the variables `rest` (domains of at most 32 values; $MAXSUM_LOCAL_SEARCH_ROWS=0 leaves it out,
    // the budget in bytes can be set: A/B runs and tests); word: sizeof(T)
    void upload_rows(lsearch::HostSlots& hs, const std::vector<int32_t>& rest, const HostGraph& hg, int max_dom, int word,
                     hipStream_t st) {
        const int64_t budget = lsearch::HostSlots::rows_budget();
        have_rows = budget > 0 && max_dom <= 32 && hs.build_rows(rest, hg.dom, hg.vrow, hg.toff, hg.tables, word, 32, budget);
        rows_int8 = hs.rows_int8 ? 1 : 0;
        if (!have_rows) return;
        // an upload that fails (device memory) leaves the strided path: free what was allocated and carry on
        const bool ok = rows.upload(hs.rows, st) == hipSuccess && row_base.upload(hs.row_base, st) == hipSuccess &&
                        row_nb_stride.upload(hs.row_nb_stride, st) == hipSuccess &&
                        row_nb0_stride.upload(hs.row_nb0_stride, st) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            rows.release(), row_base.release(), row_nb_stride.release(), row_nb0_stride.release();
            have_rows = false;
        }
        hs.rows.clear();
        hs.rows.shrink_to_fit();
    }

    lsearch::Slots view() const {
        return lsearch::Slots{base.p, stride_v.p, nb_rowptr.p, nb_var.p, nb_stride.p, nb0_var.p, nb0_stride.p,
                              conc_rowptr.p, conc_var.p, have_rows ? rows.p : nullptr, row_base.p, row_nb_stride.p,
                              row_nb0_stride.p, rows_int8};
    }
};

// ---- the packed view (local_search.h).  Packed positions: the packed variables in wave order, then the others;
// the engines on the packed view keep their dynamic state in that order (Dev::q).
inline std::vector<int32_t> packed_order(const lsearch::HostPack& hp, int nV) {
    std::vector<int32_t> q(nV, -1);
    int nq = 0;
    for (int v : hp.vars) q[v] = nq++;
    for (int v = 0; v < nV; ++v)
        if (q[v] < 0) q[v] = nq++;
    return q;
}

template <typename T>
struct DevPack {
    Buf<lsearch::PackWave> waves;
    Buf<int32_t> nb, slot, rest, dom;  // dom: [packed variables] dom_size in packed order
    Buf<int8_t> rec8;                  // the records: small integers where every entry is one, else T
    Buf<T> recT;
    bool int8 = false;
    int n_rest = 0;
    int32_t n_lanes = 0;

    int upload(const lsearch::HostPack& hp, const std::vector<int32_t>& q, const std::vector<int32_t>& h_dom, hipStream_t st) {
        int8 = hp.int8_exact;
        if (int8) MXS_TRY(rec8.upload(narrowed<int8_t>(hp.rec), st));
        else MXS_TRY(recT.upload(narrowed<T>(hp.rec), st));
        std::vector<int32_t> pdom(hp.vars.size());
        for (int v : hp.vars) pdom[q[v]] = h_dom[v];
        MXS_TRY(waves.upload(hp.waves, st));
        MXS_TRY(nb.upload(remap(hp.nb, q), st));
        MXS_TRY(slot.upload(hp.slot, st));
        MXS_TRY(rest.upload(hp.rest, st));
        MXS_TRY(dom.upload(pdom, st));
        n_rest = (int)hp.rest.size();
        n_lanes = (int32_t)hp.nb.size();
        return MXS_OK;
    }

    lsearch::Pack view() const {
        return lsearch::Pack{waves.p, nb.p, slot.p, int8 ? (const void*)rec8.p : (const void*)recT.p, n_lanes};
    }
};

// ---- the shell of an mxs_*_create: Handle is the C handle {Base* impl}, args go to Engine<T>::init after the
// graph and the parameters
template <typename Handle, template <typename> class Engine, typename... Args>
int create(const mxs_graph* g, const mxs_params* p, Handle** out, Args... args) {
    if (!g || !p || !out) return fail(MXS_E_INVALID, "null argument");
    *out = nullptr;
    try {
        decltype(Handle::impl) impl = nullptr;
        if (p->dtype == MXS_DTYPE_F32) impl = new Engine<float>();
        else impl = new Engine<double>();
        int rc = impl->init(*g, *p, args...);
        if (rc) {
            delete impl;
            return rc;
        }
        *out = new Handle{impl};
        return MXS_OK;
    } catch (const std::exception& ex) {
        return fail(MXS_E_NOMEM, ex.what());
    }
}

}  // namespace mxs_host
