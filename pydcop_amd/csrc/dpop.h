// dpop.h -- the reference's DPOP (pydcop/algorithms/dpop.py: Petcu & Faltings 2005) on gfx950, #included at the
// end of mgm.hip after mgm2.h (one translation unit for the gfx950 library and for the serial emulated build of
// tests/emu).  tests/dpop_oracle.py restates the same arithmetic in numpy; both follow the reference bit for bit.
//
// The tree (parent, ordered children) comes from the caller.  The host plan validates it, gives every constraint
// to the deepest variable of its scope, and computes the separators bottom-up.  A node's separator is listed in the
// reference's dimension order: first appearance over [UTIL of child 1, UTIL of child 2, ..., constraint 1, ...]
// (join, relations.py:1701-1704, then projection removes the node's own variable), and its UTIL table is stored
// in C order over that list, so mxs_dpop_get_util returns the reference's array as it is.
//
// One flat pool of T holds [variable costs | constraint tables | UTIL tables]; a term of a node's join is an offset
// into it plus one stride per separator digit plus the stride of the node's own variable.
//   k_dpop_util   per output entry: min / max over d of  (((cost_v[d] + U_c1) + U_c2) + ... + r_1) + r_2 ...
//                 in that order (no contraction, no reassociation), the first optimum under a strict compare
//   k_dpop_value  per node, top-down: the same sums at the separator's chosen indices; writes idx[v], cost[v]
// Both walk the levels [begin, end) themselves.  A launch of several levels has ONE workgroup and puts a fence and a
// barrier between levels (narrow levels: a DFS tree is deep and most levels are tiny); a launch of one level
// has one workgroup per block of entries.
#pragma once

#include <algorithm>
#include <cmath>

namespace dpop {

using mxs_host::Buf;
using mxs_host::fail;

constexpr int TPB = 128;          // consecutive threads on consecutive entries: coalesced stores
constexpr int MAX_DIGITS = 31;    // separator variables with more than one value: 2^31 entries at the very least
constexpr int TERM_CACHE = 8;     // term base offsets kept in LDS; further terms recompute theirs per d
constexpr int64_t MAX_TABLE = 2147483647;  // entries of one table (32-bit entry arithmetic on the device)
constexpr int DEFAULT_FUSE_ENTRIES = 128;  // levels up to one block of entries are walked by one workgroup (the A/B)
constexpr double INT32_BOUND = 2147483647.0;  // find_arg_optimal starts from the int32 extremes (relations.py:1568-1571)

template <typename T>
struct Dev {
    T* pool;                    // [costs | tables | utils]
    const int32_t* dom;         // [n_vars]
    const int32_t* entries;     // [n_vars] UTIL entries (1 for a root: its one "entry" is the VALUE step)
    const int64_t* util_off;    // [n_vars] pool offset of the UTIL (-1: root)
    const int32_t* sep_ptr;     // [n_vars + 1] -> sep_var / sep_size: the separator variables of more than one value
    const int32_t* sep_var;
    const int32_t* sep_size;
    const int32_t* term_ptr;    // [n_vars + 1] -> the terms of the node's join, in the reference's order
    const int64_t* term_off;    // pool offset of the term's table
    const int32_t* term_sv;     // stride of the node's own variable in it
    const int32_t* dim_ptr;     // [n_terms + 1] -> (dim_pos, dim_stride): the separator digits the term depends on
    const int32_t* dim_pos;
    const int32_t* dim_stride;
    const int32_t* ulevel_ptr;  // [n_heights + 1] -> ublk_*: the blocks of TPB entries of a height level
    const int32_t* ublk_node;
    const int32_t* ublk_first;
    const int32_t* vlevel_ptr;  // [n_depths + 1] -> vnode: the nodes of a depth level
    const int32_t* vnode;
    int32_t* idx;               // [n_vars] chosen value index
    T* cost;                    // [n_vars] the joined value at the chosen entry
};

// the offset of the entry of term t that the digits in column `tid` of s_dig select (the node's own variable at 0)
template <typename T>
__device__ __forceinline__ int32_t term_base(const Dev<T>& P, int t, int32_t (*s_dig)[TPB], int tid) {
    int32_t base = 0;
    for (int k = P.dim_ptr[t]; k < P.dim_ptr[t + 1]; ++k) base += s_dig[P.dim_pos[k]][tid] * P.dim_stride[k];
    return base;
}

// min / max over d of the joined value of node v at the digits in column `tid`; the first optimum
template <typename T, bool IS_MAX>
__device__ __forceinline__ void joined_optimum(const Dev<T>& P, int v, int32_t (*s_dig)[TPB],
                                               int32_t (*s_base)[TPB], int tid, T& best, int32_t& arg) {
    const int t0 = P.term_ptr[v], nt = P.term_ptr[v + 1] - t0;
    const int nc = nt < TERM_CACHE ? nt : TERM_CACHE;
    for (int t = 0; t < nc; ++t) s_base[t][tid] = term_base(P, t0 + t, s_dig, tid);
    const int D = P.dom[v];
    best = (T)0;
    arg = 0;
    for (int d = 0; d < D; ++d) {
        T acc = P.pool[P.term_off[t0] + s_base[0][tid] + (int64_t)d * P.term_sv[t0]];  // term 0: the variable's costs
        for (int t = 1; t < nt; ++t) {
            const int32_t base = t < TERM_CACHE ? s_base[t][tid] : term_base(P, t0 + t, s_dig, tid);
            acc = acc + P.pool[P.term_off[t0 + t] + base + (int64_t)d * P.term_sv[t0 + t]];
        }
        if (d == 0 || (IS_MAX ? best < acc : best > acc)) {
            best = acc;
            arg = d;
        }
    }
}

template <typename T, bool IS_MAX>
__global__ __launch_bounds__(TPB) void k_dpop_util(Dev<T> P, int lvl_begin, int lvl_end) {
    __shared__ int32_t s_dig[MAX_DIGITS][TPB];
    __shared__ int32_t s_base[TERM_CACHE][TPB];
    const int tid = threadIdx.x;
    for (int L = lvl_begin; L < lvl_end; ++L) {
        const int b1 = P.ulevel_ptr[L + 1];
        for (int b = P.ulevel_ptr[L] + (int)blockIdx.x; b < b1; b += (int)gridDim.x) {
            const int v = P.ublk_node[b];
            const int32_t e = P.ublk_first[b] + tid;
            if (e < P.entries[v]) {
                const int s0 = P.sep_ptr[v], S = P.sep_ptr[v + 1] - s0;
                uint32_t rem = (uint32_t)e;
                for (int j = S - 1; j >= 0; --j) {
                    const uint32_t sz = (uint32_t)P.sep_size[s0 + j], q = rem / sz;
                    s_dig[j][tid] = (int32_t)(rem - q * sz);
                    rem = q;
                }
                T best;
                int32_t arg;
                joined_optimum<T, IS_MAX>(P, v, s_dig, s_base, tid, best, arg);
                P.pool[P.util_off[v] + e] = best;
            }
        }
        if (lvl_end - lvl_begin > 1) {  // one workgroup walks the levels: the next one reads what this one wrote
            __threadfence();
            __syncthreads();
        }
    }
}

template <typename T, bool IS_MAX>
__global__ __launch_bounds__(TPB) void k_dpop_value(Dev<T> P, int lvl_begin, int lvl_end) {
    __shared__ int32_t s_dig[MAX_DIGITS][TPB];
    __shared__ int32_t s_base[TERM_CACHE][TPB];
    const int tid = threadIdx.x;
    for (int L = lvl_begin; L < lvl_end; ++L) {
        const int n1 = P.vlevel_ptr[L + 1];
        for (int i = P.vlevel_ptr[L] + (int)blockIdx.x * TPB + tid; i < n1; i += (int)gridDim.x * TPB) {
            const int v = P.vnode[i];
            const int s0 = P.sep_ptr[v], S = P.sep_ptr[v + 1] - s0;
            for (int j = 0; j < S; ++j) s_dig[j][tid] = P.idx[P.sep_var[s0 + j]];
            T best;
            int32_t arg;
            joined_optimum<T, IS_MAX>(P, v, s_dig, s_base, tid, best, arg);
            P.idx[v] = arg;
            P.cost[v] = best;
        }
        if (lvl_end - lvl_begin > 1) {
            __threadfence();
            __syncthreads();
        }
    }
}

struct Launch {
    int32_t begin, end;
    uint32_t grid;
};

enum { ST_COMPONENTS, ST_DEPTH, ST_SEP, ST_WIDEST, ST_ENTRIES, ST_BYTES, ST_LAUNCH_UTIL, ST_LAUNCH_VALUE, ST_UTIL_NS,
       ST_VALUE_NS, ST_COUNT };

struct Base {
    virtual ~Base() {}
    virtual int init(const mxs_graph& G, const mxs_params& p, const int32_t* parent, const int32_t* crow,
                     const int32_t* cidx, int64_t max_bytes, int32_t fuse_entries, int32_t device) = 0;
    virtual int solve() = 0;
    virtual int get_state(int32_t* idx, double* cost) = 0;
    virtual int eval_cost(const int32_t* idx, double infinity, double* cost, int64_t* violations) = 0;
    virtual int get_util(int32_t var, double* buf, int64_t n) = 0;
    int64_t stats[ST_COUNT] = {0};
    std::vector<std::vector<int32_t>> sep;  // every node's separator, the reference's dimension order
    std::vector<int32_t> h_parent;
};

template <typename T>
struct Engine : Base {
    int device = 0;
    bool solved = false;
    hipStream_t stream = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    mxs_host::HostGraph hg;
    std::vector<int32_t> h_entries;
    std::vector<int64_t> h_uoff;
    std::vector<Launch> util_launches, value_launches;
    Buf<T> pool, cost;
    Buf<int32_t> dom, entries, sep_ptr, sep_var, sep_size, term_ptr, term_sv, dim_ptr, dim_pos, dim_stride, ulevel_ptr,
        ublk_node, ublk_first, vlevel_ptr, vnode, idx;
    Buf<int64_t> util_off, term_off;
    Dev<T> g{};
    bool is_max = false;

    ~Engine() override {
        for (auto& e : ev)
            if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
    }

    int init(const mxs_graph& G, const mxs_params& p, const int32_t* parent, const int32_t* crow, const int32_t* cidx,
             int64_t max_bytes, int32_t fuse_entries, int32_t dev) override {
        if (int rc = mxs_host::check_device(dev)) return rc;  // (the device itself is touched after the validation)
        device = dev;
        if (int rc = hg.load(G, p)) return rc;
        const int nV = hg.nV, nF = hg.nF, nE = hg.nE;
        if (max_bytes < 0) return fail(MXS_E_INVALID, "dpop: negative max_bytes");
        if (nV && (!parent || !crow || (!cidx && crow[nV] > 0))) return fail(MXS_E_INVALID, "dpop: null tree arrays");
        is_max = hg.is_max;
        for (int f = 0; f < nF; ++f)
            if (hg.toff[f + 1] - hg.toff[f] > MAX_TABLE) return fail(MXS_E_INVALID, "dpop: constraint table larger than 2^31 - 1 entries");
        // the reference is only defined while every partial sum lies strictly inside the int32 range
        double bound = 0;
        for (int f = 0; f < nF; ++f) {
            double m = 0;
            for (int64_t i = hg.toff[f]; i < hg.toff[f + 1]; ++i) {
                if (!std::isfinite(hg.tables[i])) return fail(MXS_E_INVALID, "dpop: constraint tables must be finite (no inf / NaN entries)");
                m = std::max(m, std::fabs(hg.tables[i]));
            }
            bound += m;
        }
        for (int v = 0; v < nV; ++v) {
            double m = 0;
            for (int64_t i = hg.coff[v]; i < hg.coff[v + 1]; ++i) {
                if (!std::isfinite(hg.var_cost[i])) return fail(MXS_E_INVALID, "dpop: variable costs must be finite (no inf / NaN entries)");
                m = std::max(m, std::fabs(hg.var_cost[i]));
            }
            bound += m;
        }
        if (bound >= INT32_BOUND)
            return fail(MXS_E_INVALID, "dpop: the costs can add up to " + std::to_string(bound) +
                                           ", outside the int32 range in which the reference's DPOP is defined (sum of "
                                           "the tables' and the variable costs' largest magnitudes must stay below 2147483647)");

        // ---- the tree: parent / children consistent, acyclic
        h_parent.assign(parent, parent + nV);
        std::vector<int32_t> seen_child(nV, 0);
        if (nV && crow[0] != 0) return fail(MXS_E_INVALID, "dpop: child_rowptr must start at 0");
        for (int v = 0; v < nV; ++v) {
            if (h_parent[v] < -1 || h_parent[v] >= nV || h_parent[v] == v) return fail(MXS_E_INVALID, "dpop: not a pseudo-tree (parent out of range)");
            if (crow[v + 1] < crow[v]) return fail(MXS_E_INVALID, "dpop: child_rowptr must not decrease");
        }
        if (nV && crow[nV] > nV) return fail(MXS_E_INVALID, "dpop: not a pseudo-tree (more children than variables)");
        for (int v = 0; v < nV; ++v)
            for (int k = crow[v]; k < crow[v + 1]; ++k) {
                const int c = cidx[k];
                if (c < 0 || c >= nV || h_parent[c] != v || seen_child[c]++)
                    return fail(MXS_E_INVALID, "dpop: not a pseudo-tree (the children lists do not match the parent array)");
            }
        for (int v = 0; v < nV; ++v)
            if (h_parent[v] >= 0 && !seen_child[v])
                return fail(MXS_E_INVALID, "dpop: not a pseudo-tree (the children lists do not match the parent array)");
        // pre-order from the roots: depth, entry / exit times; a cycle is never reached from a root
        std::vector<int32_t> depth(nV, -1), tin(nV, 0), tout(nV, 0), order;
        order.reserve(nV);
        int64_t n_roots = 0;
        {
            std::vector<std::pair<int32_t, int32_t>> stack;
            int32_t clock = 0;
            for (int r = 0; r < nV; ++r) {
                if (h_parent[r] != -1) continue;
                ++n_roots;
                depth[r] = 0;
                tin[r] = clock++;
                order.push_back(r);
                stack.push_back({r, crow[r]});
                while (!stack.empty()) {
                    auto& top = stack.back();
                    if (top.second == crow[top.first + 1]) {
                        tout[top.first] = clock;
                        stack.pop_back();
                        continue;
                    }
                    const int c = cidx[top.second++];
                    depth[c] = depth[top.first] + 1;
                    tin[c] = clock++;
                    order.push_back(c);
                    stack.push_back({c, crow[c]});
                }
            }
        }
        if ((int)order.size() != nV) return fail(MXS_E_INVALID, "dpop: not a pseudo-tree (the parent array has a cycle)");
        // ---- every constraint on one root path, owned by its deepest variable
        std::vector<int32_t> owner(nF);
        for (int f = 0; f < nF; ++f) {
            int low = hg.evar[hg.frow[f]];
            for (int e = hg.frow[f]; e < hg.frow[f + 1]; ++e)
                if (depth[hg.evar[e]] > depth[low]) low = hg.evar[e];
            for (int e = hg.frow[f]; e < hg.frow[f + 1]; ++e) {
                const int u = hg.evar[e];
                if (!(tin[u] <= tin[low] && tin[low] < tout[u]))
                    return fail(MXS_E_INVALID, "dpop: not a pseudo-tree (the scope of constraint " + std::to_string(f) +
                                                   " does not lie on one root path)");
            }
            owner[f] = low;
        }
        std::vector<std::vector<int32_t>> cons(nV);
        {
            std::vector<int32_t> taken(nF, 0);
            for (int v = 0; v < nV; ++v)
                for (int k = hg.vrow[v]; k < hg.vrow[v + 1]; ++k) {
                    const int e = hg.vedges[k];
                    if (e < 0 || e >= nE || hg.evar[e] != v) return fail(MXS_E_INVALID, "var_edges inconsistent with edge_var");
                    const int f = hg.efac[e];
                    if (owner[f] == v && !taken[f]++) cons[v].push_back(f);
                }
            for (int f = 0; f < nF; ++f)
                if (!taken[f]) return fail(MXS_E_INVALID, "var_edges does not cover every edge");
        }
        // ---- separators bottom-up (reverse pre-order: children before parents), heights, sizes
        sep.assign(nV, {});
        std::vector<int32_t> height(nV, 0), mark(nV, -1);
        h_entries.assign(nV, 1);
        int64_t total = 0, widest = 0, widest_sep = 0, max_depth = 0;
        for (int i = nV - 1; i >= 0; --i) {
            const int v = order[i];
            mark[v] = v;
            auto add = [&](int u) {
                if (mark[u] != v) {
                    mark[u] = v;
                    sep[v].push_back(u);
                }
            };
            for (int k = crow[v]; k < crow[v + 1]; ++k) {
                const int c = cidx[k];
                height[v] = std::max(height[v], height[c] + 1);
                for (int u : sep[c]) add(u);
            }
            for (int f : cons[v])
                for (int e = hg.frow[f]; e < hg.frow[f + 1]; ++e) add(hg.evar[e]);
            max_depth = std::max<int64_t>(max_depth, depth[v]);
            if (h_parent[v] < 0) continue;  // (a root's separator is empty: every scope lies on a root path)
            double n = 1;
            int digits = 0;
            for (int u : sep[v]) {
                n *= hg.dom[u];
                digits += hg.dom[u] > 1;
            }
            widest_sep = std::max<int64_t>(widest_sep, (int64_t)sep[v].size());
            if (n > 9.0e18) {
                total = INT64_MAX;
                continue;
            }
            const int64_t ne = (int64_t)n;
            widest = std::max(widest, ne);
            total = total > INT64_MAX - ne ? INT64_MAX : total + ne;
            h_entries[v] = ne <= MAX_TABLE && digits <= MAX_DIGITS ? (int32_t)ne : -1;
        }
        stats[ST_COMPONENTS] = n_roots;
        stats[ST_DEPTH] = max_depth;
        stats[ST_SEP] = widest_sep;
        stats[ST_WIDEST] = widest;
        stats[ST_ENTRIES] = total;
        stats[ST_BYTES] = total > INT64_MAX / (int64_t)sizeof(T) ? INT64_MAX : total * (int64_t)sizeof(T);
        // ---- the budget, before anything is allocated
        MXS_TRY(hipSetDevice(device));
        int64_t budget = max_bytes;
        if (budget == 0) {
            size_t free_b = 0, total_b = 0;
            MXS_TRY(hipMemGetInfo(&free_b, &total_b));
            budget = (int64_t)(free_b / 10 * 8);  // 80 % of what is free: the graph, the plan and the runtime need the rest
        }
        if (stats[ST_BYTES] > budget)
            return fail(MXS_E_NOMEM, "dpop: the UTIL tables need " + (total == INT64_MAX ? std::string("more than 9e18") : std::to_string(stats[ST_BYTES])) +
                                         " bytes (" + (total == INT64_MAX ? std::string("more than 9e18") : std::to_string(total)) + " entries, the widest " +
                                         std::to_string(widest) + " over a separator of " + std::to_string(widest_sep) +
                                         " variables), over the budget of " + std::to_string(budget) + " bytes");
        for (int v = 0; v < nV; ++v)
            if (h_entries[v] < 0)
                return fail(MXS_E_INVALID, "dpop: the UTIL table of variable " + std::to_string(v) + " has more than 2^31 - 1 entries");
        // ---- pool layout and the terms
        const int64_t n_cost = hg.coff[nV], n_tab = hg.toff[nF];
        h_uoff.assign(nV, -1);
        int64_t at = n_cost + n_tab;
        for (int v = 0; v < nV; ++v)
            if (h_parent[v] >= 0) {
                h_uoff[v] = at;
                at += h_entries[v];
            }
        std::vector<int32_t> v_sep_ptr(nV + 1, 0), v_sep_var, v_sep_size, v_term_ptr(nV + 1, 0), v_term_sv, v_dim_ptr(1, 0), v_dim_pos,
            v_dim_stride, pos(nV, -1);
        std::vector<int64_t> v_term_off;
        std::vector<int32_t> acc_stride;
        for (int v = 0; v < nV; ++v) {
            int S = 0;
            for (int u : sep[v])
                if (hg.dom[u] > 1) {
                    pos[u] = S++;
                    v_sep_var.push_back(u);
                    v_sep_size.push_back(hg.dom[u]);
                }
            v_sep_ptr[v + 1] = (int32_t)v_sep_var.size();
            acc_stride.assign(S, 0);
            // one term: the table at `off` over the variables scope[0..n) in C order
            auto term = [&](int64_t off, const int32_t* scope, int n) {
                int64_t stride = 1;
                int32_t sv = 0;
                std::fill(acc_stride.begin(), acc_stride.end(), 0);
                for (int k = n - 1; k >= 0; --k) {
                    const int u = scope[k];
                    if (u == v) sv += (int32_t)stride;
                    else if (hg.dom[u] > 1) acc_stride[pos[u]] += (int32_t)stride;
                    stride *= hg.dom[u];
                }
                v_term_off.push_back(off);
                v_term_sv.push_back(sv);
                for (int j = 0; j < S; ++j)
                    if (acc_stride[j]) {
                        v_dim_pos.push_back(j);
                        v_dim_stride.push_back(acc_stride[j]);
                    }
                v_dim_ptr.push_back((int32_t)v_dim_pos.size());
            };
            const int32_t self = v;
            term(hg.coff[v], &self, 1);
            for (int k = crow[v]; k < crow[v + 1]; ++k) term(h_uoff[cidx[k]], sep[cidx[k]].data(), (int)sep[cidx[k]].size());
            for (int f : cons[v]) term(n_cost + hg.toff[f], hg.evar.data() + hg.frow[f], hg.frow[f + 1] - hg.frow[f]);
            v_term_ptr[v + 1] = (int32_t)v_term_off.size();
            for (int u : sep[v]) pos[u] = -1;
        }
        // ---- levels: UTIL by height (leaves first, roots have none), VALUE by depth (roots first)
        int n_heights = 0;
        for (int v = 0; v < nV; ++v) n_heights = std::max(n_heights, height[v] + 1);
        const int n_depths = nV ? (int)max_depth + 1 : 0;
        std::vector<std::vector<int32_t>> by_height(n_heights), by_depth(n_depths);
        for (int v : order) {
            if (h_parent[v] >= 0) by_height[height[v]].push_back(v);
            by_depth[depth[v]].push_back(v);
        }
        std::vector<int32_t> v_ulevel(1, 0), v_ublk_node, v_ublk_first, v_vlevel(1, 0), v_vnode;
        std::vector<int64_t> level_entries(n_heights, 0);
        for (int h = 0; h < n_heights; ++h) {
            for (int v : by_height[h]) {
                level_entries[h] += h_entries[v];
                for (int64_t first = 0; first < h_entries[v]; first += TPB) {
                    v_ublk_node.push_back(v);
                    v_ublk_first.push_back((int32_t)first);
                }
            }
            if (v_ublk_node.size() > (size_t)INT32_MAX) return fail(MXS_E_INVALID, "dpop: more than 2^31 - 1 blocks of entries");
            v_ulevel.push_back((int32_t)v_ublk_node.size());
        }
        for (int d = 0; d < n_depths; ++d) {
            v_vnode.insert(v_vnode.end(), by_depth[d].begin(), by_depth[d].end());
            v_vlevel.push_back((int32_t)v_vnode.size());
        }
        const int64_t cap = fuse_entries < 0 ? DEFAULT_FUSE_ENTRIES : fuse_entries;
        auto plan = [&](int n_levels, auto&& size_of, auto&& grid_of, std::vector<Launch>& out) {
            out.clear();
            for (int L = 0; L < n_levels;) {
                if (size_of(L) == 0) {
                    ++L;
                } else if (size_of(L) <= cap) {  // a run of narrow levels: one workgroup walks them
                    int E = L + 1;
                    while (E < n_levels && size_of(E) <= cap) ++E;
                    out.push_back({L, E, 1u});
                    L = E;
                } else {
                    out.push_back({L, L + 1, grid_of(L)});
                    ++L;
                }
            }
        };
        plan(n_heights, [&](int L) { return level_entries[L]; },
             [&](int L) { return (uint32_t)(v_ulevel[L + 1] - v_ulevel[L]); }, util_launches);
        plan(n_depths, [&](int L) { return (int64_t)by_depth[L].size(); },
             [&](int L) { return (uint32_t)((by_depth[L].size() + TPB - 1) / TPB); }, value_launches);
        stats[ST_LAUNCH_UTIL] = (int64_t)util_launches.size();
        stats[ST_LAUNCH_VALUE] = (int64_t)value_launches.size();
        // ---- upload
        MXS_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        for (auto& e : ev) MXS_TRY(hipEventCreate(&e));
        {
            std::vector<T> head((size_t)(n_cost + n_tab));
            for (int64_t i = 0; i < n_cost; ++i) head[(size_t)i] = (T)hg.var_cost[i];
            for (int64_t i = 0; i < n_tab; ++i) head[(size_t)(n_cost + i)] = (T)hg.tables[(size_t)i];
            MXS_TRY(pool.alloc((size_t)at));
            if (!head.empty()) {
                MXS_TRY(hipMemcpyAsync(pool.p, head.data(), head.size() * sizeof(T), hipMemcpyHostToDevice, stream));
                MXS_TRY(hipStreamSynchronize(stream));
            }
        }
        MXS_TRY(dom.upload(hg.dom, stream));
        MXS_TRY(entries.upload(h_entries, stream));
        MXS_TRY(util_off.upload(h_uoff, stream));
        MXS_TRY(sep_ptr.upload(v_sep_ptr, stream));
        MXS_TRY(sep_var.upload(v_sep_var, stream));
        MXS_TRY(sep_size.upload(v_sep_size, stream));
        MXS_TRY(term_ptr.upload(v_term_ptr, stream));
        MXS_TRY(term_off.upload(v_term_off, stream));
        MXS_TRY(term_sv.upload(v_term_sv, stream));
        MXS_TRY(dim_ptr.upload(v_dim_ptr, stream));
        MXS_TRY(dim_pos.upload(v_dim_pos, stream));
        MXS_TRY(dim_stride.upload(v_dim_stride, stream));
        MXS_TRY(ulevel_ptr.upload(v_ulevel, stream));
        MXS_TRY(ublk_node.upload(v_ublk_node, stream));
        MXS_TRY(ublk_first.upload(v_ublk_first, stream));
        MXS_TRY(vlevel_ptr.upload(v_vlevel, stream));
        MXS_TRY(vnode.upload(v_vnode, stream));
        MXS_TRY(idx.alloc(nV));
        MXS_TRY(cost.alloc(nV));
        g = Dev<T>{pool.p, dom.p, entries.p, util_off.p, sep_ptr.p, sep_var.p, sep_size.p, term_ptr.p, term_off.p, term_sv.p,
                   dim_ptr.p, dim_pos.p, dim_stride.p, ulevel_ptr.p, ublk_node.p, ublk_first.p, vlevel_ptr.p, vnode.p, idx.p, cost.p};
        return MXS_OK;
    }

    template <bool IS_MAX>
    int launch_all() {
        MXS_TRY(hipEventRecord(ev[0], stream));
        for (const Launch& l : util_launches) {
            hipLaunchKernelGGL((k_dpop_util<T, IS_MAX>), dim3(l.grid), dim3(TPB), 0, stream, g, l.begin, l.end);
            MXS_TRY(hipGetLastError());
        }
        MXS_TRY(hipEventRecord(ev[1], stream));
        for (const Launch& l : value_launches) {
            hipLaunchKernelGGL((k_dpop_value<T, IS_MAX>), dim3(l.grid), dim3(TPB), 0, stream, g, l.begin, l.end);
            MXS_TRY(hipGetLastError());
        }
        MXS_TRY(hipEventRecord(ev[2], stream));
        MXS_TRY(hipStreamSynchronize(stream));
        float u_ms = 0, v_ms = 0;
        MXS_TRY(hipEventElapsedTime(&u_ms, ev[0], ev[1]));
        MXS_TRY(hipEventElapsedTime(&v_ms, ev[1], ev[2]));
        stats[ST_UTIL_NS] = (int64_t)((double)u_ms * 1e6);
        stats[ST_VALUE_NS] = (int64_t)((double)v_ms * 1e6);
        return MXS_OK;
    }

    int solve() override {
        MXS_TRY(hipSetDevice(device));
        int rc = is_max ? launch_all<true>() : launch_all<false>();
        if (rc) return rc;
        solved = true;
        return MXS_OK;
    }

    int get_state(int32_t* out_idx, double* out_cost) override {
        if (!solved) return fail(MXS_E_STATE, "dpop: no solution yet (call mxs_dpop_solve first)");
        MXS_TRY(hipSetDevice(device));
        const int nV = hg.nV;
        if (!nV) return MXS_OK;
        std::vector<T> hc(nV);
        std::vector<int32_t> hi(nV);
        MXS_TRY(hipMemcpyAsync(hi.data(), idx.p, 4 * (size_t)nV, hipMemcpyDeviceToHost, stream));
        MXS_TRY(hipMemcpyAsync(hc.data(), cost.p, sizeof(T) * nV, hipMemcpyDeviceToHost, stream));
        MXS_TRY(hipStreamSynchronize(stream));
        for (int v = 0; v < nV; ++v) {
            if (out_idx) out_idx[v] = hi[v];
            if (out_cost) out_cost[v] = (double)hc[v];
        }
        return MXS_OK;
    }

    int get_util(int32_t var, double* buf, int64_t n) override {
        if (!solved) return fail(MXS_E_STATE, "dpop: no solution yet (call mxs_dpop_solve first)");
        if (var < 0 || var >= (int)hg.dom.size()) return fail(MXS_E_INVALID, "dpop: variable out of range");
        if (h_parent[var] < 0) return fail(MXS_E_INVALID, "dpop: a root sends no UTIL");
        if (!buf || n != h_entries[var]) return fail(MXS_E_INVALID, "dpop: the buffer must hold the UTIL's " + std::to_string(h_entries[var]) + " entries");
        MXS_TRY(hipSetDevice(device));
        std::vector<T> h((size_t)n);
        MXS_TRY(hipMemcpyAsync(h.data(), pool.p + h_uoff[var], sizeof(T) * (size_t)n, hipMemcpyDeviceToHost, stream));
        MXS_TRY(hipStreamSynchronize(stream));
        for (int64_t i = 0; i < n; ++i) buf[i] = (double)h[(size_t)i];
        return MXS_OK;
    }

    // DCOP.solution_cost of an assignment: every constraint and every variable's own cost
    int eval_cost(const int32_t* in_idx, double infinity, double* cst, int64_t* viol) override {
        std::vector<int32_t> c;
        const int nV = hg.nV;
        if (!in_idx) {
            c.resize(nV);
            int rc = get_state(c.data(), nullptr);
            if (rc) return rc;
            in_idx = c.data();
        }
        return hg.eval_cost(in_idx, infinity, cst, viol);
    }
};

}  // namespace dpop

struct mxs_dpop {
    dpop::Base* impl;
};

extern "C" {

int mxs_dpop_create(const mxs_graph* g, const mxs_params* p, const int32_t* parent, const int32_t* child_rowptr,
                    const int32_t* child_idx, int64_t max_bytes, int32_t fuse_entries, int32_t device, mxs_dpop** out) {
    return mxs_host::create<mxs_dpop, dpop::Engine>(g, p, out, parent, child_rowptr, child_idx, max_bytes, fuse_entries, device);
}
int mxs_dpop_solve(mxs_dpop* e) { return e ? e->impl->solve() : mxs_host::fail(MXS_E_INVALID, "null handle"); }
int mxs_dpop_get_state(mxs_dpop* e, int32_t* idx, double* cost) {
    return e ? e->impl->get_state(idx, cost) : mxs_host::fail(MXS_E_INVALID, "null handle");
}
int mxs_dpop_eval_cost(mxs_dpop* e, const int32_t* idx, double infinity, double* cost, int64_t* violations) {
    return e ? e->impl->eval_cost(idx, infinity, cost, violations) : mxs_host::fail(MXS_E_INVALID, "null handle");
}
int mxs_dpop_stats(const mxs_dpop* e, int64_t* out, int32_t n) {
    if (!e || !out || n < 0) return mxs_host::fail(MXS_E_INVALID, "null handle or buffer");
    for (int i = 0; i < n; ++i) out[i] = i < dpop::ST_COUNT ? e->impl->stats[i] : 0;
    return MXS_OK;
}
int mxs_dpop_util_dims(const mxs_dpop* e, int32_t var, int32_t* dims, int32_t* n) {
    if (!e || !n) return mxs_host::fail(MXS_E_INVALID, "null handle or count");
    if (var < 0 || var >= (int32_t)e->impl->sep.size()) return mxs_host::fail(MXS_E_INVALID, "dpop: variable out of range");
    if (e->impl->h_parent[var] < 0) return mxs_host::fail(MXS_E_INVALID, "dpop: a root sends no UTIL");
    const auto& s = e->impl->sep[var];
    if (dims) {
        if (*n < (int32_t)s.size()) return mxs_host::fail(MXS_E_INVALID, "dpop: the dims buffer is too short");
        for (size_t i = 0; i < s.size(); ++i) dims[i] = s[i];
    }
    *n = (int32_t)s.size();
    return MXS_OK;
}
int mxs_dpop_get_util(mxs_dpop* e, int32_t var, double* buf, int64_t n_entries) {
    return e ? e->impl->get_util(var, buf, n_entries) : mxs_host::fail(MXS_E_INVALID, "null handle");
}
int mxs_dpop_destroy(mxs_dpop* e) {
    if (e) {
        delete e->impl;
        delete e;
    }
    return MXS_OK;
}

}  // extern "C"
