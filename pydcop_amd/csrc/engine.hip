// engine.hip -- the C-ABI of include/maxsum_gpu.h on top of the gfx950 kernels.
//
// Host side of one engine = one GPU, one HIP stream:
//   create   build_layout (layout.cpp) -> upload -> cycle 0 (start) on the device
//   run      one k_sweep launch per synchronous cycle (+ one k_factor_nary launch
//            when the graph has workgroup-per-factor classes), ping-ponging the
//            two buffers of each message array; launch-bound cycle loops are
//            replayed from a hipGraph
//   get_*    copy back, undo the internal permutation (and the max-mode negation)
// There is no host fallback: every cycle runs on the device.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <unistd.h>

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/maxsum_gpu.h"
#include "../../include/maxsum_gpu_quiescence.h"
#include "kernels.h"
#include "anytime.h"
#include "quiescence.h"
#include "nary_box.h"
#include "bin_box.h"
#include "small_box.h"
#include "layout.h"

namespace mxs {

static thread_local std::string g_err;

static int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

}  // namespace mxs
// the error slot of the calling thread, for the other translation units of the library
// (amaxsum.hip); not part of the C-ABI: hidden
extern "C" __attribute__((visibility("hidden"))) void mxs_set_last_error(const char* msg) { mxs::g_err = msg ? msg : ""; }
namespace mxs {

static hipError_t copy_sync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind,
                            hipStream_t st) {
    if (!bytes) return hipSuccess;
    hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, st);
    if (e != hipSuccess) return e;
    return hipStreamSynchronize(st);
}

#define HIP_TRY(expr)                                                                       \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess)                                                               \
            return fail(MXS_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));      \
    } while (0)

// ---- RCCL, bound at run time -------------------------------------------------------
// The sharded cycle loop calls RCCL itself (grouped ncclSend / ncclRecv per peer = an
// all-to-all with fixed counts) so that no interpreter sits between two cycles.  The
// library is dlopen'ed from the path the host gives (the copy torch bundles when torch
// is in the process, else /opt/rocm/lib/librccl.so): like the HIP runtime, there must
// be one copy per process.  Only the handful of entry points used here are declared;
// the types mirror rccl.h (ncclUniqueId = 128 opaque bytes passed by value).
struct NcclUniqueId {
    char internal[MXS_UNIQUE_ID_BYTES];
};
struct Rccl {
    void* handle = nullptr;
    int (*GetUniqueId)(NcclUniqueId*) = nullptr;
    int (*CommInitRank)(void**, int, NcclUniqueId, int) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*Send)(const void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*Recv)(void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
};
constexpr int NCCL_F32 = 7, NCCL_F64 = 8;  // ncclFloat32 / ncclFloat64 (rccl.h)

static const Rccl* load_rccl(const char* path, std::string& err) {
    static std::mutex mu;
    static std::map<std::string, std::unique_ptr<Rccl>> libs;
    const std::string key = path && *path ? path : "librccl.so";
    std::lock_guard<std::mutex> lock(mu);
    auto it = libs.find(key);
    if (it != libs.end()) return it->second.get();
    std::unique_ptr<Rccl> r(new Rccl());
    r->handle = dlopen(key.c_str(), RTLD_NOW | RTLD_GLOBAL);
    if (!r->handle) {
        const char* m = dlerror();
        err = "cannot load RCCL (" + key + "): " + (m ? m : "?");
        return nullptr;
    }
    bool ok = true;
    auto sym = [&](const char* name) {
        void* p = dlsym(r->handle, name);
        if (!p) {
            ok = false;
            err = std::string("RCCL library misses ") + name;
        }
        return p;
    };
    r->GetUniqueId = (int (*)(NcclUniqueId*))sym("ncclGetUniqueId");
    r->CommInitRank = (int (*)(void**, int, NcclUniqueId, int))sym("ncclCommInitRank");
    r->CommDestroy = (int (*)(void*))sym("ncclCommDestroy");
    r->Send = (int (*)(const void*, size_t, int, int, void*, hipStream_t))sym("ncclSend");
    r->Recv = (int (*)(void*, size_t, int, int, void*, hipStream_t))sym("ncclRecv");
    r->GroupStart = (int (*)())sym("ncclGroupStart");
    r->GroupEnd = (int (*)())sym("ncclGroupEnd");
    r->GetErrorString = (const char* (*)(int))sym("ncclGetErrorString");
    if (!ok) return nullptr;
    const Rccl* out = r.get();
    libs[key] = std::move(r);
    return out;
}

#define NCCL_TRY(expr)                                                                      \
    do {                                                                                    \
        int _r = (expr);                                                                    \
        if (_r != 0)                                                                        \
            return fail(MXS_E_COMM, std::string(#expr) + ": " + rccl->GetErrorString(_r));  \
    } while (0)

template <typename U>
struct DevBuf {
    U* p = nullptr;
    size_t n = 0;
    hipError_t alloc(size_t count) {
        if (p) (void)hipFree(p);  // re-allocation (e.g. a second attempt at setting an exchange up)
        p = nullptr;
        n = count;
        return hipMalloc((void**)&p, std::max<size_t>(count, 1) * sizeof(U));
    }
    // Copies go through the engine's own (non-blocking) stream so that they are
    // ordered with its kernels; the host vector may die right after the call.
    hipError_t upload(const std::vector<U>& h, hipStream_t st) {
        hipError_t e = alloc(h.size());
        if (e != hipSuccess || h.empty()) return e;
        e = hipMemcpyAsync(p, h.data(), h.size() * sizeof(U), hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return e;
        return hipStreamSynchronize(st);
    }
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
};

struct EngineBase {
    virtual ~EngineBase() {}
    virtual int init(const mxs_graph& g, const mxs_params& p, int device) = 0;
    virtual int reset() = 0;
    virtual int run_async(int n) = 0;
    virtual int sync() = 0;
    virtual int run_timed(int n, float* ms) = 0;
    virtual int run_reps(int n, int reps, float* ms) = 0;
    virtual int get_assignment(int32_t* idx, double* belief) = 0;
    virtual int get_messages(double* v2f, double* f2v, uint8_t* cv, uint8_t* cf) = 0;
    virtual int set_state(const double* v2f, const double* f2v, const uint8_t* cv, const uint8_t* cf,
                          const int32_t* idx, const double* belief, int64_t cyc) = 0;
    virtual int eval_cost(const int32_t* idx, double infinity, double* cost, int64_t* viol) = 0;
    virtual int halo_setup(const int32_t* se, int64_t ns, const int32_t* re, int64_t nr) = 0;
    virtual int halo_buffers(void** s, int64_t* sb, void** r, int64_t* rb) = 0;
    virtual int halo_bind(void* s, void* r) = 0;
    virtual int step_compute() = 0;
    virtual int step_pack() = 0;
    virtual int step_unpack() = 0;
    virtual int comm_init(const char* path, int rank, int world, const uint8_t* id,
                          const int64_t* sc, const int64_t* rc) = 0;
    virtual int comm_exchange() = 0;
    virtual int run_sharded(int n) = 0;
    virtual void shard_mode(int32_t* f, int32_t* d) const = 0;
    virtual int peer_export(int rank, int world, const int64_t* sc, const int64_t* rc, mxs_peer_info* out) = 0;
    virtual int peer_connect(const mxs_peer_info* all) = 0;
    virtual bool peer_mode() const = 0;
    virtual int debug_timeline(int64_t* out, int32_t cap, int32_t* n_blocks) = 0;
    virtual int update_table(int32_t factor, const double* table, int64_t n) = 0;
    virtual int set_parent(int32_t factor, const double* parent, int32_t nd, const int32_t* dims, const uint8_t* ext) = 0;
    virtual int slice_factor(int32_t factor, const int32_t* ext_idx) = 0;
    // best state and cost trace on the device (include/maxsum_gpu_anytime.h)
    virtual int track_best(int32_t every, double infinity, int32_t trace_cap) = 0;
    virtual int get_best(int64_t* cycle, double* cost, int64_t* viol, int32_t* idx) = 0;
    virtual int get_cost_trace(int64_t* cycle, double* cost, int64_t* viol, int32_t cap, int32_t* n, int64_t* evals) = 0;
    virtual int track_restart() = 0;  // the state or the cost function has changed: the record starts again from here
    virtual bool tracking() const = 0;
    // the end condition on the device (include/maxsum_gpu_quiescence.h)
    virtual int watch_quiescence(int32_t every) = 0;
    virtual int quiescence(int32_t* quiescent, int64_t* cycle, int64_t* checks, int64_t* active, int64_t* last_check) = 0;
    virtual int run_until_quiescent(int32_t max_cycles, int32_t poll, int32_t* quiescent, int64_t* cycle, int64_t* ran) = 0;
    virtual int quiet_restart() = 0;  // the state or the cost function has changed: the fixed point no longer holds
    virtual bool watching() const = 0;
    Layout L;
    mxs_params params{};
    int64_t cycles = 0;
    hipStream_t stream = nullptr;  // compute stream
    hipStream_t comm = nullptr;    // sharded operation: pack / collective / unpack
    int launches_per_cycle = 1;
};

template <typename T>
struct Engine : EngineBase {
    int device = 0;
    int cur = 0;  // buffers holding the messages of the last finished cycle
    DevBuf<T> v2f[2], f2v[2], tables, var_cost, belief, halo_send, halo_recv;
    DevBuf<uint8_t> cF, cV, owned, fowned;
    DevBuf<int32_t> vrowptr, vdom, init_idx, edge_gen_factor, edge_dom, sel, vell;
    DevBuf<WaveMeta> vwave;
    DevBuf<int32_t> edge_v2f, f2v_off, vslot_f2v, vslot_v2f;
    DevBuf<int32_t> frowptr, edge_var_int, eval_idx;
    DevBuf<int64_t> vcost_off, eval_tab_off, halo_send_off, halo_recv_off, timeline;
    bool timeline_on = false;
    DevBuf<FactorGen> fgen;
    DevBuf<uint32_t> sched;     // block schedule of launch 0 (Layout::sched), may be empty
    DevBuf<uint8_t> ctables;    // compact table records (Layout::ctables), may be empty
    size_t ctables_used = 0;    // bytes of it that hold images once append_bin2_full_image has grown it (0: ctables.n)
    DevBuf<ClassInfo> classes;  // sweep classes in launch order
    DevBuf<ClassInfo> classes2; // cut factor classes (second sweep launch of a sharded cycle)
    DevBuf<ClassInfo> classes_f; // both lists as ONE grid (fused sharded launch), cut classes last
    DevBuf<ClassInfo> classes8;  // the K_V_PACK8 class (its own launch)
    DevBuf<uint32_t> halo_flags; // [0] exchanges unpacked so far, [1] error bits, [2] unpack block counter
    bool fused = false;          // sharded cycles use the fused launch
    uint32_t unpacks = 0;        // unpack kernels enqueued since the last reset
    DevBuf<NaryDesc> ndesc;
    DevBuf<WideBlock> wide_blocks;
    DevBuf<HubBlock> hub_blocks;
    bool has_hub = false;        // a K_V_HUB class rides in the sweep launch: the k_sweep_hub instantiations
#ifdef MXS_WIDE_PROFILE
    DevBuf<int64_t> wide_prof;
#endif
    DevBuf<double> eval_tables, eval_var_cost, part_cost;
    DevBuf<unsigned long long> part_viol;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // The wide variable kernels (latency-bound, few waves) and the workgroup-per-factor launches
    // (compute-bound since their tables are narrow) of one cycle read the same old buffers and
    // write disjoint new ones (Jacobi): the wide kernels go to a side stream and run beside the
    // n-ary launches.  Eager launches only; $MAXSUM_NARY_OVERLAP=0 keeps one stream.
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    bool overlap = false, capturing = false;
    bool streaming = false;  // non-temporal stores / index loads in the sweep (cycle larger than the Infinity Cache)
    hipEvent_t ev_p1 = nullptr;    // phase 1 of the current cycle enqueued (variables are done)
    hipEvent_t ev_halo = nullptr;  // ghost messages of the last exchange are in place
    bool halo_pending = false;
    hipGraphExec_t graph_exec = nullptr;
    int graph_cycles = 0;  // cycles per replay (even), 0 = no graph
    bool graph_tried = false;
    int64_t n_halo_send = 0, n_halo_recv = 0;
    T* send_buf = nullptr;  // packed staging buffers: the engine's own (halo_send /
    T* recv_buf = nullptr;  // halo_recv) or caller-owned memory (mxs_halo_bind)
    bool halo_ready = false;
    static constexpr int EVAL_BLOCKS = 1024;
    static_assert(EVAL_BLOCKS <= ANY_MAX_PARTS, "k_any_final stages every partial of k_eval in LDS");
    // mxs_track_best: the best state and the cost trace, on the device (anytime.h)
    struct Anytime {
        bool on = false;
        int every = 0;         // evaluate after every cycle c with c % every == 0
        double infinity = 0;
        int graph_phase = 0;   // cycle count % every at the start of the captured chunk
        DevBuf<AnyState> st;
        DevBuf<int32_t> snap;  // [n_vars] internal order
        DevBuf<long long> tr_cycle, tr_viol;
        DevBuf<double> tr_cost;
    } any;
    // mxs_watch_quiescence: the end condition, on the device (quiescence.h)
    struct Quiet {
        bool on = false;
        int every = 0;        // check after every cycle c with c % every == 0 or c % every == 1
        int graph_phase = 0;  // cycle count % every at the start of the captured chunk
        int blocks = 1;       // the grid of k_quiet_count
        QuietLists lists{};   // (device pointers into `tiles` and `gather`)
        DevBuf<QuietState> st;
        DevBuf<QuietTile> tiles;
        DevBuf<uint32_t> gather, part;
    } quiet;
    static constexpr int FUSED_MAX_CUT_BLOCKS = 1024;  // half of the 2048 resident workgroup slots

    ~Engine() override {
        for (int q = 0; q < MXS_MAX_PEERS; ++q) {
            if (peer_local[q]) continue;
            if (peer_ghost[q]) (void)hipIpcCloseMemHandle(peer_ghost[q]);
            if (peer_flag[q]) (void)hipIpcCloseMemHandle(peer_flag[q]);
        }
        if (nccl_comm) {
            if (comm) (void)hipStreamSynchronize(comm);
            (void)rccl->CommDestroy(nccl_comm);
        }
#ifdef MXS_WIDE_PROFILE
        wide_profile_dump();
#endif
        if (graph_exec) (void)hipGraphExecDestroy(graph_exec);
        if (ev_fork) (void)hipEventDestroy(ev_fork);
        if (ev_join) (void)hipEventDestroy(ev_join);
        if (side) (void)hipStreamDestroy(side);
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (ev_p1) (void)hipEventDestroy(ev_p1);
        if (ev_halo) (void)hipEventDestroy(ev_halo);
        if (comm) (void)hipStreamDestroy(comm);
        if (stream) (void)hipStreamDestroy(stream);
    }

    SweepArgs<T> make_args(int from, bool start, int phase = 1) const {
        SweepArgs<T> a{};
        a.v2f_old = v2f[from].p;
        a.v2f_new = v2f[from ^ 1].p;
        a.f2v_old = f2v[from].p;
        a.f2v_new = f2v[from ^ 1].p;
        a.tables = tables.p;
        a.ctables = ctables.p;
        a.tab_neg = L.is_max ? 1 : 0;
        a.var_cost = var_cost.p;
        a.cF = cF.p;
        a.cV = cV.p;
        a.edge_v2f = edge_v2f.p;
        a.f2v_off = f2v_off.p;
        a.vrowptr = vrowptr.p;
        a.vslot_f2v = vslot_f2v.p;
        a.vslot_v2f = vslot_v2f.p;
        a.vell = vell.p;
        a.vwave = vwave.p;
        a.hub_blocks = hub_blocks.p;
        a.vdom = vdom.p;
        a.vcost_off = vcost_off.p;
        a.init_idx = init_idx.p;
        a.fgen = fgen.p;
        a.edge_gen_factor = edge_gen_factor.p;
        a.edge_dom = edge_dom.p;
        a.sel = sel.p;
        a.belief = belief.p;
        a.damping = (T)params.damping;
        a.stability = (T)params.stability;
        a.damp_f = (params.damping_nodes & MXS_DAMP_FACTORS) ? 1 : 0;
        a.damp_v = (params.damping_nodes & MXS_DAMP_VARS) ? 1 : 0;
        a.start = start ? 1 : 0;
        a.start_mode = params.start_messages;
        a.null_f2v = (int32_t)L.null_f2v;
        a.timeline = timeline_on ? timeline.p : nullptr;
#ifdef MXS_WIDE_PROFILE  // profiling build (make variant DEFS=-DMXS_WIDE_PROFILE): phase clocks of k_variable_wide
        if (!timeline_on) a.timeline = wide_prof.p;
#endif
        a.halo_flags = nullptr;
        a.need_epoch = 0;
        a.send_out = direct ? send2[from ^ 1].p : nullptr;  // the parity this cycle writes
        a.send_slot = direct ? send_slot.p : nullptr;
        a.n_peers = 0;
        a.me = comm_rank;
        a.ghost_lo = INT32_MAX;
        a.ghost_old = nullptr;
        for (int q = 0; q < MXS_MAX_PEERS; ++q) {
            a.peer_first[q] = INT32_MAX;
            a.peer_dst[q] = nullptr;
        }
        if (p2p) {
            // this launch becomes publish number gen + 1: it reads the records of publish `gen`
            // (ghost region gen % 3; all zeros in the start cycle, like every other message) and
            // stores its own into region (gen + 1) % 3 of the peers
            a.n_peers = comm_world;
            a.ghost_lo = (int32_t)L.v2f_elems;
            a.ghost_old = start ? ghost3.p + 3 * ghost_len : ghost3.p + (int64_t)(gen % 3) * ghost_len;
            a.send_slot = send_slot.p;
            a.send_out = nullptr;
            for (int q = 0; q < comm_world; ++q) {
                a.peer_first[q] = peer_first[q];
                a.peer_dst[q] = peer_ghost[q] ? peer_ghost[q] + (int64_t)((gen + 1) % 3) * peer_len[q] + peer_at[q] : nullptr;
            }
        }
        if (phase == 3) {  // fused sharded launch: phase-1 classes, then the cut factor classes
            a.n_classes = (int32_t)L.fused_block_base.size();
            for (int i = 0; i < MAX_CLASSES; ++i)
                a.block_base[i] = i < a.n_classes ? L.fused_block_base[i] : INT32_MAX;
            a.classes = classes_f.p;
            a.halo_flags = halo_flags.p;
            a.need_epoch = p2p ? gen : unpacks;  // every exchange enqueued so far has to be in place
            return a;
        }
        const std::vector<int32_t>& order = phase == 1 ? L.sweep_order : L.sweep_order2;
        a.n_classes = (int32_t)order.size();
        for (int i = 0; i < MAX_CLASSES; ++i)
            a.block_base[i] = i < a.n_classes ? L.classes[order[i]].block_base : INT32_MAX;
        a.classes = phase == 1 ? classes.p : classes2.p;
        a.sched = (phase == 1 && !L.sched.empty()) ? sched.p : nullptr;
        return a;
    }

    int launch_sweep(const SweepArgs<T>& a, int nb) {
        if (nb <= 0) return MXS_OK;
        const dim3 grid(nb), block(BLOCK);
        if (p2p) {  // peer-store twin
            switch (L.dsel) {
                case 2: hipLaunchKernelGGL((k_sweep_p2p<T, 2>), grid, block, 0, stream, a); break;
                case 3: hipLaunchKernelGGL((k_sweep_p2p<T, 3>), grid, block, 0, stream, a); break;
                case 4: hipLaunchKernelGGL((k_sweep_p2p<T, 4>), grid, block, 0, stream, a); break;
                default: hipLaunchKernelGGL((k_sweep_p2p<T, 0>), grid, block, 0, stream, a); break;
            }
        } else if (timeline_on && has_hub) {  // profiling twin, hub class on board
            if (L.dsel == 3) hipLaunchKernelGGL((k_sweep_timeline_hub<T, 3>), grid, block, 0, stream, a);
            else hipLaunchKernelGGL((k_sweep_timeline_hub<T, 0>), grid, block, 0, stream, a);
        } else if (timeline_on) {  // profiling twin
            switch (L.dsel) {
                case 2: hipLaunchKernelGGL((k_sweep_timeline<T, 2>), grid, block, 0, stream, a); break;
                case 3: hipLaunchKernelGGL((k_sweep_timeline<T, 3>), grid, block, 0, stream, a); break;
                case 4: hipLaunchKernelGGL((k_sweep_timeline<T, 4>), grid, block, 0, stream, a); break;
                default: hipLaunchKernelGGL((k_sweep_timeline<T, 0>), grid, block, 0, stream, a); break;
            }
        } else if (has_hub) {  // the instantiations that carry the hub class (kernels.h variable_hub): D = 3 or any
#define MXS_SWEEP_HUB(DS)                                                                                          \
    do {                                                                                                           \
        if (streaming) {                                                                                           \
            if (a.sched) hipLaunchKernelGGL((k_sweep_hub<T, DS, NT_STREAMING, true>), grid, block, 0, stream, a);  \
            else hipLaunchKernelGGL((k_sweep_hub<T, DS, NT_STREAMING, false>), grid, block, 0, stream, a);         \
        } else {                                                                                                   \
            if (a.sched) hipLaunchKernelGGL((k_sweep_hub<T, DS, MXS_NT, true>), grid, block, 0, stream, a);        \
            else hipLaunchKernelGGL((k_sweep_hub<T, DS, MXS_NT, false>), grid, block, 0, stream, a);               \
        }                                                                                                          \
    } while (0)
            if (L.dsel == 3) MXS_SWEEP_HUB(3);
            else MXS_SWEEP_HUB(0);
#undef MXS_SWEEP_HUB
        } else {
            // <.., policy, schedule>: NT_STREAMING when the cycle does not fit the Infinity Cache (kernels.h);
            // the lean instantiation when the launch has a block schedule
#define MXS_SWEEP(DS)                                                                                          \
    do {                                                                                                       \
        if (streaming) {                                                                                       \
            if (a.sched) hipLaunchKernelGGL((k_sweep<T, DS, NT_STREAMING, true>), grid, block, 0, stream, a);  \
            else hipLaunchKernelGGL((k_sweep<T, DS, NT_STREAMING, false>), grid, block, 0, stream, a);         \
        } else {                                                                                               \
            if (a.sched) hipLaunchKernelGGL((k_sweep<T, DS, MXS_NT, true>), grid, block, 0, stream, a);        \
            else hipLaunchKernelGGL((k_sweep<T, DS, MXS_NT, false>), grid, block, 0, stream, a);               \
        }                                                                                                      \
    } while (0)
            switch (L.dsel) {
                case 2:  // its own kernel (SGPR budget, kernels.h)
                    if (streaming) {
                        if (a.sched) hipLaunchKernelGGL((k_sweep_d2<T, NT_STREAMING, true>), grid, block, 0, stream, a);
                        else hipLaunchKernelGGL((k_sweep_d2<T, NT_STREAMING, false>), grid, block, 0, stream, a);
                    } else {
                        if (a.sched) hipLaunchKernelGGL((k_sweep_d2<T, MXS_NT, true>), grid, block, 0, stream, a);
                        else hipLaunchKernelGGL((k_sweep_d2<T, MXS_NT, false>), grid, block, 0, stream, a);
                    }
                    break;
                case 3: MXS_SWEEP(3); break;
                case 4: MXS_SWEEP(4); break;
                default: MXS_SWEEP(0); break;
            }
#undef MXS_SWEEP
        }
        HIP_TRY(hipGetLastError());
        return MXS_OK;
    }

    // Is the block size of the launch group a multiple of the LAST dimension of every factor in it
    // (kernels.h, nary_batch: LS)?  Looked at once per group (the groups change only in widen_factor).
    std::vector<int8_t> nary_ls_cache;
    bool nary_last_same(const NaryLaunch& nl) {
        const size_t idx = (size_t)(&nl - L.nary_launches.data());
        if (nary_ls_cache.size() != L.nary_launches.size()) nary_ls_cache.assign(L.nary_launches.size(), -1);
        if (nary_ls_cache[idx] < 0) {
            int8_t ok = 1;
            for (int j = 0; j < nl.count && ok; ++j) {
                const NaryDesc& d = L.ndesc[nl.first + j];
                if (nl.threads % d.dom[(d.arity & 255) - 1] != 0) ok = 0;
            }
            nary_ls_cache[idx] = ok;
        }
        return nary_ls_cache[idx] == 1;
    }

    // The largest scope (sum of domain sizes) of a launch group, rounded up to an even number of elements: what its blocks'
    // LDS arrays are sized for (looked at once per group).
    std::vector<int32_t> nary_cap_cache;
    int nary_group_cap(const NaryLaunch& nl) {
        const size_t idx = (size_t)(&nl - L.nary_launches.data());
        if (nary_cap_cache.size() != L.nary_launches.size()) nary_cap_cache.assign(L.nary_launches.size(), -1);
        if (nary_cap_cache[idx] < 0) {
            int cap = 2;
            for (int j = 0; j < nl.count; ++j) {
                const NaryDesc& d = L.ndesc[nl.first + j];
                int sumd = 0;
                for (int i = 0; i < (d.arity & 255); ++i) sumd += d.dom[i];
                cap = std::max(cap, sumd);
            }
            nary_cap_cache[idx] = (cap + 1) & ~1;
        }
        return nary_cap_cache[idx];
    }

    // the launch group of a workgroup-per-factor factor
    const NaryLaunch* launch_of(int fi) const {
        for (const NaryLaunch& x : L.nary_launches)
            if (L.f_ndesc[fi] >= x.first && L.f_ndesc[fi] < x.first + x.count) return &x;
        return nullptr;
    }

    // The launch group the K_V_PACK8 variable class rides in (its workgroups become the first ones of that grid): the
    // LARGEST lane-grid group that reads no ghost -- -1: none, the class has a launch of its own.  (Two latency-bound launches
    // of a cache-resident cycle overlap only inside one grid: on two streams coloring_100k_d8 runs 59-61 us against 51.8 one
    // after the other, the fork / join events cost more than the overlap hides -- profiles/r05_d8_overlap_ab_v1.txt.)
    int pack8_host_group() const {
        if (L.pack8_classes.empty() || !L.opt.pack8_fused) return -1;
        if (params.layout_flags & (32 | 64)) return -1;  // (one-side timing experiments: the class keeps a launch of its own)
        int best = -1;
        for (size_t i = 0; i < L.nary_launches.size(); ++i) {
            const NaryLaunch& nl = L.nary_launches[i];
            if (!is_bin2(nl.box) || nl.cut) continue;
            if (best < 0 || nl.count > L.nary_launches[best].count) best = (int)i;
        }
        return best;
    }

    int launch_nary(const SweepArgs<T>& a, int cut) {
        const int host8 = cut == 0 ? pack8_host_group() : -1;
        for (const NaryLaunch& nl : L.nary_launches) {
            if (nl.cut != cut) continue;
            const NaryDesc* d = ndesc.p + nl.first;
            if (is_bin2(nl.box)) {  // binary / unary tables: a lane grid per factor (bin_box.h)
                const bool host = host8 >= 0 && &nl == &L.nary_launches[host8];
                const int nb8 = host ? (L.classes[L.pack8_classes[0]].count + BLOCK - 1) / BLOCK : 0;
                if (!launch_factor_bin2<T>(nl, a, d, stream, host ? (const ClassInfo*)classes8.p : nullptr, nb8))
                    return fail(MXS_E_STATE, "no lane-grid kernel for this launch group");
                HIP_TRY(hipGetLastError());
                continue;
            }
            if (is_small(nl.box)) {  // arity 3..5 over small domains: a lane group per factor (small_box.h)
                if (!launch_factor_small<T>(nl, a, d, stream)) return fail(MXS_E_STATE, "no small-domain kernel for this launch group");
                HIP_TRY(hipGetLastError());
                continue;
            }
            if (nl.box) {  // one wave per factor, minima in registers (nary_box.h)
                if (!launch_factor_box3<T>(nl, a, d, stream)) return fail(MXS_E_STATE, "no box kernel for this launch group");
                HIP_TRY(hipGetLastError());
                continue;
            }
            const dim3 grid((unsigned)nl.count), block((unsigned)nl.threads);
            const bool ls = nary_last_same(nl);
            // LDS of a block: three arrays as long as the group's largest scope (sum of its domain sizes), in 8-byte words
            const int cap = nary_group_cap(nl);
            const size_t lds = (size_t)3 * cap * 8;
#define MXS_NARY_PACKED(AR, NJ, TT)                                                                                                        \
    do {                                                                                                                                   \
        if (AR == 3 && ls) {  /* kernels.h, nary_batch: LS */                                                                              \
            if (a.tab_neg) hipLaunchKernelGGL((k_factor_nary_packed<T, AR, NJ, TT, true, AR == 3>), grid, block, lds, stream, a, d, cap);  \
            else hipLaunchKernelGGL((k_factor_nary_packed<T, AR, NJ, TT, false, AR == 3>), grid, block, lds, stream, a, d, cap);           \
        } else if (a.tab_neg) hipLaunchKernelGGL((k_factor_nary_packed<T, AR, NJ, TT, true>), grid, block, lds, stream, a, d, cap);        \
        else hipLaunchKernelGGL((k_factor_nary_packed<T, AR, NJ, TT, false>), grid, block, lds, stream, a, d, cap);                        \
    } while (0)
#define MXS_NARY_CASE(AR, NJ)                                                                      \
    case (AR) * 16 + (NJ):                                                                         \
        if (nl.tab_type == TAB_I8) MXS_NARY_PACKED(AR, NJ, int8_t);                                \
        else if (nl.tab_type == TAB_I16) MXS_NARY_PACKED(AR, NJ, int16_t);                         \
        else if (nl.tab_type == TAB_F32) MXS_NARY_PACKED(AR, NJ, float);                           \
        else hipLaunchKernelGGL((k_factor_nary<T, AR, NJ>), grid, block, lds, stream, a, d, cap);  \
        break;
            if (nl.nj == NARY_NJ_MULTI) {  // full-width tables in passes of NARY_MAX_R entries per value of the first variable
#define MXS_NARY_MULTI(AR)                                                                                                                     \
    case AR:                                                                                                                                   \
        if (nl.tab_type == TAB_I8) {                                                                                                           \
            if (a.tab_neg) hipLaunchKernelGGL((k_factor_nary<T, AR, NARY_MAX_NJ, true, int8_t, true>), grid, block, lds, stream, a, d, cap);   \
            else hipLaunchKernelGGL((k_factor_nary<T, AR, NARY_MAX_NJ, true, int8_t, false>), grid, block, lds, stream, a, d, cap);            \
        } else if (nl.tab_type == TAB_I16) {                                                                                                   \
            if (a.tab_neg) hipLaunchKernelGGL((k_factor_nary<T, AR, NARY_MAX_NJ, true, int16_t, true>), grid, block, lds, stream, a, d, cap);  \
            else hipLaunchKernelGGL((k_factor_nary<T, AR, NARY_MAX_NJ, true, int16_t, false>), grid, block, lds, stream, a, d, cap);           \
        } else if (nl.tab_type == TAB_FULL) {                                                                                                  \
            hipLaunchKernelGGL((k_factor_nary<T, AR, NARY_MAX_NJ, true>), grid, block, lds, stream, a, d, cap);                                \
        } else {                                                                                                                               \
            return fail(MXS_E_STATE, "no multi-pass n-ary kernel for this storage type");                                                      \
        }                                                                                                                                      \
        break;
                switch (nl.arity) {
                    MXS_NARY_MULTI(3) MXS_NARY_MULTI(4) MXS_NARY_MULTI(5) MXS_NARY_MULTI(6)
                    default: return fail(MXS_E_STATE, "no multi-pass n-ary kernel for this arity");
                }
#undef MXS_NARY_MULTI
                HIP_TRY(hipGetLastError());
                continue;
            }
            switch (nl.arity * 16 + nl.nj) {
                MXS_NARY_CASE(2, 1) MXS_NARY_CASE(2, 2) MXS_NARY_CASE(2, 3) MXS_NARY_CASE(2, 4)
                MXS_NARY_CASE(3, 1) MXS_NARY_CASE(3, 2) MXS_NARY_CASE(3, 3) MXS_NARY_CASE(3, 4)
                MXS_NARY_CASE(4, 1) MXS_NARY_CASE(4, 2) MXS_NARY_CASE(4, 3) MXS_NARY_CASE(4, 4)
                MXS_NARY_CASE(5, 1) MXS_NARY_CASE(5, 2) MXS_NARY_CASE(5, 3) MXS_NARY_CASE(5, 4)
                default: return fail(MXS_E_STATE, "no n-ary kernel for this (arity, size) group");
            }
#undef MXS_NARY_CASE
#undef MXS_NARY_PACKED
            HIP_TRY(hipGetLastError());
        }
        return MXS_OK;
    }

    // The wide variable class (k_variable_wide: a workgroup per run of variables of one domain size) and the
    // lane-per-edge class of the domains of 5..8 values (k_variable_pack8).
    int launch_wide(const SweepArgs<T>& a, hipStream_t ws) {
        if (!L.pack8_classes.empty() && pack8_host_group() < 0) {
            const ClassInfo& ci = L.classes[L.pack8_classes[0]];
            hipLaunchKernelGGL((k_variable_pack8<T>), dim3((unsigned)((ci.count + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, ws, a,
                               (const ClassInfo*)classes8.p);
            HIP_TRY(hipGetLastError());
        }
        if (!L.wide_blocks.empty()) {
            hipLaunchKernelGGL((k_variable_wide<T>), dim3((unsigned)L.wide_blocks.size()), dim3(WIDE_TPB), 0, ws, a,
                               (const WideBlock*)wide_blocks.p);
            HIP_TRY(hipGetLastError());
        }
        return MXS_OK;
    }
    int n_wide_launches() const { return (L.wide_blocks.empty() ? 0 : 1) + ((L.pack8_classes.empty() || pack8_host_group() >= 0) ? 0 : 1); }

    // Enqueue (part of) one cycle reading buffer `from` on the compute stream.
    //   phase 1: every variable class and every factor class that reads owned variables only
    //   phase 2: the cut factor classes of a shard (they read ghost messages, i.e. they are
    //            the only work that depends on the halo exchange of the previous cycle)
    // A single-GPU engine has no phase-2 work.
    int launch_phase(int from, bool start, int phase) {
        const SweepArgs<T> a = make_args(from, start, phase);
        if (phase == 3) {  // everything of the cycle; the cut factor blocks wait inside the sweep
            int rc = launch_sweep(a, L.n_blocks_fused);
            if (rc) return rc;
            { int rc2 = launch_wide(a, stream); if (rc2) return rc2; }
            return launch_nary(a, 0);
        }
        if (phase == 1) {
            // isolated variables only act in cycle 0
            int rc = launch_sweep(a, (start || L.sweep_regular) ? L.n_blocks_sweep : 0);
            if (rc) return rc;
            // (timing experiments, results wrong: layout_flags bit5 = variable side only, bit6 = factor side only -- the launches
            // outside the sweep honour them too)
            const bool vars_only = (params.layout_flags & 32) != 0, factors_only = (params.layout_flags & 64) != 0;
            if (vars_only || factors_only) {
                if (!factors_only) { rc = launch_wide(a, stream); if (rc) return rc; }
                return vars_only ? MXS_OK : launch_nary(a, 0);
            }
            const bool fork = overlap && !capturing && n_wide_launches() > 0 && !L.nary_launches.empty();
            hipStream_t ws = stream;
            if (fork) {  // the side stream starts where the compute stream is now
                HIP_TRY(hipEventRecord(ev_fork, stream));
                HIP_TRY(hipStreamWaitEvent(side, ev_fork, 0));
                ws = side;
            }
            rc = launch_wide(a, ws);
            if (rc) return rc;
            if (fork) HIP_TRY(hipEventRecord(ev_join, side));
            rc = launch_nary(a, 0);
            if (rc) return rc;
            if (fork) HIP_TRY(hipStreamWaitEvent(stream, ev_join, 0));  // the cycle ends when both have
            return MXS_OK;
        }
        int rc = launch_sweep(a, L.n_blocks_sweep2);
        if (rc) return rc;
        return launch_nary(a, 1);
    }

    int launch_cycle(int from, bool start) {
        int rc = launch_phase(from, start, 1);
        if (rc) return rc;
        return launch_phase(from, start, 2);
    }

    // The ClassInfo arrays of the three launch flavours (from L.classes).
    int upload_class_arrays() {
        std::vector<ClassInfo> order;
        for (int c : L.sweep_order) order.push_back(L.classes[c]);
        HIP_TRY(classes.upload(order, stream));
        order.clear();
        for (int c : L.sweep_order2) order.push_back(L.classes[c]);
        HIP_TRY(classes2.upload(order, stream));
        order.clear();
        if (L.n_blocks_fused > 0) {
            for (int c : L.sweep_order) order.push_back(L.classes[c]);
            for (int c : L.sweep_order2) order.push_back(L.classes[c]);
            for (size_t i = 0; i < order.size(); ++i) order[i].block_base = L.fused_block_base[i];
        }
        HIP_TRY(classes_f.upload(order, stream));
        order.clear();
        for (int c : L.pack8_classes) order.push_back(L.classes[c]);
        HIP_TRY(classes8.upload(order, stream));
        return MXS_OK;
    }

    // A new table entry does not fit the narrow type a class stores its tables in: from now on
    // the class reads the full-width image, which every update keeps current.
    int promote_class(int cls) {
        if (L.classes[cls].tab_type == TAB_FULL) return MXS_OK;
        { int rc = sync(); if (rc) return rc; }
        L.classes[cls].tab_type = TAB_FULL;
        for (int fi = 0; fi < L.n_factors; ++fi)
            if (L.f_class[fi] == cls) L.f_tab_type[fi] = (uint8_t)TAB_FULL;
        if (graph_exec) {  // the captured cycle loop holds the pointers of the old class arrays
            (void)hipGraphExecDestroy(graph_exec);
            graph_exec = nullptr;
            graph_tried = false;
        }
        return upload_class_arrays();
    }

    // Factor fi can no longer be read from its narrow image: a register class goes back to full
    // width as a whole; a workgroup-per-factor factor just gets its descriptor switched.
    int widen_factor(int fi, const double* values = nullptr) {
        if (L.f_tab_type[fi] == TAB_FULL) return MXS_OK;
        if (L.f_class[fi] >= 0) return promote_class(L.f_class[fi]);
        { int rc = sync(); if (rc) return rc; }
        int64_t bin2_at = -1;  // a lane-grid factor: its new full-width image (bin_box.h reads an image at every width)
        if (const NaryLaunch* nl = launch_of(fi); nl && is_bin2(nl->box)) {
            int rc = append_bin2_full_image(fi, *nl, values, &bin2_at);
            if (rc) return rc;
        }
        // the factor moves to the full-width launch group of its (arity, size): regroup the
        // descriptors (stable: every other factor keeps its relative place)
        struct Item { int cut, code, type, fi; NaryDesc d; };
        std::vector<int> fi_of(L.ndesc.size(), -1);
        for (int f2 = 0; f2 < L.n_factors; ++f2)
            if (L.f_ndesc[f2] >= 0) fi_of[L.f_ndesc[f2]] = f2;
        std::vector<Item> items;
        for (const NaryLaunch& nl : L.nary_launches)
            for (int j = 0; j < nl.count; ++j) {
                Item it{nl.cut, nary_group_code(nl.box, nl.arity, nl.nj, nl.threads / 64), nl.tab_type, fi_of[nl.first + j],
                        L.ndesc[nl.first + j]};
                if (it.fi == fi && bin2_at >= 0) {  // (the same lane grid, reading the full-width image)
                    it.type = TAB_FULL;
                    it.d.tab_off = bin2_at;
                } else if (it.fi == fi) {  // (out of a box group: the full-width kernel's group of its size)
                    it.type = TAB_FULL;
                    it.d.tab_off = L.f_tab_base[fi];
                    int64_t R = 1;
                    for (int i = 1; i < nl.arity; ++i) R *= it.d.dom[i];
                    // (a multi-pass group keeps its kernel: only the storage type changes)
                    if (!(nl.box == 0 && nl.nj == NARY_NJ_MULTI)) it.code = nary_group_code(0, nl.arity, nary_classic_nj(R), nary_classic_waves(R));
                }
                items.push_back(it);
            }
        std::stable_sort(items.begin(), items.end(), [](const Item& x, const Item& y) {
            return x.cut != y.cut ? x.cut < y.cut : x.code != y.code ? x.code < y.code : x.type < y.type;
        });
        L.ndesc.clear();
        L.nary_launches.clear();
        nary_ls_cache.clear();
        nary_cap_cache.clear();
        for (size_t i = 0; i < items.size(); ++i) {
            const Item& it = items[i];
            if (i == 0 || it.cut != items[i - 1].cut || it.code != items[i - 1].code || it.type != items[i - 1].type)
                L.nary_launches.push_back(NaryLaunch{(it.code / 256) % 16, (it.code / 16) % 16, (it.code % 16) * 64,
                                                     (int32_t)i, 0, it.cut, it.type, it.code / 4096});
            L.nary_launches.back().count += 1;
            L.f_ndesc[it.fi] = (int32_t)i;
            L.ndesc.push_back(it.d);
        }
        L.f_tab_type[fi] = (uint8_t)TAB_FULL;
        if (bin2_at >= 0) L.f_ctab_off[fi] = bin2_at;
        if (graph_exec) {  // the captured loop has the old launch groups
            (void)hipGraphExecDestroy(graph_exec);
            graph_exec = nullptr;
            graph_tried = false;
        }
        HIP_TRY(ndesc.upload(L.ndesc, stream));
        launches_per_cycle = ((L.n_blocks_sweep > 0 && L.sweep_regular) ? 1 : 0) + (L.n_blocks_sweep2 > 0 ? 1 : 0) +
                             (int)L.nary_launches.size() + n_wide_launches();
        return MXS_OK;
    }

    int init(const mxs_graph& g, const mxs_params& p, int dev) override {
        params = p;
        device = dev;
        std::string e = build_layout(g, p, L);
        if (!e.empty()) return fail(MXS_E_INVALID, e);
        // hipGraph replay pays off only when a cycle is shorter than a launch: measured on
        // MI355X it changes nothing from 8 MB per cycle up (7.8 vs 7.9 us at 10k variables,
        // 26.8 vs 27.1 at 100k) and SLOWS long kernels down (Ising 1024^2: 182 vs 133 us,
        // 1M-variable colouring 434 vs 370 us, meeting_50k 1351 vs 1176 us per cycle).
        // Default (graph_chunk < 0): graphs of 32 cycles below 4 MB per cycle, eager above.
        if (params.graph_chunk < 0) params.graph_chunk = L.algorithmic_bytes < (4 << 20) ? 32 : 0;
        {   // cache policy of the sweep: streaming (nt stores, nt index loads) once a cycle moves more
            // than the 256-MB Infinity Cache holds; MAXSUM_STREAMING=0/1 forces it (A/B runs)
            streaming = L.algorithmic_bytes > ((int64_t)256 << 20);
            const char* env = getenv("MAXSUM_STREAMING");
            if (env && (env[0] == '0' || env[0] == '1')) streaming = env[0] == '1';
        }
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
            return fail(MXS_E_NODEVICE, "no HIP device visible: the Max-Sum engine has no CPU fallback");
        if (dev < 0 || dev >= count) return fail(MXS_E_INVALID, "device index out of range");
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, dev));
        if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos)
            return fail(MXS_E_NODEVICE, std::string("device is ") + prop.gcnArchName +
                                            ", this library is built for gfx950 (MI355X) only");
        HIP_TRY(hipSetDevice(dev));
        HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        HIP_TRY(hipEventCreate(&ev0));
        HIP_TRY(hipEventCreate(&ev1));
        HIP_TRY(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&ev_join, hipEventDisableTiming));
        {   // Two streams pay when a cycle is long: measured (profiles/r05_variable_wave_ab_v1.txt, flags=1048576 rows =
            // this code) peav_50k 218.6 -> 205.5 us (f32 151.0 -> 136.1), meeting_50k 252.6 -> 249.4, but the
            // cache-resident coloring_100k_d8 53.3 -> 64.2 us (f32 42.8 -> 53.6): two latency-bound launches of full
            // occupancy only get in each other's way, and the fork / join events are not free.  Default: from 400 MB per
            // cycle on; $MAXSUM_NARY_OVERLAP=0/1 forces it.
            const char* env = getenv("MAXSUM_NARY_OVERLAP");
            overlap = L.algorithmic_bytes >= ((int64_t)400 << 20);
            if (env && (env[0] == '0' || env[0] == '1')) overlap = env[0] == '1';
        }
        {   // the comm stream's kernels (pack, RCCL, unpack) go first whenever a slot frees up
            int lo = 0, hi = 0;
            HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
            HIP_TRY(hipStreamCreateWithPriority(&comm, hipStreamNonBlocking, hi));
        }
        HIP_TRY(hipEventCreateWithFlags(&ev_p1, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&ev_halo, hipEventDisableTiming));

        auto conv = [](const std::vector<double>& src) {
            std::vector<T> out(src.size());
            for (size_t i = 0; i < src.size(); ++i) out[i] = (T)src[i];
            return out;
        };
        for (int b = 0; b < 2; ++b) {
            HIP_TRY(v2f[b].alloc((size_t)L.v2f_elems));
            HIP_TRY(f2v[b].alloc((size_t)L.f2v_elems));
        }
        HIP_TRY(edge_v2f.upload(L.v2f_off, stream));
        HIP_TRY(f2v_off.upload(L.f2v_off, stream));
        HIP_TRY(vslot_f2v.upload(L.vslot_f2v, stream));
        HIP_TRY(vslot_v2f.upload(L.vslot_v2f, stream));
        HIP_TRY(tables.upload(conv(L.tables), stream));
        HIP_TRY(ctables.upload(L.ctables, stream));
        HIP_TRY(var_cost.upload(conv(L.var_cost), stream));
        HIP_TRY(cF.alloc((size_t)L.n_edges));
        HIP_TRY(cV.alloc((size_t)L.n_cv));
        HIP_TRY(vell.upload(L.vell, stream));
        HIP_TRY(vwave.upload(L.vwave, stream));
        HIP_TRY(owned.upload(L.owned, stream));
        HIP_TRY(fowned.upload(L.fowned, stream));
        HIP_TRY(vrowptr.upload(L.vrowptr, stream));
        HIP_TRY(vdom.upload(L.vdom, stream));
        HIP_TRY(init_idx.upload(L.init_idx, stream));
        HIP_TRY(edge_gen_factor.upload(L.edge_gen_factor, stream));
        HIP_TRY(edge_dom.upload(L.edge_dom, stream));
        HIP_TRY(sel.alloc((size_t)L.n_vars));
        HIP_TRY(belief.alloc((size_t)L.n_vars));
        HIP_TRY(vcost_off.upload(L.vcost_off, stream));
        HIP_TRY(fgen.upload(L.fgen, stream));
        { int rc = upload_class_arrays(); if (rc) return rc; }
        HIP_TRY(sched.upload(L.sched, stream));
        HIP_TRY(halo_flags.alloc(64));
        HIP_TRY(ndesc.upload(L.ndesc, stream));
        HIP_TRY(wide_blocks.upload(L.wide_blocks, stream));
        HIP_TRY(hub_blocks.upload(L.hub_blocks, stream));
        has_hub = !L.hub_blocks.empty();
#ifdef MXS_WIDE_PROFILE
        if (!L.wide_blocks.empty()) {
            HIP_TRY(wide_prof.alloc(8 * L.wide_blocks.size()));
            HIP_TRY(hipMemset(wide_prof.p, 0, sizeof(int64_t) * 8 * L.wide_blocks.size()));
        }
#endif
        // solution_cost data
        HIP_TRY(frowptr.upload(L.frowptr, stream));
        HIP_TRY(edge_var_int.upload(L.edge_var_int, stream));
        HIP_TRY(eval_tab_off.upload(L.eval_tab_off, stream));
        HIP_TRY(eval_tables.upload(L.eval_tables, stream));
        HIP_TRY(eval_var_cost.upload(L.eval_var_cost, stream));
        HIP_TRY(eval_idx.alloc((size_t)L.n_vars));
        HIP_TRY(part_cost.alloc(EVAL_BLOCKS));
        HIP_TRY(part_viol.alloc(EVAL_BLOCKS));
        launches_per_cycle = ((L.n_blocks_sweep > 0 && L.sweep_regular) ? 1 : 0) + (L.n_blocks_sweep2 > 0 ? 1 : 0) +
                             (int)L.nary_launches.size() + n_wide_launches();
        return reset();
    }

    int reset() override {
        HIP_TRY(hipSetDevice(device));
        // Nothing enqueued before the reset may still write after the memsets below: an unpack
        // or a direct RCCL receive of the previous run (comm stream) would leave stale ghost
        // V->F messages where cycle 0 expects zeros.  Callers need not sync first.
        if (comm) HIP_TRY(hipStreamSynchronize(comm));
        HIP_TRY(hipStreamSynchronize(stream));
        for (int b = 0; b < 2; ++b) {
            HIP_TRY(hipMemsetAsync(v2f[b].p, 0, std::max<size_t>(v2f[b].n, 1) * sizeof(T), stream));
            HIP_TRY(hipMemsetAsync(f2v[b].p, 0, std::max<size_t>(f2v[b].n, 1) * sizeof(T), stream));
        }
        HIP_TRY(hipMemsetAsync(cF.p, 0, std::max<size_t>(cF.n, 1), stream));
        HIP_TRY(hipMemsetAsync(cV.p, 0, std::max<size_t>(cV.n, 1), stream));
        HIP_TRY(hipMemsetAsync(sel.p, 0, std::max<size_t>(sel.n, 1) * sizeof(int32_t), stream));
        HIP_TRY(hipMemsetAsync(belief.p, 0, std::max<size_t>(belief.n, 1) * sizeof(T), stream));
        if (!p2p) HIP_TRY(hipMemsetAsync(halo_flags.p, 0, 64 * sizeof(uint32_t), stream));  // (peers write a p2p shard's)
        unpacks = 0;
        cur = 0;
        cycles = 0;
        // cycle 0 == start() of every computation (computations.py:741-753)
        // (peer-store mode: the caller has made sure every rank is here -- no peer is still
        // running cycles of the previous run; the start cycle reads zeros for the ghosts and its
        // records are pushed afterwards, see p2p_push)
        int rc = p2p ? launch_phase(cur, true, 3) : launch_cycle(cur, true);
        if (rc) return rc;
        cur ^= 1;
        halo_pending = false;
        if (p2p) {  // the start launch has stored its records at the peers itself
            rc = p2p_publish();
            if (rc) return rc;
            return sync();
        }
        HIP_TRY(hipEventRecord(ev_p1, stream));
        if (halo_ready) {  // the start messages have to cross too
            rc = pack();
            if (rc) return rc;
        }
        if (any.on) {  // the record and the trace start again: the first record is the start state
            HIP_TRY(hipMemsetAsync(any.st.p, 0, sizeof(AnyState), stream));
            rc = launch_track(0);
            if (rc) return rc;
        }
        rc = quiet_restart();
        if (rc) return rc;
        return sync();
    }

    // Capture `chunk` (even) cycles into a hipGraph: launch-bound loops replay it.
    // The cycles a captured chunk holds while tracking: the configured chunk rounded to a multiple of `every` (and of 2,
    // the parity), 0 where no graph is built (graph_chunk 0, or evaluations more than 256 cycles apart: eager).
    // The same while watching for quiescence: a multiple of its `every` too, so that the checks sit at fixed places.
    int tracked_chunk() const {
        int chunk = params.graph_chunk < 0 ? 32 : params.graph_chunk;
        if (chunk < 2) return 0;
        chunk &= ~1;
        auto lcm = [](int64_t a, int64_t b) {
            int64_t x = a, y = b;
            while (y) { const int64_t r = x % y; x = y; y = r; }
            return a / x * b;
        };
        int64_t unit = 2;
        if (any.on) unit = lcm(unit, any.every);
        if (unit <= 256 && quiet.on) unit = lcm(unit, quiet.every);
        if (unit > 256) return 0;
        return (int)(std::max<int64_t>(1, chunk / unit) * unit);
    }
    // is a graph worth capturing for n cycles?  Twice the chunk, as ever; while tracking or watching, twice the REAL chunk
    bool worth_graph(int n) const {
        if (any.on || quiet.on) return tracked_chunk() >= 2 && n >= 2 * tracked_chunk();
        return n >= 2 * std::max(2, params.graph_chunk < 0 ? 32 : params.graph_chunk);
    }
    // `at`: the engine's cycle count where the capture starts.  While tracking, the captured chunk is a multiple of
    // `every` and holds the tracking launches at the positions that follow from `at` (any.graph_phase): a replay is
    // only started at a cycle count with the same remainder (run_async aligns, as it does for the parity).  The checks
    // of mxs_watch_quiescence likewise (quiet.graph_phase).
    void try_build_graph(int64_t at) {
        graph_tried = true;
        int chunk = params.graph_chunk;
        if (chunk < 0) chunk = 32;
        if (chunk < 2) return;
        chunk &= ~1;
        if (any.on || quiet.on) chunk = tracked_chunk();
        if (chunk < 2) return;
        if (cur != 0) return;  // captured with parity 0; run() aligns first
        hipGraph_t graph = nullptr;
        if (hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
            (void)hipGetLastError();
            return;
        }
        int from = 0;
        bool ok = true;
        capturing = true;  // (one stream inside a capture)
        for (int i = 0; i < chunk && ok; ++i) {
            ok = launch_cycle(from, false) == MXS_OK;
            from ^= 1;
            if (ok) ok = after_cycle(at + i + 1, from) == MXS_OK;
        }
        capturing = false;
        if (hipStreamEndCapture(stream, &graph) != hipSuccess || !ok || !graph) {
            (void)hipGetLastError();
            if (graph) (void)hipGraphDestroy(graph);
            return;
        }
        if (hipGraphInstantiate(&graph_exec, graph, nullptr, nullptr, 0) != hipSuccess) {
            (void)hipGetLastError();
            graph_exec = nullptr;
        } else {
            graph_cycles = chunk;
            if (any.on) any.graph_phase = (int)(at % any.every);
            if (quiet.on) quiet.graph_phase = (int)(at % quiet.every);
        }
        (void)hipGraphDestroy(graph);
    }

    int run_async(int n) override {
        if (n < 0) return fail(MXS_E_INVALID, "n_cycles must be >= 0");
        HIP_TRY(hipSetDevice(device));
        if (halo_ready)
            return fail(MXS_E_STATE, "a sharded engine must be stepped with mxs_step_compute/pack/unpack");
        int left = n;
        if (any.on || quiet.on) return run_tracked(n);
        if (left > 0 && cur != 0) {  // align to the parity the graph was captured with
            int rc = launch_cycle(cur, false);
            if (rc) return rc;
            cur ^= 1;
            --left;
        }
        if (!graph_tried && left >= 2 * std::max(2, params.graph_chunk < 0 ? 32 : params.graph_chunk))
            try_build_graph(cycles + (n - left));
        while (graph_exec && left >= graph_cycles) {
            HIP_TRY(hipGraphLaunch(graph_exec, stream));
            left -= graph_cycles;
        }
        for (; left > 0; --left) {
            int rc = launch_cycle(cur, false);
            if (rc) return rc;
            cur ^= 1;
        }
        cycles += n;
        return MXS_OK;
    }

    // What is queued behind cycle c (its messages are in buffer `now`): the evaluation of mxs_track_best when
    // c % every == 0, the check of mxs_watch_quiescence when c % every is 0 or 1.
    int after_cycle(int64_t c, int now) {
        if (any.on && c % any.every == 0) {
            int rc = launch_track(-1);
            if (rc) return rc;
        }
        if (quiet.on && c % quiet.every <= 1) return launch_quiet(now);
        return MXS_OK;
    }

    // run_async while tracking or watching: the same cycles, an evaluation queued behind every cycle c with
    // c % every == 0 (a check behind every c with c % every <= 1).  A replay holds these at fixed places, so it starts only
    // where the parity AND the remainders of the cycle count are those of the capture; the cycles before that, and the
    // tail, are eager.
    int run_tracked(int n) {
        int left = n;
        int64_t c = cycles;
        auto eager = [&]() {
            int rc = launch_cycle(cur, false);
            if (rc) return rc;
            cur ^= 1;
            --left;
            ++c;
            return after_cycle(c, cur);
        };
        if (left > 0 && cur != 0) {
            int rc = eager();
            if (rc) return rc;
        }
        if (!graph_tried && worth_graph(left)) try_build_graph(c);
        auto aligned = [&]() {
            return cur == 0 && (!any.on || c % any.every == any.graph_phase) && (!quiet.on || c % quiet.every == quiet.graph_phase);
        };
        for (int64_t tries = graph_cycles; graph_exec && left >= graph_cycles && !aligned() && tries > 0; --tries) {
            int rc = eager();
            if (rc) return rc;
        }
        while (graph_exec && aligned() && left >= graph_cycles) {
            HIP_TRY(hipGraphLaunch(graph_exec, stream));
            left -= graph_cycles;
            c += graph_cycles;
        }
        while (left > 0) {
            int rc = eager();
            if (rc) return rc;
        }
        cycles = c;
        return MXS_OK;
    }

#ifdef MXS_WIDE_PROFILE
    void wide_profile_dump() {
        if (!wide_prof.p) return;
        const int ng = (int)L.wide_blocks.size();
        std::vector<int64_t> h(8 * (size_t)ng);
        (void)hipDeviceSynchronize();
        (void)hipMemcpy(h.data(), wide_prof.p, sizeof(int64_t) * h.size(), hipMemcpyDeviceToHost);
        double acc[8] = {0};
        for (int g = 0; g < ng; ++g) for (int k = 0; k < 8; ++k) acc[k] += (double)h[8 * g + k];
        const double nb = acc[7] > 0 ? acc[7] : 1;
        fprintf(stderr, "k_variable_wide phase clocks per block (s_memtime ticks; %d blocks timed): stage %.0f | chains+beliefs %.0f | "
                        "selection %.0f | messages %.0f | stores %.0f | loop end %.0f | whole %.0f\n",
                (int)acc[7], acc[0] / nb, acc[1] / nb, acc[2] / nb, acc[3] / nb, acc[4] / nb, acc[5] / nb, acc[6] / nb);
    }
#endif
    int sync() override {
        HIP_TRY(hipStreamSynchronize(stream));
        if (comm) HIP_TRY(hipStreamSynchronize(comm));
        if (fused || p2p) {  // did a cut factor block give up waiting for its halo?
            uint32_t h[1] = {0};
            HIP_TRY(hipMemcpyAsync(h, halo_flags.p + HALO_ERR_WORD, sizeof(h), hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            if (h[0] != 0)
                return fail(MXS_E_STATE, "sharded cycle: cut factors waited > 5 s for a halo exchange that "
                                         "never arrived (an exchange / mxs_step_unpack per mxs_step_compute?)");
        }
        return MXS_OK;
    }

    int run_timed(int n, float* ms) override {
        HIP_TRY(hipSetDevice(device));
        // build the graph outside the timed region
        if (!graph_tried && cur == 0 && worth_graph(n)) try_build_graph(cycles);
        HIP_TRY(hipEventRecord(ev0, stream));
        int rc = run_async(n);
        if (rc) return rc;
        HIP_TRY(hipEventRecord(ev1, stream));
        HIP_TRY(hipEventSynchronize(ev1));
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, ev0, ev1));
        if (ms) *ms = t;
        return MXS_OK;
    }

    // `reps` repetitions of n cycles enqueued BACK TO BACK -- one HIP event between two repetitions, ONE host wait at
    // the end -- and the device time of every repetition: what a benchmark needs to quote a median over a timed
    // region long enough for the clocks to settle when one repetition is a fraction of a millisecond.
    int run_reps(int n, int reps, float* ms) override {
        HIP_TRY(hipSetDevice(device));
        if (n < 1 || reps < 1 || reps > 100000) return fail(MXS_E_INVALID, "mxs_run_reps: n >= 1, 1 <= reps <= 100000");
        if (halo_ready || p2p) return fail(MXS_E_STATE, "mxs_run_reps: not on a sharded engine");
        if (!graph_tried && cur == 0 && worth_graph(n)) try_build_graph(cycles);
        std::vector<hipEvent_t> evs((size_t)reps + 1, nullptr);
        int rc = MXS_OK;
        hipError_t he = hipSuccess;
        for (hipEvent_t& e : evs)
            if (he == hipSuccess) he = hipEventCreate(&e);
        for (int r = 0; r < reps && he == hipSuccess && rc == MXS_OK; ++r) {
            if (r == 0) he = hipEventRecord(evs[0], stream);
            if (he == hipSuccess) rc = run_async(n);
            if (rc == MXS_OK && he == hipSuccess) he = hipEventRecord(evs[r + 1], stream);
        }
        if (he == hipSuccess && rc == MXS_OK) he = hipEventSynchronize(evs[reps]);
        for (int r = 0; r < reps && he == hipSuccess && rc == MXS_OK; ++r) {
            float t = 0.f;
            he = hipEventElapsedTime(&t, evs[r], evs[r + 1]);
            if (ms) ms[r] = t;
        }
        for (hipEvent_t e : evs)
            if (e) (void)hipEventDestroy(e);
        if (rc) return rc;
        HIP_TRY(he);
        return sync();
    }

    int get_assignment(int32_t* idx, double* bel) override {
        HIP_TRY(hipSetDevice(device));
        { int rc = sync(); if (rc) return rc; }
        const int nV = L.n_vars;
        std::vector<int32_t> hs(nV);
        std::vector<T> hb(nV);
        if (nV) {
            HIP_TRY(copy_sync(hs.data(), sel.p, sizeof(int32_t) * nV, hipMemcpyDeviceToHost, stream));
            HIP_TRY(copy_sync(hb.data(), belief.p, sizeof(T) * nV, hipMemcpyDeviceToHost, stream));
        }
        const double sign = L.is_max ? -1.0 : 1.0;
        for (int vi = 0; vi < nV; ++vi) {
            const int v = L.var_i2e[vi];
            if (idx) idx[v] = hs[vi];
            if (bel) bel[v] = sign * (double)hb[vi];
        }
        return MXS_OK;
    }

    int get_messages(double* v2f_out, double* f2v_out, uint8_t* cv, uint8_t* cf) override {
        HIP_TRY(hipSetDevice(device));
        { int rc = sync(); if (rc) return rc; }
        const int nE = L.n_edges;
        // (peer-store mode: the ghost records live behind the V2F buffer, offsets >= v2f_elems)
        std::vector<T> hv((size_t)(L.v2f_elems + (p2p ? ghost_len : 0))), hf((size_t)L.f2v_elems);
        std::vector<uint8_t> hcF(nE), hcV((size_t)L.n_cv);
        if (L.v2f_elems)
            HIP_TRY(copy_sync(hv.data(), v2f[cur].p, sizeof(T) * (size_t)L.v2f_elems, hipMemcpyDeviceToHost, stream));
        if (p2p && ghost_len)
            HIP_TRY(copy_sync(hv.data() + L.v2f_elems, ghost3.p + (int64_t)(gen % 3) * ghost_len,
                              sizeof(T) * (size_t)ghost_len, hipMemcpyDeviceToHost, stream));
        if (L.f2v_elems)
            HIP_TRY(copy_sync(hf.data(), f2v[cur].p, sizeof(T) * hf.size(), hipMemcpyDeviceToHost, stream));
        if (nE) {
            HIP_TRY(copy_sync(hcF.data(), cF.p, nE, hipMemcpyDeviceToHost, stream));
            HIP_TRY(copy_sync(hcV.data(), cV.p, (size_t)L.n_cv, hipMemcpyDeviceToHost, stream));
        }
        // caller's message offsets: prefix of the edge domain sizes in caller order
        std::vector<int64_t> ext_off(nE + 1, 0);
        for (int e = 0; e < nE; ++e) ext_off[e + 1] = ext_off[e] + L.edge_dom[L.edge_e2i[e]];
        const double sign = L.is_max ? -1.0 : 1.0;
        for (int ei = 0; ei < nE; ++ei) {
            const int e = L.edge_i2e[ei];
            const int D = L.edge_dom[ei];
            for (int d = 0; d < D; ++d) {
                if (v2f_out) v2f_out[ext_off[e] + d] = sign * (double)hv[L.v2f_off[ei] + d];
                if (f2v_out) f2v_out[ext_off[e] + d] = sign * (double)hf[L.f2v_off[ei] + d];
            }
            if (cf) cf[e] = L.edge_fcim[ei] ? (uint8_t)(int)hf[L.f2v_off[ei] + D] : hcF[ei];
        }
        if (cv)
            for (int k = 0; k < nE; ++k) {
                const int ei = L.vslot_edge[k];
                cv[L.edge_i2e[ei]] = L.edge_vcim[ei] ? (uint8_t)(int)hv[L.v2f_off[ei] + L.edge_dom[ei]]
                                                     : hcV[L.vslot_cv[k]];
            }
        return MXS_OK;
    }

    // mxs_set_state: the caller's arrays (layouts of get_messages / get_assignment) -> device
    // records of the CURRENT buffers.  Read-modify-write of whole buffers: padding, null blocks
    // and whatever the caller leaves out stay as they are.
    int set_state(const double* v2f_in, const double* f2v_in, const uint8_t* cv, const uint8_t* cf,
                  const int32_t* idx, const double* bel, int64_t cyc) override {
        HIP_TRY(hipSetDevice(device));
        { int rc = sync(); if (rc) return rc; }
        if (halo_ready || p2p) return fail(MXS_E_STATE, "mxs_set_state on a shard with an exchange set up");
        if (cyc < 0) return fail(MXS_E_INVALID, "negative cycle count");
        const int nE = L.n_edges, nV = L.n_vars;
        std::vector<T> hv((size_t)L.v2f_elems), hf((size_t)L.f2v_elems);
        std::vector<uint8_t> hcF(nE), hcV((size_t)L.n_cv);
        if (L.v2f_elems) HIP_TRY(copy_sync(hv.data(), v2f[cur].p, sizeof(T) * hv.size(), hipMemcpyDeviceToHost, stream));
        if (L.f2v_elems) HIP_TRY(copy_sync(hf.data(), f2v[cur].p, sizeof(T) * hf.size(), hipMemcpyDeviceToHost, stream));
        if (nE) {
            HIP_TRY(copy_sync(hcF.data(), cF.p, nE, hipMemcpyDeviceToHost, stream));
            HIP_TRY(copy_sync(hcV.data(), cV.p, (size_t)L.n_cv, hipMemcpyDeviceToHost, stream));
        }
        std::vector<int64_t> ext_off(nE + 1, 0);
        for (int e = 0; e < nE; ++e) ext_off[e + 1] = ext_off[e] + L.edge_dom[L.edge_e2i[e]];
        const double sign = L.is_max ? -1.0 : 1.0;
        for (int ei = 0; ei < nE; ++ei) {
            const int e = L.edge_i2e[ei];
            const int D = L.edge_dom[ei];
            for (int d = 0; d < D; ++d) {
                if (v2f_in) hv[L.v2f_off[ei] + d] = (T)(sign * v2f_in[ext_off[e] + d]);
                if (f2v_in) hf[L.f2v_off[ei] + d] = (T)(sign * f2v_in[ext_off[e] + d]);
            }
            if (cf) {
                if (cf[e] > SAME_COUNT) return fail(MXS_E_INVALID, "send counter above SAME_COUNT");
                if (L.edge_fcim[ei]) hf[L.f2v_off[ei] + D] = (T)(int)cf[e];
                else hcF[ei] = cf[e];
            }
        }
        if (cv)
            for (int k = 0; k < nE; ++k) {
                const int ei = L.vslot_edge[k];
                const uint8_t c = cv[L.edge_i2e[ei]];
                if (c > SAME_COUNT) return fail(MXS_E_INVALID, "send counter above SAME_COUNT");
                if (L.edge_vcim[ei]) hv[L.v2f_off[ei] + L.edge_dom[ei]] = (T)(int)c;
                else hcV[L.vslot_cv[k]] = c;
            }
        if (L.v2f_elems) HIP_TRY(copy_sync(v2f[cur].p, hv.data(), sizeof(T) * hv.size(), hipMemcpyHostToDevice, stream));
        if (L.f2v_elems) HIP_TRY(copy_sync(f2v[cur].p, hf.data(), sizeof(T) * hf.size(), hipMemcpyHostToDevice, stream));
        if (nE) {
            HIP_TRY(copy_sync(cF.p, hcF.data(), nE, hipMemcpyHostToDevice, stream));
            HIP_TRY(copy_sync(cV.p, hcV.data(), (size_t)L.n_cv, hipMemcpyHostToDevice, stream));
        }
        if ((idx || bel) && nV) {
            std::vector<int32_t> hs(nV);
            std::vector<T> hb(nV);
            HIP_TRY(copy_sync(hs.data(), sel.p, sizeof(int32_t) * nV, hipMemcpyDeviceToHost, stream));
            HIP_TRY(copy_sync(hb.data(), belief.p, sizeof(T) * nV, hipMemcpyDeviceToHost, stream));
            for (int vi = 0; vi < nV; ++vi) {
                const int v = L.var_i2e[vi];
                if (idx) {
                    if (idx[v] < 0 || idx[v] >= L.vdom[vi]) return fail(MXS_E_INVALID, "selection index out of the domain");
                    hs[vi] = idx[v];
                }
                if (bel) hb[vi] = (T)(sign * bel[v]);
            }
            HIP_TRY(copy_sync(sel.p, hs.data(), sizeof(int32_t) * nV, hipMemcpyHostToDevice, stream));
            HIP_TRY(copy_sync(belief.p, hb.data(), sizeof(T) * nV, hipMemcpyHostToDevice, stream));
        }
        cycles = cyc;
        return MXS_OK;
    }

    // the one k_eval launch of mxs_eval_cost and of a tracked evaluation: the same arguments, the same grid
    EvalArgs eval_args(const int32_t* didx, double infinity) const {
        EvalArgs a{};
        a.frowptr = frowptr.p;
        a.edge_var_int = edge_var_int.p;
        a.edge_dom = edge_dom.p;
        a.tab_off = eval_tab_off.p;
        a.tables = eval_tables.p;
        a.vdom = vdom.p;
        a.vcost_off = vcost_off.p;
        a.var_cost = eval_var_cost.p;
        a.owned = owned.p;
        a.fowned = fowned.p;
        a.idx = didx;
        a.part_cost = part_cost.p;
        a.part_viol = part_viol.p;
        a.n_factors = L.n_factors;
        a.n_vars = L.n_vars;
        a.infinity = infinity;
        return a;
    }
    int eval_blocks() const {
        const int total = L.n_factors + L.n_vars;
        return std::max(1, std::min(EVAL_BLOCKS, (total + BLOCK - 1) / BLOCK));
    }

    // ---- best state and cost trace (include/maxsum_gpu_anytime.h, anytime.h) ----------------------------------
    // One evaluation of `sel`, queued on the compute stream with no read-back: k_eval, k_any_final, k_any_copy.
    // Behind launch_cycle it comes after the join of the wide-variable side stream (k_variable_wide writes `sel`
    // too) and before the next cycle's sweep; inside a capture it is three more nodes of the one captured stream.
    // first_cycle >= 0: a first record at that cycle (never captured: the argument is the host's cycle count);
    // < 0: the periodic evaluation, whose cycle number the device keeps (AnyState::next_cycle) because a
    // captured graph freezes kernel arguments.
    int launch_track(long long first_cycle) {
        const int nb = eval_blocks(), nV = L.n_vars;
        hipLaunchKernelGGL(k_eval, dim3(nb), dim3(BLOCK), 0, stream, eval_args(sel.p, any.infinity));
        AnyTrace tr{any.tr_cycle.p, any.tr_cost.p, any.tr_viol.p, (int32_t)any.tr_cycle.n};
        hipLaunchKernelGGL(k_any_final, dim3(1), dim3(ANY_TPB), 0, stream, nb, L.is_max ? 1 : 0, (const double*)part_cost.p,
                           (const unsigned long long*)part_viol.p, first_cycle, any.every, any.st.p, tr);
        hipLaunchKernelGGL(k_any_copy, dim3((unsigned)std::max(1, (nV + ANY_TPB - 1) / ANY_TPB)), dim3(ANY_TPB), 0, stream, nV,
                           (const int32_t*)sel.p, any.snap.p, any.st.p);
        HIP_TRY(hipGetLastError());
        return MXS_OK;
    }
    void drop_graph() {  // the captured cycle loop has (or lacks) the tracking launches of the old setting
        if (graph_exec) {
            (void)hipGraphExecDestroy(graph_exec);
            graph_exec = nullptr;
        }
        graph_tried = false;
    }
    bool tracking() const override { return any.on; }
    int track_best(int32_t every, double infinity, int32_t trace_cap) override {
        HIP_TRY(hipSetDevice(device));
        if (every < 0 || trace_cap < 0) return fail(MXS_E_INVALID, "mxs_track_best: every >= 0 and trace_capacity >= 0");
        if (halo_ready || nccl_comm || p2p)
            return fail(MXS_E_STATE, "mxs_track_best: not on a sharded engine (a shard's cost is partial)");
        { int rc = sync(); if (rc) return rc; }
        auto release = [](auto& b) {
            if (b.p) (void)hipFree(b.p);
            b.p = nullptr;
            b.n = 0;
        };
        if (every == 0) {
            if (any.on) drop_graph();
            any.on = false;
            any.every = 0;
            release(any.st), release(any.snap), release(any.tr_cycle), release(any.tr_viol), release(any.tr_cost);
            return MXS_OK;
        }
        {   // all the new buffers first: a call that fails leaves the old setting as it was
            Anytime fresh;
            HIP_TRY(fresh.st.alloc(1));
            HIP_TRY(fresh.snap.alloc((size_t)L.n_vars));
            HIP_TRY(fresh.tr_cycle.alloc((size_t)trace_cap));
            HIP_TRY(fresh.tr_viol.alloc((size_t)trace_cap));
            HIP_TRY(fresh.tr_cost.alloc((size_t)trace_cap));
            auto swap = [](auto& a, auto& b) { std::swap(a.p, b.p); std::swap(a.n, b.n); };
            swap(any.st, fresh.st), swap(any.snap, fresh.snap), swap(any.tr_cycle, fresh.tr_cycle);
            swap(any.tr_viol, fresh.tr_viol), swap(any.tr_cost, fresh.tr_cost);
        }
        any.on = true;
        any.every = every;
        any.infinity = infinity;
        drop_graph();
        HIP_TRY(hipMemsetAsync(any.st.p, 0, sizeof(AnyState), stream));
        return launch_track(cycles);
    }
    int track_restart() override { return any.on ? launch_track(cycles) : MXS_OK; }
    int get_best(int64_t* cycle, double* cost, int64_t* viol, int32_t* idx) override {
        HIP_TRY(hipSetDevice(device));
        if (!any.on) return fail(MXS_E_STATE, "mxs_get_best needs mxs_track_best (every > 0) first");
        { int rc = sync(); if (rc) return rc; }
        AnyState h{};
        HIP_TRY(copy_sync(&h, any.st.p, sizeof(h), hipMemcpyDeviceToHost, stream));
        if (cycle) *cycle = h.best_cycle;
        if (cost) *cost = h.best_cost;
        if (viol) *viol = h.best_viol;
        if (idx && L.n_vars) {
            std::vector<int32_t> hs((size_t)L.n_vars);
            HIP_TRY(copy_sync(hs.data(), any.snap.p, sizeof(int32_t) * hs.size(), hipMemcpyDeviceToHost, stream));
            for (int vi = 0; vi < L.n_vars; ++vi) idx[L.var_i2e[vi]] = hs[vi];
        }
        return MXS_OK;
    }
    int get_cost_trace(int64_t* cycle, double* cost, int64_t* viol, int32_t cap, int32_t* n, int64_t* evals) override {
        HIP_TRY(hipSetDevice(device));
        if (!any.on) return fail(MXS_E_STATE, "mxs_get_cost_trace needs mxs_track_best (every > 0) first");
        if (cap < 0 || (cap > 0 && (!cycle || !cost || !viol))) return fail(MXS_E_INVALID, "mxs_get_cost_trace: bad capacity or null arrays");
        { int rc = sync(); if (rc) return rc; }
        AnyState h{};
        HIP_TRY(copy_sync(&h, any.st.p, sizeof(h), hipMemcpyDeviceToHost, stream));
        const size_t k = (size_t)std::min<long long>(h.evals, std::min<long long>((long long)any.tr_cycle.n, cap));
        static_assert(sizeof(long long) == sizeof(int64_t), "the trace is copied out as it is stored");
        HIP_TRY(copy_sync(cycle, any.tr_cycle.p, sizeof(int64_t) * k, hipMemcpyDeviceToHost, stream));
        HIP_TRY(copy_sync(cost, any.tr_cost.p, sizeof(double) * k, hipMemcpyDeviceToHost, stream));
        HIP_TRY(copy_sync(viol, any.tr_viol.p, sizeof(int64_t) * k, hipMemcpyDeviceToHost, stream));
        if (n) *n = (int32_t)k;
        if (evals) *evals = h.evals;
        return MXS_OK;
    }

    // ---- quiescence (include/maxsum_gpu_quiescence.h, quiescence.h) ------------------------------------------
    // Where the 2*E send counters live (the places get_messages reads them from), listed once: tiles of whole 16-byte
    // quads of cF / cV in which every byte is an edge's counter, a gather list for the other bytes and for the
    // counters kept behind a message record.  cV slots that belong to no edge, and the cF bytes of edges whose counter
    // rides in the message, are in neither.
    int build_quiet_lists(Quiet& q) {
        const int nE = L.n_edges;
        if (L.n_cv >= (int64_t)QUIET_IN_CV || L.f2v_elems > INT32_MAX || L.v2f_elems > INT32_MAX)
            return fail(MXS_E_INVALID, "mxs_watch_quiescence: the counter arrays are beyond 2^31 entries");
        std::vector<uint8_t> useF((size_t)nE, 0), useV((size_t)L.n_cv, 0);
        std::vector<uint32_t> in_f2v, in_v2f;
        for (int ei = 0; ei < nE; ++ei) {
            if (L.edge_fcim[ei]) in_f2v.push_back((uint32_t)(L.f2v_off[ei] + L.edge_dom[ei]));
            else useF[ei] = 1;
        }
        for (int k = 0; k < nE; ++k) {
            const int ei = L.vslot_edge[k];
            if (L.edge_vcim[ei]) in_v2f.push_back((uint32_t)(L.v2f_off[ei] + L.edge_dom[ei]));
            else useV[(size_t)L.vslot_cv[k]] = 1;
        }
        std::vector<QuietTile> tiles;
        std::vector<uint32_t> gather;
        auto scan = [&](const std::vector<uint8_t>& use, uint32_t flag) {
            const size_t n = use.size(), nq = n / 16;
            auto whole = [&](size_t quad) {
                for (size_t b = 0; b < 16; ++b)
                    if (!use[quad * 16 + b]) return false;
                return true;
            };
            size_t quad = 0;
            while (quad < nq) {
                if (!whole(quad)) {
                    for (size_t b = 0; b < 16; ++b)
                        if (use[quad * 16 + b]) gather.push_back((uint32_t)(quad * 16 + b) | flag);
                    ++quad;
                    continue;
                }
                size_t len = 1;
                while (len < 64 && quad + len < nq && whole(quad + len)) ++len;
                tiles.push_back(QuietTile{(uint32_t)quad, (uint32_t)len | flag});
                quad += len;
            }
            for (size_t b = nq * 16; b < n; ++b)
                if (use[b]) gather.push_back((uint32_t)b | flag);
        };
        scan(useF, 0u);
        scan(useV, QUIET_IN_CV);
        q.lists.n_tiles = (int32_t)tiles.size();
        q.lists.n_bytes = (int32_t)gather.size();
        q.lists.n_f2v = (int32_t)in_f2v.size();
        q.lists.n_v2f = (int32_t)in_v2f.size();
        gather.insert(gather.end(), in_f2v.begin(), in_f2v.end());
        gather.insert(gather.end(), in_v2f.begin(), in_v2f.end());
        const int64_t threads = std::max<int64_t>((int64_t)tiles.size() * 64, (int64_t)gather.size());
        q.blocks = (int)std::max<int64_t>(1, std::min<int64_t>(QUIET_MAX_PARTS, (threads + QUIET_TPB - 1) / QUIET_TPB));
        // the most one lane can count: 16 per tile of its wave, 1 per gather entry of its own
        const int64_t waves = (int64_t)q.blocks * (QUIET_TPB / 64), grid = (int64_t)q.blocks * QUIET_TPB;
        const int64_t most = 16 * (((int64_t)tiles.size() + waves - 1) / waves) + ((int64_t)gather.size() + grid - 1) / grid;
        q.lists.bits = 0;
        while (q.lists.bits < 32 && (most >> q.lists.bits) != 0) ++q.lists.bits;
        HIP_TRY(q.tiles.upload(tiles, stream));
        HIP_TRY(q.gather.upload(gather, stream));
        HIP_TRY(q.part.alloc((size_t)QUIET_MAX_PARTS));
        HIP_TRY(q.st.alloc(1));
        q.lists.tiles = q.tiles.p;
        q.lists.gather = q.gather.p;
        return MXS_OK;
    }
    // One check, queued on the compute stream with no read-back: k_quiet_count, k_quiet_final.  `now`: the buffers that
    // hold the messages of the cycle just queued (a fixed place of a captured chunk has a fixed parity).  Behind
    // launch_cycle it comes after the join of the wide-variable side stream and before the next cycle's sweep.
    int launch_quiet(int now) {
        hipLaunchKernelGGL(k_quiet_count<T>, dim3((unsigned)quiet.blocks), dim3(QUIET_TPB), 0, stream, quiet.lists,
                           (const uint8_t*)cF.p, (const uint8_t*)cV.p, (const T*)f2v[now].p, (const T*)v2f[now].p, quiet.part.p);
        hipLaunchKernelGGL(k_quiet_final, dim3(1), dim3(QUIET_TPB), 0, stream, quiet.blocks, (const uint32_t*)quiet.part.p,
                           quiet.every, quiet.st.p);
        HIP_TRY(hipGetLastError());
        return MXS_OK;
    }
    bool watching() const override { return quiet.on; }
    int quiet_restart() override {
        if (!quiet.on) return MXS_OK;
        hipLaunchKernelGGL(k_quiet_restart, dim3(1), dim3(1), 0, stream, quiet.st.p, (long long)cycles, quiet.every, 0);
        HIP_TRY(hipGetLastError());
        return MXS_OK;
    }
    int watch_quiescence(int32_t every) override {
        HIP_TRY(hipSetDevice(device));
        if (every < 0) return fail(MXS_E_INVALID, "mxs_watch_quiescence: every >= 0");
        if (halo_ready || nccl_comm || p2p)
            return fail(MXS_E_STATE, "mxs_watch_quiescence: not on a sharded engine (a shard sees its own edges only)");
        { int rc = sync(); if (rc) return rc; }
        auto swap = [](auto& a, auto& b) { std::swap(a.p, b.p); std::swap(a.n, b.n); };
        Quiet fresh;  // every == 0: the old buffers go with it
        if (every > 0) {  // all the new buffers first: a call that fails leaves the old setting as it was
            int rc = build_quiet_lists(fresh);
            if (rc) return rc;
        }
        if (quiet.on || every > 0) drop_graph();
        swap(quiet.st, fresh.st), swap(quiet.tiles, fresh.tiles), swap(quiet.gather, fresh.gather), swap(quiet.part, fresh.part);
        quiet.lists = fresh.lists;
        quiet.blocks = fresh.blocks;
        quiet.on = every > 0;
        quiet.every = every;
        if (!quiet.on) return MXS_OK;
        hipLaunchKernelGGL(k_quiet_restart, dim3(1), dim3(1), 0, stream, quiet.st.p, (long long)cycles, quiet.every, 1);
        HIP_TRY(hipGetLastError());
        return MXS_OK;
    }
    int quiet_read(QuietState* h) {
        { int rc = sync(); if (rc) return rc; }
        HIP_TRY(copy_sync(h, quiet.st.p, sizeof(*h), hipMemcpyDeviceToHost, stream));
        return MXS_OK;
    }
    int quiescence(int32_t* quiescent, int64_t* cycle, int64_t* checks, int64_t* active, int64_t* last_check) override {
        HIP_TRY(hipSetDevice(device));
        if (!quiet.on) return fail(MXS_E_STATE, "mxs_quiescence needs mxs_watch_quiescence (every > 0) first");
        QuietState h{};
        { int rc = quiet_read(&h); if (rc) return rc; }
        if (quiescent) *quiescent = h.quiescent_at >= 0 ? 1 : 0;
        if (cycle) *cycle = h.quiescent_at;
        if (checks) *checks = h.checks;
        if (active) *active = h.active;
        if (last_check) *last_check = h.last_check;
        return MXS_OK;
    }
    int run_until_quiescent(int32_t max_cycles, int32_t poll, int32_t* quiescent, int64_t* cycle, int64_t* ran) override {
        HIP_TRY(hipSetDevice(device));
        if (!quiet.on) return fail(MXS_E_STATE, "mxs_run_until_quiescent needs mxs_watch_quiescence (every > 0) first");
        if (max_cycles < 0) return fail(MXS_E_INVALID, "mxs_run_until_quiescent: max_cycles >= 0");
        if (poll <= 0) poll = std::max(64, 2 * tracked_chunk());
        QuietState h{};
        { int rc = quiet_read(&h); if (rc) return rc; }
        int64_t done = 0;
        while (h.quiescent_at < 0 && done < max_cycles) {
            const int span = (int)std::min<int64_t>(poll, max_cycles - done);
            int rc = run_async(span);
            if (rc) return rc;
            done += span;
            rc = quiet_read(&h);
            if (rc) return rc;
        }
        if (quiescent) *quiescent = h.quiescent_at >= 0 ? 1 : 0;
        if (cycle) *cycle = h.quiescent_at;
        if (ran) *ran = done;
        return MXS_OK;
    }

    int eval_cost(const int32_t* idx, double infinity, double* cost, int64_t* viol) override {
        HIP_TRY(hipSetDevice(device));
        { int rc = sync(); if (rc) return rc; }
        const int nV = L.n_vars;
        const int32_t* didx = sel.p;
        if (idx) {
            std::vector<int32_t> h(nV);
            for (int vi = 0; vi < nV; ++vi) {
                const int32_t x = idx[L.var_i2e[vi]];
                if (x < 0 || x >= L.vdom[vi]) return fail(MXS_E_INVALID, "assignment index out of the domain");
                h[vi] = x;
            }
            HIP_TRY(copy_sync(eval_idx.p, h.data(), sizeof(int32_t) * nV, hipMemcpyHostToDevice, stream));
            didx = eval_idx.p;
        }
        const EvalArgs a = eval_args(didx, infinity);
        const int nb = eval_blocks();
        hipLaunchKernelGGL(k_eval, dim3(nb), dim3(BLOCK), 0, stream, a);
        HIP_TRY(hipGetLastError());
        std::vector<double> pc(nb);
        std::vector<unsigned long long> pv(nb);
        HIP_TRY(hipStreamSynchronize(stream));
        HIP_TRY(copy_sync(pc.data(), part_cost.p, sizeof(double) * nb, hipMemcpyDeviceToHost, stream));
        HIP_TRY(copy_sync(pv.data(), part_viol.p, sizeof(unsigned long long) * nb, hipMemcpyDeviceToHost, stream));
        double c = 0;
        int64_t v = 0;
        for (int i = 0; i < nb; ++i) {
            c += pc[i];
            v += (int64_t)pv[i];
        }
        if (cost) *cost = c;
        if (viol) *viol = v;
        return MXS_OK;
    }

    // Profiling: run ONE more cycle with per-block timestamps (wall_clock64 ticks,
    // 100 MHz) and return {start, end, class kind} per block of the sweep launch.
    int debug_timeline(int64_t* out, int32_t cap, int32_t* n_blocks) override {
        HIP_TRY(hipSetDevice(device));
        if (halo_ready) return fail(MXS_E_STATE, "mxs_debug_timeline: not on a sharded engine");
        if (any.on) return fail(MXS_E_STATE, "mxs_debug_timeline: not while mxs_track_best is on (its cycle would go unrecorded)");
        if (quiet.on) return fail(MXS_E_STATE, "mxs_debug_timeline: not while mxs_watch_quiescence is on (its cycle would go unchecked)");
        const int nb = L.n_blocks_sweep;
        if (n_blocks) *n_blocks = nb;
        if (!out) return MXS_OK;
        if (cap < nb) return fail(MXS_E_INVALID, "timeline buffer too small");
        if (timeline.n < (size_t)3 * nb) {
            if (timeline.p) (void)hipFree(timeline.p);
            timeline.p = nullptr;
            HIP_TRY(timeline.alloc((size_t)3 * nb));
        }
        timeline_on = true;
        int rc = launch_cycle(cur, false);
        timeline_on = false;
        if (rc) return rc;
        cur ^= 1;
        cycles += 1;
        HIP_TRY(hipStreamSynchronize(stream));
        HIP_TRY(copy_sync(out, timeline.p, sizeof(int64_t) * 3 * nb, hipMemcpyDeviceToHost, stream));
        return MXS_OK;
    }

    // change_factor_function (pydcop/algorithms/maxsum_dynamic.py:80-104): a factor gets a
    // new cost table of the same shape; messages, counters and selections carry on.
    int update_table(int32_t factor, const double* table, int64_t n) override {
        HIP_TRY(hipSetDevice(device));
        if (factor < 0 || factor >= L.n_factors) return fail(MXS_E_INVALID, "factor out of range");
        const int fi = L.factor_e2i[factor];
        const int64_t want = L.eval_tab_off[fi + 1] - L.eval_tab_off[fi];
        if (!table || n != want) return fail(MXS_E_INVALID, "the new table must have the shape of the old one");
        { int rc = sync(); if (rc) return rc; }
        const double sign = L.is_max ? -1.0 : 1.0;
        std::vector<T> h((size_t)n);
        for (int64_t k = 0; k < n; ++k) h[k] = (T)(sign * table[k]);
        DevBuf<T> staging;
        HIP_TRY(staging.upload(h, stream));
        hipLaunchKernelGGL((k_table_update<T>), dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, stream,
                           tables.p, L.f_tab_base[fi], (int64_t)L.f_tab_stride[fi], (const T*)staging.p, n);
        HIP_TRY(hipGetLastError());
        HIP_TRY(copy_sync(eval_tables.p + L.eval_tab_off[fi], table, sizeof(double) * (size_t)n,
                          hipMemcpyHostToDevice, stream));  // also waits for the kernel above
        const NaryLaunch* grp = L.f_class[fi] < 0 && L.f_ndesc[fi] >= 0 ? launch_of(fi) : nullptr;
        if (grp && is_bin2(grp->box) && L.f_tab_type[fi] == TAB_FULL) {
            // a lane-grid factor reads its image at every width (bin_box.h): re-encode it in the arithmetic type
            int rc = write_bin2_image(fi, *grp, table, n);
            if (rc) return rc;
        } else if (L.f_tab_type[fi] != TAB_FULL) {  // the factor's table is read from a narrow image
            const int t = L.f_tab_type[fi];
            const int fit = narrowest_tab_type(table, n, (int)sizeof(T));
            if (fit >= t) {  // (TAB_I8 > TAB_I16 > TAB_F32: at least as narrow as the stored type)
                const int cls = L.f_class[fi];
                std::vector<uint8_t> rec;
                if (cls >= 0) {  // register class: one record of back-to-back entries
                    rec.assign((size_t)L.classes[cls].ctab_rec, 0);
                    encode_tab_record(table, (int)n, t, rec.data());
                } else {  // workgroup-per-factor: the lane-packed / box image (layout.h, nary_place_pos)
                    const NaryDesc& d = L.ndesc[L.f_ndesc[fi]];
                    const NaryPlace pl = nary_place(*launch_of(fi), d, (int)sizeof(T));
                    rec.assign((size_t)nary_place_bytes(pl, d.dom[0]), 0);
                    for (int64_t k = 0; k < n; ++k) encode_tab_record(table + k, 1, t, rec.data() + nary_place_pos(pl, k));
                }
                HIP_TRY(copy_sync(ctables.p + L.f_ctab_off[fi], rec.data(), rec.size(), hipMemcpyHostToDevice, stream));
            } else {
                int rc = widen_factor(fi, table);
                if (rc) return rc;
            }
        }
        return MXS_OK;
    }

    // The image of lane-grid factor fi (bin_box.h), in the storage type of its launch group `nl`, from the n
    // un-negated values `table` -- at the image's current place.
    int write_bin2_image(int fi, const NaryLaunch& nl, const double* table, int64_t n) {
        const NaryDesc& d = L.ndesc[L.f_ndesc[fi]];
        const NaryPlace pl = nary_place(nl, d, (int)sizeof(T));
        std::vector<uint8_t> rec((size_t)nary_place_bytes(pl, d.dom[0]), 0);
        for (int64_t k = 0; k < n; ++k) encode_tab_entry(table[k], nl.tab_type, (int)sizeof(T), rec.data() + nary_place_pos(pl, k));
        HIP_TRY(copy_sync(ctables.p + L.f_ctab_off[fi], rec.data(), rec.size(), hipMemcpyHostToDevice, stream));
        return MXS_OK;
    }

    // A lane-grid factor leaves its narrow image: a full-width image of its own is appended to the compact-table
    // buffer (the buffer grows: a rare event, the run is stopped anyway) and filled from `values` (un-negated; NULL:
    // the factor's current table, read back from the device).  -> its byte offset in `at`.
    int append_bin2_full_image(int fi, const NaryLaunch& nl, const double* values, int64_t* at) {
        const NaryDesc& d = L.ndesc[L.f_ndesc[fi]];
        NaryLaunch full = nl;
        full.tab_type = TAB_FULL;
        const NaryPlace pl = nary_place(full, d, (int)sizeof(T));
        const int64_t n = L.eval_tab_off[fi + 1] - L.eval_tab_off[fi];
        std::vector<double> cur;
        if (!values) {
            cur.resize((size_t)n);
            HIP_TRY(copy_sync(cur.data(), eval_tables.p + L.eval_tab_off[fi], sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, stream));
            values = cur.data();
        }
        // (ctables.n = the buffer's CAPACITY from here on, ctables_used what holds images: the buffer grows geometrically, so a
        // stream of widened factors copies O(total) bytes, not O(total) per update -- ADVICE r5.  The narrow image the factor leaves
        // stays behind as dead space, and the host copy L.ctables is NOT kept current: the device buffer is authoritative after init.)
        if (ctables_used == 0) ctables_used = ctables.n;
        const size_t old_bytes = ctables_used, off = (old_bytes + 15) / 16 * 16, bytes = (size_t)nary_place_bytes(pl, d.dom[0]);
        std::vector<uint8_t> rec(bytes, 0);
        for (int64_t k = 0; k < n; ++k) encode_tab_entry(values[k], TAB_FULL, (int)sizeof(T), rec.data() + nary_place_pos(pl, k));
        if (off + bytes > ctables.n) {
            DevBuf<uint8_t> grown;
            HIP_TRY(grown.alloc(std::max(off + bytes, 2 * ctables.n + ((size_t)1 << 20))));
            if (old_bytes) HIP_TRY(copy_sync(grown.p, ctables.p, old_bytes, hipMemcpyDeviceToDevice, stream));
            std::swap(ctables.p, grown.p);
            std::swap(ctables.n, grown.n);
        }
        HIP_TRY(copy_sync(ctables.p + off, rec.data(), bytes, hipMemcpyHostToDevice, stream));
        ctables_used = off + bytes;
        *at = (int64_t)off;
        return MXS_OK;
    }

    // ---- external (read-only) variables: parent relations sliced on the device -------------
    struct ParentTab {
        DevBuf<double> buf;
        std::vector<int32_t> dims;
        std::vector<uint8_t> ext;
    };
    std::map<int, std::unique_ptr<ParentTab>> parents;  // by internal factor id

    int set_parent(int32_t factor, const double* parent, int32_t nd, const int32_t* dims, const uint8_t* ext) override {
        HIP_TRY(hipSetDevice(device));
        if (factor < 0 || factor >= L.n_factors) return fail(MXS_E_INVALID, "factor out of range");
        if (!parent || !dims || !ext || nd < 1 || nd > 32) return fail(MXS_E_INVALID, "bad parent relation");
        const int fi = L.factor_e2i[factor];
        const int e0 = L.frowptr[fi], ar = L.frowptr[fi + 1] - e0;
        int64_t total = 1;
        int w = 0;
        for (int i = 0; i < nd; ++i) {
            if (dims[i] < 1) return fail(MXS_E_INVALID, "bad parent dimension");
            total *= dims[i];
            if (total > ((int64_t)1 << 40)) return fail(MXS_E_INVALID, "parent relation too large");
            if (!ext[i]) {  // the writable dimensions, in order, are the factor's scope
                if (w >= ar || dims[i] != L.edge_dom[e0 + w])
                    return fail(MXS_E_INVALID, "the writable dimensions of the parent relation must be the factor's scope");
                ++w;
            }
        }
        if (w != ar) return fail(MXS_E_INVALID, "the writable dimensions of the parent relation must be the factor's scope");
        auto pt = std::make_unique<ParentTab>();
        pt->dims.assign(dims, dims + nd);
        pt->ext.assign(ext, ext + nd);
        std::vector<double> h(parent, parent + total);
        HIP_TRY(pt->buf.upload(h, stream));
        parents[fi] = std::move(pt);
        // every slice of this relation must fit the narrow type its class stores tables in
        if (L.f_tab_type[fi] != TAB_FULL && narrowest_tab_type(parent, total, (int)sizeof(T)) < L.f_tab_type[fi]) {
            int rc = widen_factor(fi);
            if (rc) return rc;
        }
        return MXS_OK;
    }

    int slice_factor(int32_t factor, const int32_t* ext_idx) override {
        HIP_TRY(hipSetDevice(device));
        if (factor < 0 || factor >= L.n_factors) return fail(MXS_E_INVALID, "factor out of range");
        const int fi = L.factor_e2i[factor];
        auto it = parents.find(fi);
        if (it == parents.end()) return fail(MXS_E_STATE, "no parent relation registered for this factor");
        const ParentTab& pt = *it->second;
        const int nd = (int)pt.dims.size();
        SliceDims sd{};
        int64_t stride = 1;
        std::vector<int64_t> strides(nd);
        for (int i = nd - 1; i >= 0; --i) {
            strides[i] = stride;
            stride *= pt.dims[i];
        }
        int j = 0;
        for (int i = 0; i < nd; ++i) {
            if (pt.ext[i]) {
                const int32_t x = ext_idx ? ext_idx[j] : -1;
                if (x < 0 || x >= pt.dims[i]) return fail(MXS_E_INVALID, "external value index out of its domain");
                sd.base += (int64_t)x * strides[i];
                ++j;
            } else {
                sd.dom[sd.n] = pt.dims[i];
                sd.stride[sd.n] = strides[i];
                ++sd.n;
            }
        }
        { int rc = sync(); if (rc) return rc; }
        const int64_t n = L.eval_tab_off[fi + 1] - L.eval_tab_off[fi];
        const int ctype = L.f_tab_type[fi];
        NaryPlace place{};   // narrow image of a workgroup-per-factor table (nt == 0 && box == 0: a register class)
        const NaryLaunch* grp = L.f_class[fi] < 0 && L.f_ndesc[fi] >= 0 ? launch_of(fi) : nullptr;
        const bool image = ctype != TAB_FULL || (grp && is_bin2(grp->box));  // (a lane-grid factor: an image at every width)
        if (image && L.f_class[fi] < 0) place = nary_place(*grp, L.ndesc[L.f_ndesc[fi]], (int)sizeof(T));
        else place.elem = tab_elem_bytes(ctype);
        hipLaunchKernelGGL((k_table_slice<T>), dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, stream,
                           tables.p, L.f_tab_base[fi], (int64_t)L.f_tab_stride[fi],
                           eval_tables.p + L.eval_tab_off[fi], (const double*)pt.buf.p, sd,
                           L.is_max ? -1.0 : 1.0, n,
                           image ? ctables.p + L.f_ctab_off[fi] : (uint8_t*)nullptr, ctype, place);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(stream));
        return MXS_OK;
    }

    // ---- halo -------------------------------------------------------------
    int build_elem_offsets(const int32_t* edges, int64_t n, std::vector<int64_t>& out) {
        out.clear();
        for (int64_t i = 0; i < n; ++i) {
            const int32_t e = edges[i];
            if (e < 0 || e >= L.n_edges) return fail(MXS_E_INVALID, "halo edge out of range");
            const int ei = L.edge_e2i[e];
            for (int d = 0; d < L.edge_dom[ei]; ++d) out.push_back((int64_t)L.v2f_off[ei] + d);
        }
        return MXS_OK;
    }

    std::vector<int32_t> send_ei, recv_ei;  // halo lists as internal edge ids, in the caller's order

    int halo_setup(const int32_t* se, int64_t ns, const int32_t* re, int64_t nr) override {
        HIP_TRY(hipSetDevice(device));
        if (direct) return fail(MXS_E_STATE, "mxs_halo_setup: the direct exchange is already set up");
        std::vector<int64_t> so, ro;
        int rc = build_elem_offsets(se, ns, so);
        if (rc) return rc;
        rc = build_elem_offsets(re, nr, ro);
        if (rc) return rc;
        send_ei.resize((size_t)ns);
        recv_ei.resize((size_t)nr);
        for (int64_t i = 0; i < ns; ++i) send_ei[i] = L.edge_e2i[se[i]];
        for (int64_t i = 0; i < nr; ++i) recv_ei[i] = L.edge_e2i[re[i]];
        n_halo_send = (int64_t)so.size();
        n_halo_recv = (int64_t)ro.size();
        HIP_TRY(halo_send_off.upload(so, stream));
        HIP_TRY(halo_recv_off.upload(ro, stream));
        HIP_TRY(halo_send.alloc((size_t)n_halo_send));
        HIP_TRY(halo_recv.alloc((size_t)n_halo_recv));
        send_buf = halo_send.p;
        recv_buf = halo_recv.p;
        halo_ready = true;
        // Fused sharded launch: ONE sweep per cycle whose last blocks -- the cut factor
        // classes -- wait for the halo exchange inside the kernel.  While they wait they
        // hold workgroup slots, and the pack / RCCL / unpack kernels they wait for need
        // slots too: only when the cut blocks are few (at most half of the 2048
        // resident slots), and there is no cut work outside the sweep launch.
        {
            bool cut_nary = false;
            for (const NaryLaunch& nl : L.nary_launches) cut_nary = cut_nary || nl.cut;
            const char* env = getenv("MAXSUM_SHARD_FUSED");
            fused = L.n_blocks_fused > 0 && L.n_blocks_sweep2 > 0 && L.n_blocks_sweep2 <= FUSED_MAX_CUT_BLOCKS &&
                    !cut_nary && env && env[0] == '1';  // measured slower than two launches: opt-in
            if (fused) launches_per_cycle -= 1;  // the two sweep launches are one
        }
        // the start messages of cycle 0 have to cross too: pack them now
        HIP_TRY(hipEventRecord(ev_p1, stream));
        return pack();
    }

    // comm stream: wait until the variables of the current cycle are done, then gather the
    // V->F messages of the cut edges this shard owns into the send buffer
    int pack() {
        HIP_TRY(hipStreamWaitEvent(comm, ev_p1, 0));
        if (direct) {  // padded records into the send buffer of the current parity
            if (n_send_pad > 0) {
                const int nb = (int)((n_send_pad + BLOCK - 1) / BLOCK);
                hipLaunchKernelGGL((k_halo_pack<T>), dim3(nb), dim3(BLOCK), 0, comm, (const T*)v2f[cur].p,
                                   (const int64_t*)halo_send_off.p, send2[cur].p, n_send_pad);
                HIP_TRY(hipGetLastError());
            }
            return MXS_OK;
        }
        if (n_halo_send > 0) {
            const int nb = (int)((n_halo_send + BLOCK - 1) / BLOCK);
            hipLaunchKernelGGL((k_halo_pack<T>), dim3(nb), dim3(BLOCK), 0, comm,
                               (const T*)v2f[cur].p, (const int64_t*)halo_send_off.p, send_buf,
                               n_halo_send);
            HIP_TRY(hipGetLastError());
        }
        return MXS_OK;
    }

    int halo_buffers(void** s, int64_t* sb, void** r, int64_t* rb) override {
        if (s) *s = send_buf;
        if (sb) *sb = n_halo_send * (int64_t)sizeof(T);
        if (r) *r = recv_buf;
        if (rb) *rb = n_halo_recv * (int64_t)sizeof(T);
        return MXS_OK;
    }

    int halo_bind(void* s, void* r) override {
        if (!halo_ready) return fail(MXS_E_STATE, "mxs_halo_bind needs mxs_halo_setup first");
        if ((n_halo_send && !s) || (n_halo_recv && !r)) return fail(MXS_E_INVALID, "null halo buffer");
        HIP_TRY(hipSetDevice(device));
        send_buf = (T*)s;
        recv_buf = (T*)r;
        return pack();
    }

    // One sharded cycle, split so that the halo exchange of cycle t hides behind the work
    // of cycle t+1 that does not need it:
    //   compute stream   phase 1 (t): variables + interior factors      [record ev_p1]
    //                    wait ev_halo (exchange of t-1 unpacked)
    //                    phase 2 (t): cut factors -- the only readers of ghost messages
    //   comm stream      wait ev_p1 ; pack (t) ; <the host's collective> ; unpack (t) [record ev_halo]
    // Ping-pong buffers keep the two streams on disjoint data.
    int step_compute() override {
        HIP_TRY(hipSetDevice(device));
        if (p2p) {  // one launch (it stores the cut-edge records at the peers) + the publish
            int rc = launch_phase(cur, false, 3);
            if (rc) return rc;
            cur ^= 1;
            cycles += 1;
            return p2p_publish();
        }
        if (fused) {
            // compute stream: one launch per cycle, nothing to wait for on the host side --
            // the cut factor blocks (last of the grid) wait for halo_flags[0] themselves;
            // comm stream: wait for the launch, pack, <collective>, unpack (publishes the epoch)
            int rc = launch_phase(cur, false, 3);
            if (rc) return rc;
            HIP_TRY(hipEventRecord(ev_p1, stream));
            cur ^= 1;
            cycles += 1;
            return direct ? MXS_OK : pack();
        }
        // (Round 5: the cut factor classes on a stream of their own BESIDE launch 1 -- they read nothing launch 1 of the same
        // cycle writes -- measured SLOWER than behind it: shard 0 of the 8-way cut of configs[3] 53.1 us per RCCL-loopback cycle
        // against 50.7 (profiles/r05_shard_cut_beside_ab_v1.txt): the chain launch 1 (t) -> exchange (t) -> launch 2 (t+1) ->
        // launch 1 (t+2) then crosses three streams, and every crossing costs more than the 17 us it could hide.  Removed.)
        int rc = launch_phase(cur, false, 1);
        if (rc) return rc;
        HIP_TRY(hipEventRecord(ev_p1, stream));
        if (halo_pending) HIP_TRY(hipStreamWaitEvent(stream, ev_halo, 0));
        rc = launch_phase(cur, false, 2);
        if (rc) return rc;
        cur ^= 1;
        cycles += 1;
        if (direct) return MXS_OK;  // the variable kernel has written the send buffer itself
        return pack();  // comm stream, behind ev_p1: one host call per cycle before the collective
    }

    int step_pack() override {  // kept for callers that pack separately: packs again (idempotent)
        HIP_TRY(hipSetDevice(device));
        return pack();
    }

    int step_unpack() override {
        HIP_TRY(hipSetDevice(device));
        if (p2p) return MXS_OK;  // nothing to unpack: the peers store into the ghost regions
        if (direct) {  // RCCL has received straight into the ghost slots
            if (fused) {
                ++unpacks;
                hipLaunchKernelGGL(k_halo_publish, dim3(1), dim3(1), 0, comm, halo_flags.p, unpacks);
                HIP_TRY(hipGetLastError());
            }
            HIP_TRY(hipEventRecord(ev_halo, comm));
            halo_pending = true;
            return MXS_OK;
        }
        if (n_halo_recv > 0) {
            const int nb = (int)((n_halo_recv + BLOCK - 1) / BLOCK);
            hipLaunchKernelGGL((k_halo_unpack<T>), dim3(nb), dim3(BLOCK), 0, comm, v2f[cur].p,
                               (const int64_t*)halo_recv_off.p, (const T*)recv_buf, n_halo_recv);
            HIP_TRY(hipGetLastError());
        }
        if (fused) {
            ++unpacks;
            hipLaunchKernelGGL(k_halo_publish, dim3(1), dim3(1), 0, comm, halo_flags.p, unpacks);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipEventRecord(ev_halo, comm));
        halo_pending = true;
        return MXS_OK;
    }

    // ---- native exchange: the engine calls RCCL itself -----------------------------------
    // One exchange = one group of ncclSend / ncclRecv per peer with the fixed counts of the
    // partition (an all-to-all with unequal splits) on the comm stream, between the pack and
    // the unpack of the cycle.  The cycle loop of a sharded run then stays in this library.
    // Direct exchange (set up by comm_init when the shard allows it): the variable kernel
    // writes the records of cut edges straight into a send buffer (no pack kernel), RCCL
    // receives straight into the ghost slots of the V2F buffer, laid out in receive order
    // (no unpack kernel).  What stays on the comm stream per cycle is the collective alone.
    bool direct = false;
    DevBuf<T> send2[2];             // padded records (H elements), one buffer per cycle parity
    DevBuf<int32_t> send_slot;      // per lane of the packed variable classes: record index / -1
    int64_t ghost_base = 0;         // element offset of the ghost region in a V2F buffer
    int64_t n_send_pad = 0;         // elements of a padded send buffer
    std::vector<int64_t> psend_cnt, precv_cnt, psend_at, precv_at;  // padded elements, per peer
    // Peer-store exchange: no collective and no comm stream.  Every rank maps the ghost buffer
    // and the flag words of every other rank (hipIpc); the variable kernel stores cut-edge
    // records straight into the peer's ghost region, a tiny kernel behind each launch publishes
    // the launch number in the peers' flag words, and a cycle is ONE fused launch whose cut
    // factor blocks poll those words.  Ghost regions are three deep: a peer may run one launch
    // ahead of this rank, never two (its next launch cannot finish before it has seen this one).
    bool p2p = false;
    uint32_t gen = 0;                 // publishes done by this rank (the same on every rank)
    DevBuf<T> ghost3;                 // 3 ghost regions + 1 region of zeros (start cycle), ghost_len each
    int64_t ghost_len = 0;            // elements per region (padded records, receive order)
    T* peer_ghost[MXS_MAX_PEERS] = {};      // peer q's ghost3 (mapped), nullptr for this rank
    uint32_t* peer_flag[MXS_MAX_PEERS] = {};
    bool peer_local[MXS_MAX_PEERS] = {};    // mapped without IPC (a shard of this process)
    int64_t peer_len[MXS_MAX_PEERS] = {};   // peer q's ghost_len
    int64_t peer_at[MXS_MAX_PEERS] = {};    // where my block starts inside a region of peer q
    int32_t peer_first[MXS_MAX_PEERS] = {}; // my send slots [peer_first[q], ...) go to peer q
    std::vector<int64_t> pexp_send, pexp_recv;  // counts given to peer_export
    const Rccl* rccl = nullptr;
    void* nccl_comm = nullptr;
    int comm_rank = 0, comm_world = 0;
    std::vector<int64_t> send_cnt, recv_cnt, send_at, recv_at;  // elements, per peer
    DevBuf<T> self_pad;  // world 1: one padding element sent to ourselves

    int comm_init(const char* path, int rank, int world, const uint8_t* id, const int64_t* sc,
                  const int64_t* rc) override {
        if (!halo_ready) return fail(MXS_E_STATE, "mxs_comm_init needs mxs_halo_setup first");
        if (nccl_comm) return fail(MXS_E_STATE, "the communicator of this engine exists already");
        if (world < 1 || rank < 0 || rank >= world || !id || !sc || !rc)
            return fail(MXS_E_INVALID, "mxs_comm_init: bad rank / world / counts");
        int64_t ts = 0, tr = 0;
        for (int q = 0; q < world; ++q) {
            if (sc[q] < 0 || rc[q] < 0) return fail(MXS_E_INVALID, "mxs_comm_init: negative count");
            ts += sc[q];
            tr += rc[q];
        }
        // (a rank exchanges nothing with itself; only the one-rank communicator of
        // tools/shard_cost.py loops a shard's whole halo back to measure the exchange)
        if (ts != n_halo_send || tr != n_halo_recv || (world > 1 && (sc[rank] != 0 || rc[rank] != 0)))
            return fail(MXS_E_INVALID, "mxs_comm_init: counts do not match the halo lists of mxs_halo_setup");
        std::string err;
        rccl = load_rccl(path, err);
        if (!rccl) return fail(MXS_E_COMM, err);
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(self_pad.alloc(64));
        NcclUniqueId uid;
        std::memcpy(uid.internal, id, MXS_UNIQUE_ID_BYTES);
        NCCL_TRY(rccl->CommInitRank(&nccl_comm, world, uid, rank));
        comm_rank = rank;
        comm_world = world;
        send_cnt.assign(sc, sc + world);
        recv_cnt.assign(rc, rc + world);
        send_at.assign(world, 0);
        recv_at.assign(world, 0);
        for (int q = 1; q < world; ++q) {
            send_at[q] = send_at[q - 1] + send_cnt[q - 1];
            recv_at[q] = recv_at[q - 1] + recv_cnt[q - 1];
        }
        return setup_direct();
    }

    // Try to switch the shard to the direct exchange.  Not an error when the shard does not
    // qualify (pack / unpack kernels and the compact staging buffers stay in use then).
    int setup_direct() {
        const char* env = getenv("MAXSUM_SHARD_DIRECT");
        if ((env && env[0] == '0') || send_buf != halo_send.p) return MXS_OK;
        const int nE = L.n_edges;
        // (1)-(3) what both exchanges need (plan_direct): every sent edge is a lane of a packed variable class
        // and is sent once, the received edges are exactly the ghost edges, the per-peer ranges, one record length
        std::vector<int32_t> slot;
        int64_t g_len = 0;
        int Hs = 0;
        if (!plan_direct(slot, g_len, Hs)) return MXS_OK;
        // here the ghost records stay in the V2F array itself: they must be one block of it
        int64_t n_ghost = 0, g0 = INT64_MAX;
        for (int ei = 0; ei < nE; ++ei)
            if (!L.owned[L.edge_var_int[ei]]) {
                ++n_ghost;
                g0 = std::min<int64_t>(g0, L.v2f_off[ei]);
            }
        if (n_ghost && g0 + g_len > L.v2f_elems) return MXS_OK;
        n_send_pad = (int64_t)send_ei.size() * Hs;
        { int rc = sync(); if (rc) return rc; }
        // (4) ghost slots in receive order
        ghost_base = n_ghost ? g0 : 0;
        int64_t at = ghost_base;
        for (int32_t ei : recv_ei) {
            L.v2f_off[ei] = (int32_t)at;
            at += L.edge_half[ei];
        }
        for (int k = 0; k < nE; ++k) L.vslot_v2f[k] = L.v2f_off[L.vslot_edge[k]];
        for (NaryDesc& d : L.ndesc)
            for (int i = 0; i < (d.arity & 255); ++i) d.v2f_off[i] = L.v2f_off[d.edge_base + i];
        HIP_TRY(hipMemcpyAsync(edge_v2f.p, L.v2f_off.data(), sizeof(int32_t) * (size_t)nE, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(vslot_v2f.p, L.vslot_v2f.data(), sizeof(int32_t) * (size_t)nE, hipMemcpyHostToDevice, stream));
        if (!L.ndesc.empty())
            HIP_TRY(hipMemcpyAsync(ndesc.p, L.ndesc.data(), sizeof(NaryDesc) * L.ndesc.size(), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        // (5) padded send buffers + the lanes' slots; pack offsets in the padded format
        for (int b = 0; b < 2; ++b) {
            HIP_TRY(send2[b].alloc((size_t)std::max<int64_t>(n_send_pad, 1)));
            HIP_TRY(hipMemsetAsync(send2[b].p, 0, sizeof(T) * (size_t)std::max<int64_t>(n_send_pad, 1), stream));
        }
        HIP_TRY(send_slot.upload(slot, stream));
        std::vector<int64_t> so;
        for (int32_t ei : send_ei)
            for (int d = 0; d < L.edge_half[ei]; ++d) so.push_back((int64_t)L.v2f_off[ei] + d);
        HIP_TRY(halo_send_off.upload(so, stream));
        direct = true;
        // the messages of the current cycle (the start messages right after mxs_create): packed
        // by the generic kernel this once, later cycles write the send buffer themselves
        return pack();
    }

    int comm_exchange() override {
        if (p2p) return MXS_OK;  // the launches exchange by themselves
        if (!nccl_comm) return fail(MXS_E_STATE, "no communicator: call mxs_comm_init first");
        HIP_TRY(hipSetDevice(device));
        const int dt = sizeof(T) == 8 ? NCCL_F64 : NCCL_F32;
        if (direct) {
            // send buffer of the cycle just enqueued (written by its variable kernel: wait for
            // it), ghost slots of the V2F buffer that cycle wrote
            HIP_TRY(hipStreamWaitEvent(comm, ev_p1, 0));
            NCCL_TRY(rccl->GroupStart());
            if (comm_world == 1 && psend_cnt[0] == 0) {
                NCCL_TRY(rccl->Send(self_pad.p, 1, dt, 0, nccl_comm, comm));
                NCCL_TRY(rccl->Recv(self_pad.p + 32, 1, dt, 0, nccl_comm, comm));
            }
            for (int q = 0; q < comm_world; ++q) {
                if (psend_cnt[q])
                    NCCL_TRY(rccl->Send(send2[cur].p + psend_at[q], (size_t)psend_cnt[q], dt, q, nccl_comm, comm));
                if (precv_cnt[q])
                    NCCL_TRY(rccl->Recv(v2f[cur].p + ghost_base + precv_at[q], (size_t)precv_cnt[q], dt, q,
                                        nccl_comm, comm));
            }
            NCCL_TRY(rccl->GroupEnd());
            return MXS_OK;
        }
        NCCL_TRY(rccl->GroupStart());
        if (comm_world == 1 && send_cnt[0] == 0) {
            // nothing crosses; one padding element to ourselves keeps the very call sequence
            // of a multi-GPU run testable on a one-GPU box
            NCCL_TRY(rccl->Send(self_pad.p, 1, dt, 0, nccl_comm, comm));
            NCCL_TRY(rccl->Recv(self_pad.p + 32, 1, dt, 0, nccl_comm, comm));
        }
        for (int q = 0; q < comm_world; ++q) {
            if (send_cnt[q])
                NCCL_TRY(rccl->Send(send_buf + send_at[q], (size_t)send_cnt[q], dt, q, nccl_comm, comm));
            if (recv_cnt[q])
                NCCL_TRY(rccl->Recv(recv_buf + recv_at[q], (size_t)recv_cnt[q], dt, q, nccl_comm, comm));
        }
        NCCL_TRY(rccl->GroupEnd());
        return MXS_OK;
    }

    bool peer_mode() const override { return p2p; }

    // ONE planner for the direct RCCL exchange (setup_direct) and the peer-store exchange (peer_export), from
    // comm_world / send_cnt / recv_cnt: the lanes' slots in the send buffer (every sent edge is a lane of a packed
    // variable class and is sent once), the received edges = the ghost edges, each once (g_len = their elements),
    // the halo lists split by peer (psend_* / precv_*), one record length on the send side (Hs).
    // false: the shard does not qualify (pack / unpack kernels and the compact staging buffers stay in use).
    bool plan_direct(std::vector<int32_t>& slot, int64_t& g_len, int& Hs) {
        const int nE = L.n_edges;
        const int world = comm_world;
        slot.assign(L.vell.size(), -1);
        std::vector<const ClassInfo*> packed;
        for (const ClassInfo& ci : L.classes)
            if (ci.kind == K_V_PACK) packed.push_back(&ci);
        for (size_t i = 0; i < send_ei.size(); ++i) {
            const int64_t off = L.v2f_off[send_ei[i]];
            const ClassInfo* home = nullptr;
            for (const ClassInfo* ci : packed)
                if (off >= ci->v2f_base && off < ci->v2f_base + (int64_t)ci->count * ci->H) home = ci;
            if (!home) return false;
            const int64_t pos = home->ell_base + (off - home->v2f_base) / home->H;
            if (slot[pos] >= 0) return false;
            slot[pos] = (int32_t)i;
        }
        std::vector<uint8_t> seen(nE, 0);
        int64_t n_ghost = 0;
        g_len = 0;
        for (int ei = 0; ei < nE; ++ei)
            if (!L.owned[L.edge_var_int[ei]]) ++n_ghost;
        if ((int64_t)recv_ei.size() != n_ghost) return false;
        for (int32_t ei : recv_ei) {
            if (L.owned[L.edge_var_int[ei]] || seen[ei]) return false;
            seen[ei] = 1;
            g_len += L.edge_half[ei];
        }
        auto split = [&](const std::vector<int32_t>& edges, const std::vector<int64_t>& cnt,
                         std::vector<int64_t>& pcnt, std::vector<int64_t>& pat) -> bool {
            pcnt.assign(world, 0);
            pat.assign(world, 0);
            size_t i = 0;
            int64_t at = 0;
            for (int q = 0; q < world; ++q) {
                pat[q] = at;
                int64_t left = cnt[q];
                while (left > 0 && i < edges.size()) {
                    left -= L.edge_dom[edges[i]];
                    pcnt[q] += L.edge_half[edges[i]];
                    ++i;
                }
                if (left != 0) return false;
                at += pcnt[q];
            }
            return i == edges.size();
        };
        if (!split(send_ei, send_cnt, psend_cnt, psend_at) || !split(recv_ei, recv_cnt, precv_cnt, precv_at))
            return false;
        Hs = 0;
        for (int32_t ei : send_ei) {
            if (Hs == 0) Hs = L.edge_half[ei];
            if (L.edge_half[ei] != Hs) return false;
        }
        return true;
    }

    // Peer-store exchange, step 1: decide whether this shard qualifies, allocate the ghost
    // regions and the flag words, and describe them for the other ranks.
    int peer_export(int rank, int world, const int64_t* sc, const int64_t* rc, mxs_peer_info* out) override {
        if (!out) return fail(MXS_E_INVALID, "null argument");
        std::memset(out, 0, sizeof(*out));
        if (!halo_ready) return fail(MXS_E_STATE, "mxs_peer_export needs mxs_halo_setup first");
        if (p2p || direct || nccl_comm) return fail(MXS_E_STATE, "the exchange of this shard is already set up");
        if (world < 2 || world > MXS_MAX_PEERS || rank < 0 || rank >= world || !sc || !rc)
            return fail(MXS_E_INVALID, "mxs_peer_export: 2..8 ranks of one node");
        HIP_TRY(hipSetDevice(device));
        comm_rank = rank;
        // the fused launch has to be possible (cut factor work inside the sweep launch, few
        // enough cut blocks) and the cut factors must be binary register classes (they are the
        // ones that address the ghost region)
        bool ok = L.n_blocks_fused > 0 && L.n_blocks_sweep2 > 0 && L.n_blocks_sweep2 <= FUSED_MAX_CUT_BLOCKS &&
                  send_buf == halo_send.p;
        for (const NaryLaunch& nl : L.nary_launches) ok = ok && !nl.cut;
        for (int c : L.sweep_order2) ok = ok && L.classes[c].kind == K_F_BIN;
        std::vector<int32_t> slot;
        int Hs = 0;
        comm_world = world;
        send_cnt.assign(sc, sc + world);
        recv_cnt.assign(rc, rc + world);
        ok = ok && plan_direct(slot, ghost_len, Hs);
        ok = ok && L.v2f_elems + ghost_len < ((int64_t)1 << 31) - 8192;
        const char* env = getenv("MAXSUM_SHARD_P2P");
        if (env && env[0] == '0') ok = false;
        if (!ok) return MXS_OK;  // out->qualifies stays 0: the caller falls back to RCCL
        ghost_len = (ghost_len + 63) / 64 * 64;
        HIP_TRY(ghost3.alloc((size_t)(4 * std::max<int64_t>(ghost_len, 64))));
        HIP_TRY(hipMemsetAsync(ghost3.p, 0, sizeof(T) * ghost3.n, stream));
        HIP_TRY(hipMemsetAsync(halo_flags.p, 0, 64 * sizeof(uint32_t), stream));
        HIP_TRY(send_slot.upload(slot, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        hipIpcMemHandle_t hg, hf;
        HIP_TRY(hipIpcGetMemHandle(&hg, ghost3.p));
        HIP_TRY(hipIpcGetMemHandle(&hf, halo_flags.p));
        static_assert(sizeof(hg) == MXS_IPC_HANDLE_BYTES, "hipIpcMemHandle_t is 64 bytes");
        std::memcpy(out->ghost_handle, &hg, MXS_IPC_HANDLE_BYTES);
        std::memcpy(out->flag_handle, &hf, MXS_IPC_HANDLE_BYTES);
        out->pid = (int64_t)getpid();
        out->ghost_ptr = (uint64_t)(uintptr_t)ghost3.p;
        out->flag_ptr = (uint64_t)(uintptr_t)halo_flags.p;
        out->qualifies = 1;
        out->rank = rank;
        out->ghost_len = ghost_len;
        for (int q = 0; q < world; ++q) {
            out->recv_at[q] = precv_at[q];     // where rank q's block starts inside my regions
            out->recv_len[q] = precv_cnt[q];   // ... and how long it is (checked against q's sends)
        }
        pexp_send.assign(sc, sc + world);
        pexp_recv.assign(rc, rc + world);
        return MXS_OK;
    }

    // Step 2 (every rank holds every rank's mxs_peer_info, all of them qualifying): map the
    // peers' buffers, point the ghost edges at the ghost region, push the current records.
    int peer_connect(const mxs_peer_info* all) override {
        if (!all) return fail(MXS_E_INVALID, "null argument");
        if (pexp_send.empty() || p2p) return fail(MXS_E_STATE, "mxs_peer_connect needs mxs_peer_export first");
        HIP_TRY(hipSetDevice(device));
        const int world = comm_world, me = comm_rank;
        for (int q = 0; q < world; ++q) {
            if (!all[q].qualifies || all[q].rank != q) return fail(MXS_E_INVALID, "mxs_peer_connect: a rank does not qualify");
            if (q != me && all[q].recv_len[me] != psend_cnt[q])
                return fail(MXS_E_INVALID, "mxs_peer_connect: what a peer expects from this rank is not what it sends");
        }
        for (int q = 0; q < world; ++q) {
            peer_first[q] = (int32_t)(psend_at[q] / std::max<int64_t>(1, send_ei.empty() ? 1 : L.edge_half[send_ei[0]]));
            peer_len[q] = all[q].ghost_len;
            peer_at[q] = all[q].recv_at[me];
            if (q == me) continue;
            if (all[q].pid == (int64_t)getpid()) {  // a shard of this very process: no IPC needed
                peer_ghost[q] = (T*)(uintptr_t)all[q].ghost_ptr;
                peer_flag[q] = (uint32_t*)(uintptr_t)all[q].flag_ptr;
                peer_local[q] = true;
                continue;
            }
            hipIpcMemHandle_t hg, hf;
            std::memcpy(&hg, all[q].ghost_handle, MXS_IPC_HANDLE_BYTES);
            std::memcpy(&hf, all[q].flag_handle, MXS_IPC_HANDLE_BYTES);
            void *pg = nullptr, *pf = nullptr;
            HIP_TRY(hipIpcOpenMemHandle(&pg, hg, hipIpcMemLazyEnablePeerAccess));
            HIP_TRY(hipIpcOpenMemHandle(&pf, hf, hipIpcMemLazyEnablePeerAccess));
            peer_ghost[q] = (T*)pg;
            peer_flag[q] = (uint32_t*)pf;
        }
        { int rc = sync(); if (rc) return rc; }
        // ghost edges address the ghost region: V2F offsets >= v2f_elems, in receive order
        const int nE = L.n_edges;
        int64_t at = L.v2f_elems;
        for (int32_t ei : recv_ei) {
            L.v2f_off[ei] = (int32_t)at;
            at += L.edge_half[ei];
        }
        for (int k = 0; k < nE; ++k) L.vslot_v2f[k] = L.v2f_off[L.vslot_edge[k]];
        HIP_TRY(hipMemcpyAsync(edge_v2f.p, L.v2f_off.data(), sizeof(int32_t) * (size_t)nE, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(vslot_v2f.p, L.vslot_v2f.data(), sizeof(int32_t) * (size_t)nE, hipMemcpyHostToDevice, stream));
        // offsets of the padded records of the send order (k_p2p_push)
        std::vector<int64_t> so;
        for (int32_t ei : send_ei)
            for (int d = 0; d < L.edge_half[ei]; ++d) so.push_back((int64_t)L.v2f_off[ei] + d);
        n_send_pad = (int64_t)so.size();
        HIP_TRY(halo_send_off.upload(so, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        p2p = true;
        fused = true;
        launches_per_cycle = 1 + n_wide_launches() + (int)L.nary_launches.size();
        gen = 0;
        return p2p_push();
    }

    // Store the CURRENT records of the cut edges into the peers' next ghost region and publish:
    // the state right after mxs_create / mxs_reset, whose start cycle ran before any peer was
    // listening (reset) or mapped (create).  Counts as one publish on every rank.
    int p2p_push() {
        if (n_send_pad > 0) {
            PeerDst<T> dst{};
            for (int q = 0; q < MXS_MAX_PEERS; ++q) {
                dst.first[q] = q < comm_world ? peer_first[q] : INT32_MAX;
                dst.p[q] = (q < comm_world && peer_ghost[q])
                               ? peer_ghost[q] + (int64_t)((gen + 1) % 3) * peer_len[q] + peer_at[q] : nullptr;
            }
            const int Hs = L.edge_half[send_ei[0]];
            const int nb = (int)((n_send_pad + BLOCK - 1) / BLOCK);
            hipLaunchKernelGGL((k_p2p_push<T>), dim3(nb), dim3(BLOCK), 0, stream, (const T*)v2f[cur].p,
                               (const int64_t*)halo_send_off.p, dst, Hs, n_send_pad);
            HIP_TRY(hipGetLastError());
        }
        return p2p_publish();
    }

    // The publish runs on the compute stream, right behind the launch it announces (+2.5 us
    // per cycle).  $MAXSUM_P2P_PUBLISH=comm moves it to the comm stream behind an event so that
    // the next launch starts at once -- measured slower (34.7 vs 30.3 us per cycle with the
    // exchange looped back): the event + dispatch latency delays the flag beyond the ~15 us the
    // cut blocks of the next launch can wait for free.
    int p2p_publish() {
        ++gen;
        PeerFlags pf{};
        for (int q = 0; q < MXS_MAX_PEERS; ++q) pf.p[q] = q < comm_world ? peer_flag[q] : nullptr;
        static const bool inline_publish = [] {
            const char* e = getenv("MAXSUM_P2P_PUBLISH");
            return !(e && std::string(e) == "comm");
        }();
        hipStream_t st = stream;
        if (!inline_publish) {
            HIP_TRY(hipEventRecord(ev_p1, stream));
            HIP_TRY(hipStreamWaitEvent(comm, ev_p1, 0));
            st = comm;
        }
        hipLaunchKernelGGL(k_p2p_publish, dim3(1), dim3(64), 0, st, pf, comm_rank, comm_world, gen);
        HIP_TRY(hipGetLastError());
        return MXS_OK;
    }

    void shard_mode(int32_t* f, int32_t* d) const override {
        if (f) *f = fused ? 1 : 0;
        if (d) *d = p2p ? 2 : direct ? 1 : 0;
    }

    int run_sharded(int n) override {
        if (n < 0) return fail(MXS_E_INVALID, "n_cycles must be >= 0");
        for (int i = 0; i < n; ++i) {
            int rc = step_compute();  // both phases + pack
            if (rc) return rc;
            rc = comm_exchange();
            if (rc) return rc;
            rc = step_unpack();
            if (rc) return rc;
        }
        return MXS_OK;
    }
};

}  // namespace mxs

struct mxs_engine {
    std::unique_ptr<mxs::EngineBase> impl;
};

using mxs::fail;
using mxs::g_err;

#define CHECK_HANDLE(e)                                           \
    do {                                                          \
        if (!(e) || !(e)->impl) return fail(MXS_E_INVALID, "null engine handle"); \
    } while (0)

extern "C" {

int mxs_device_count(int32_t* count) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        n = 0;
    }
    if (count) *count = n;
    return MXS_OK;
}

int mxs_create(const mxs_graph* g, const mxs_params* p, int32_t device, mxs_engine** out) {
    if (!g || !p || !out) return fail(MXS_E_INVALID, "null argument");
    *out = nullptr;
    try {
        std::unique_ptr<mxs::EngineBase> impl;
        if (p->dtype == MXS_DTYPE_F32) impl.reset(new mxs::Engine<float>());
        else if (p->dtype == MXS_DTYPE_F64) impl.reset(new mxs::Engine<double>());
        else return fail(MXS_E_INVALID, "invalid dtype");
        int rc = impl->init(*g, *p, device);
        if (rc) return rc;
        *out = new mxs_engine{std::move(impl)};
        return MXS_OK;
    } catch (const std::bad_alloc&) {
        return fail(MXS_E_NOMEM, "out of host memory");
    } catch (const std::exception& ex) {
        return fail(MXS_E_INVALID, ex.what());
    }
}

int mxs_reset(mxs_engine* e) { CHECK_HANDLE(e); return e->impl->reset(); }

int mxs_run(mxs_engine* e, int32_t n) {
    CHECK_HANDLE(e);
    int rc = e->impl->run_async(n);
    if (rc) return rc;
    return e->impl->sync();
}

int mxs_run_timed(mxs_engine* e, int32_t n, float* ms) { CHECK_HANDLE(e); return e->impl->run_timed(n, ms); }
int mxs_run_reps(mxs_engine* e, int32_t n, int32_t reps, float* ms) { CHECK_HANDLE(e); return e->impl->run_reps(n, reps, ms); }
int mxs_run_async(mxs_engine* e, int32_t n) { CHECK_HANDLE(e); return e->impl->run_async(n); }
int mxs_sync(mxs_engine* e) { CHECK_HANDLE(e); return e->impl->sync(); }

int mxs_cycle_count(const mxs_engine* e, int64_t* cycles) {
    CHECK_HANDLE(e);
    if (cycles) *cycles = e->impl->cycles;
    return MXS_OK;
}

int mxs_get_assignment(mxs_engine* e, int32_t* idx, double* belief) {
    CHECK_HANDLE(e);
    return e->impl->get_assignment(idx, belief);
}

int mxs_get_messages(mxs_engine* e, double* v2f, double* f2v, uint8_t* cv, uint8_t* cf) {
    CHECK_HANDLE(e);
    return e->impl->get_messages(v2f, f2v, cv, cf);
}

int mxs_set_state(mxs_engine* e, const double* v2f, const double* f2v, const uint8_t* cv, const uint8_t* cf,
                  const int32_t* idx, const double* belief, int64_t cycles) {
    CHECK_HANDLE(e);
    int rc = e->impl->set_state(v2f, f2v, cv, cf, idx, belief, cycles);
    if (!rc) rc = e->impl->track_restart();
    return rc ? rc : e->impl->quiet_restart();
}

int mxs_table_storage(const mxs_engine* e, int64_t factors[4], int64_t* table_bytes) {
    CHECK_HANDLE(e);
    const mxs::Layout& L = e->impl->L;
    const int64_t w = L.opt.word;
    int64_t n[4] = {0, 0, 0, 0}, bytes = 0;
    for (int fi = 0; fi < L.n_factors; ++fi) {
        const int t = L.f_tab_type[fi];
        const int64_t entries = L.eval_tab_off[fi + 1] - L.eval_tab_off[fi];
        n[t] += 1;
        if (L.f_class[fi] >= 0) bytes += t == mxs::TAB_FULL ? entries * w : L.classes[L.f_class[fi]].ctab_rec;
        else if (L.f_ndesc[fi] < 0) bytes += entries * w;
        else {  // full-width rows, a lane-packed image (D0 * threads * slot), box records, or the lane-grid image of a binary table
            for (const mxs::NaryLaunch& x : L.nary_launches)
                if (L.f_ndesc[fi] >= x.first && L.f_ndesc[fi] < x.first + x.count) {
                    const mxs::NaryDesc& d = L.ndesc[L.f_ndesc[fi]];
                    if (t == mxs::TAB_FULL && !mxs::is_bin2(x.box)) bytes += entries * w;
                    else bytes += mxs::nary_place_bytes(mxs::nary_place(x, d, (int)w), d.dom[0]);
                }
        }
    }
    if (factors) std::memcpy(factors, n, sizeof(n));
    if (table_bytes) *table_bytes = bytes;
    return MXS_OK;
}

int mxs_set_parent_table(mxs_engine* e, int32_t factor, const double* parent, int32_t n_dims,
                         const int32_t* dims, const uint8_t* is_external) {
    CHECK_HANDLE(e);
    int rc = e->impl->set_parent(factor, parent, n_dims, dims, is_external);
    if (!rc) rc = e->impl->track_restart();
    return rc ? rc : e->impl->quiet_restart();
}

int mxs_slice_factor(mxs_engine* e, int32_t factor, const int32_t* external_idx) {
    CHECK_HANDLE(e);
    int rc = e->impl->slice_factor(factor, external_idx);
    if (!rc) rc = e->impl->track_restart();
    return rc ? rc : e->impl->quiet_restart();
}

int mxs_eval_cost(mxs_engine* e, const int32_t* idx, double infinity, double* cost, int64_t* viol) {
    CHECK_HANDLE(e);
    return e->impl->eval_cost(idx, infinity, cost, viol);
}

int mxs_cycle_bytes(const mxs_engine* e, int64_t* bytes, int32_t* launches) {
    CHECK_HANDLE(e);
    if (bytes) *bytes = e->impl->L.algorithmic_bytes;
    if (launches) *launches = e->impl->launches_per_cycle;
    return MXS_OK;
}

int mxs_factor_order(const mxs_engine* e, int32_t* tiled) {
    CHECK_HANDLE(e);
    if (tiled) *tiled = e->impl->L.tiled ? 1 : 0;
    return MXS_OK;
}

int mxs_factor_kernels(const mxs_engine* e, int64_t counts[7]) {
    CHECK_HANDLE(e);
    if (!counts) return MXS_OK;
    const mxs::Layout& L = e->impl->L;
    for (int i = 0; i < 7; ++i) counts[i] = 0;
    for (int fi = 0; fi < L.n_factors; ++fi) {
        if (L.f_class[fi] >= 0) {
            const int k = L.classes[L.f_class[fi]].kind;
            counts[k == mxs::K_F_UNARY ? 0 : k == mxs::K_F_BIN ? 1 : 2] += 1;
        } else if (L.f_ndesc[fi] >= 0) {
            for (const mxs::NaryLaunch& x : L.nary_launches)
                if (L.f_ndesc[fi] >= x.first && L.f_ndesc[fi] < x.first + x.count)
                    counts[mxs::is_small(x.box) ? 6 : mxs::is_bin2(x.box) ? 5 : x.box ? 4 : 3] += 1;
        } else {
            counts[2] += 1;
        }
    }
    return MXS_OK;
}

int mxs_variable_kernels(const mxs_engine* e, int64_t counts[6]) {
    CHECK_HANDLE(e);
    if (!counts) return MXS_OK;
    const mxs::Layout& L = e->impl->L;
    for (int i = 0; i < 6; ++i) counts[i] = 0;
    int64_t swept = 0;
    for (const mxs::ClassInfo& ci : L.classes) {
        int64_t n = 0;
        if (ci.kind == mxs::K_V_PACK || ci.kind == mxs::K_V_PACK8) {  // (count = lanes: the variables are in the wave records)
            for (int64_t w = ci.ell_base >> 6; w < (ci.ell_base + ci.count) >> 6; ++w) n += ((uint32_t)L.vwave[w].deg_nv >> 8) & 255u;
            counts[ci.kind == mxs::K_V_PACK ? 0 : 1] += n;
        } else if (ci.kind == mxs::K_V_WIDE) {
            counts[2] += (n = ci.count);
        } else if (ci.kind == mxs::K_V_GEN && !ci.start_only) {
            counts[3] += (n = ci.count);
        } else if (ci.kind == mxs::K_V_HUB) {  // (count = workgroups: a variable's first one starts at its edge 0)
            for (int32_t w = ci.first; w < ci.first + ci.count; ++w) n += L.hub_blocks[w].ko0 == 0;
            counts[5] += n;
        }
        swept += n;
    }
    counts[4] = L.n_vars - swept;
    return MXS_OK;
}

int mxs_halo_setup(mxs_engine* e, const int32_t* se, int64_t ns, const int32_t* re, int64_t nr) {
    CHECK_HANDLE(e);
    if ((ns && !se) || (nr && !re) || ns < 0 || nr < 0) return fail(MXS_E_INVALID, "bad halo lists");
    if (e->impl->tracking()) return fail(MXS_E_STATE, "mxs_halo_setup: not while mxs_track_best is on (a shard's cost is partial)");
    if (e->impl->watching()) return fail(MXS_E_STATE, "mxs_halo_setup: not while mxs_watch_quiescence is on (a shard sees its own edges only)");
    return e->impl->halo_setup(se, ns, re, nr);
}

int mxs_halo_buffers(mxs_engine* e, void** s, int64_t* sb, void** r, int64_t* rb) {
    CHECK_HANDLE(e);
    return e->impl->halo_buffers(s, sb, r, rb);
}

int mxs_halo_bind(mxs_engine* e, void* s, void* r) { CHECK_HANDLE(e); return e->impl->halo_bind(s, r); }

#define CHECK_UNTRACKED(e, what)                                                                              \
    do {                                                                                                      \
        if ((e)->impl->tracking()) return fail(MXS_E_STATE, what ": not while mxs_track_best is on");         \
        if ((e)->impl->watching()) return fail(MXS_E_STATE, what ": not while mxs_watch_quiescence is on");   \
    } while (0)
int mxs_step_compute(mxs_engine* e) { CHECK_HANDLE(e); CHECK_UNTRACKED(e, "mxs_step_compute"); return e->impl->step_compute(); }
int mxs_step_pack(mxs_engine* e) { CHECK_HANDLE(e); CHECK_UNTRACKED(e, "mxs_step_pack"); return e->impl->step_pack(); }
int mxs_step_unpack(mxs_engine* e) { CHECK_HANDLE(e); CHECK_UNTRACKED(e, "mxs_step_unpack"); return e->impl->step_unpack(); }

int mxs_track_best(mxs_engine* e, int32_t every, double infinity, int32_t trace_capacity) {
    CHECK_HANDLE(e);
    return e->impl->track_best(every, infinity, trace_capacity);
}
int mxs_get_best(mxs_engine* e, int64_t* cycle, double* cost, int64_t* violations, int32_t* idx) {
    CHECK_HANDLE(e);
    return e->impl->get_best(cycle, cost, violations, idx);
}
int mxs_get_cost_trace(mxs_engine* e, int64_t* cycle, double* cost, int64_t* violations, int32_t capacity, int32_t* n,
                       int64_t* evaluations) {
    CHECK_HANDLE(e);
    return e->impl->get_cost_trace(cycle, cost, violations, capacity, n, evaluations);
}

int mxs_watch_quiescence(mxs_engine* e, int32_t every) {
    CHECK_HANDLE(e);
    return e->impl->watch_quiescence(every);
}
int mxs_quiescence(mxs_engine* e, int32_t* quiescent, int64_t* cycle, int64_t* checks, int64_t* active, int64_t* last_check_cycle) {
    CHECK_HANDLE(e);
    return e->impl->quiescence(quiescent, cycle, checks, active, last_check_cycle);
}
int mxs_run_until_quiescent(mxs_engine* e, int32_t max_cycles, int32_t poll, int32_t* quiescent, int64_t* cycle,
                            int64_t* cycles_run) {
    CHECK_HANDLE(e);
    return e->impl->run_until_quiescent(max_cycles, poll, quiescent, cycle, cycles_run);
}

int mxs_comm_unique_id(const char* rccl_path, uint8_t* id) {
    if (!id) return fail(MXS_E_INVALID, "null argument");
    std::string err;
    const mxs::Rccl* rccl = mxs::load_rccl(rccl_path, err);
    if (!rccl) return fail(MXS_E_COMM, err);
    mxs::NcclUniqueId uid;
    int r = rccl->GetUniqueId(&uid);
    if (r != 0) return fail(MXS_E_COMM, std::string("ncclGetUniqueId: ") + rccl->GetErrorString(r));
    std::memcpy(id, uid.internal, MXS_UNIQUE_ID_BYTES);
    return MXS_OK;
}

int mxs_comm_init(mxs_engine* e, const char* rccl_path, int32_t rank, int32_t world, const uint8_t* id,
                  const int64_t* send_counts, const int64_t* recv_counts) {
    CHECK_HANDLE(e);
    return e->impl->comm_init(rccl_path, rank, world, id, send_counts, recv_counts);
}

int mxs_comm_exchange(mxs_engine* e) { CHECK_HANDLE(e); return e->impl->comm_exchange(); }
int mxs_run_sharded(mxs_engine* e, int32_t n) { CHECK_HANDLE(e); return e->impl->run_sharded(n); }

int mxs_peer_export(mxs_engine* e, int32_t rank, int32_t world, const int64_t* send_counts,
                    const int64_t* recv_counts, mxs_peer_info* out) {
    CHECK_HANDLE(e);
    return e->impl->peer_export(rank, world, send_counts, recv_counts, out);
}

int mxs_peer_connect(mxs_engine* e, const mxs_peer_info* all) {
    CHECK_HANDLE(e);
    return e->impl->peer_connect(all);
}

int mxs_shard_mode(const mxs_engine* e, int32_t* fused_launch, int32_t* direct_exchange) {
    CHECK_HANDLE(e);
    e->impl->shard_mode(fused_launch, direct_exchange);
    return MXS_OK;
}

int mxs_stream(mxs_engine* e, void** stream) {
    CHECK_HANDLE(e);
    if (stream) *stream = (void*)e->impl->comm;
    return MXS_OK;
}

int mxs_debug_timeline(mxs_engine* e, int64_t* out, int32_t cap, int32_t* n_blocks) {
    CHECK_HANDLE(e);
    return e->impl->debug_timeline(out, cap, n_blocks);
}

int mxs_update_factor_table(mxs_engine* e, int32_t factor, const double* table, int64_t n) {
    CHECK_HANDLE(e);
    int rc = e->impl->update_table(factor, table, n);
    if (!rc) rc = e->impl->track_restart();
    return rc ? rc : e->impl->quiet_restart();
}

int mxs_destroy(mxs_engine* e) {
    if (!e) return MXS_OK;
    delete e;
    return MXS_OK;
}

const char* mxs_last_error(void) { return g_err.c_str(); }

int32_t mxs_version(void) { return 270; }  // 2.1: + mxs_run_reps, mxs_factor_kernels, mxs_variable_kernels (round 5)
                                           // 2.2: mxs_variable_kernels reports six classes (+ the hub class, round 6)
                                           // 2.3: + mxs_mgm2_*
                                           // 2.4: + mxs_dpop_*
                                           // 2.5: + mxs_gdba_*
                                           // 2.6: + mxs_dba_*
                                           // 2.7: + mxs_dsa_create_replicas, _replicas, _get_state_replica, _replica_costs, _track_best, _get_best
#ifndef MXS_BUILD_KIND   // 1: the hipcc build for gfx950; 0: anything else (the host emulation of tests/emu), refused by the
#if defined(__HIPCC__)   // binding outside tests (pydcop_amd/engine.py, load_library).  Derived from the compiler: a build that
#define MXS_BUILD_KIND 1 // forgets the flag cannot claim to be the device build.
#else
#define MXS_BUILD_KIND 0
#endif
#endif
int32_t mxs_build_kind(void) { return MXS_BUILD_KIND; }
  // 2.0: mxs_graph gained eval_var_cost

}  // extern "C"
