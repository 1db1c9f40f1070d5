// quiescence.h -- the DEVICE side of the Max-Sum engine's end condition (mxs_watch_quiescence,
// include/maxsum_gpu_quiescence.h; the host side is Engine::launch_quiet in engine.hip).  A cycle in which no directed
// edge sends leaves the whole state as it was, so every later cycle is that cycle again.  A send counter is SAME_COUNT
// after a silent cycle AND after a fourth send; two consecutive looks tell them apart: all 2*E counters == SAME_COUNT
// after cycle c-1 and after cycle c  <=>  cycle c sent nothing.  One check is two launches in stream order:
// k_quiet_count leaves per-block counts of the counters != SAME_COUNT, k_quiet_final adds them and applies the rule.
// Nothing is read back and nothing is an atomic; the counts are integers: the same bits from run to run.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"  // SAME_COUNT

namespace mxs {

constexpr int QUIET_MAX_PARTS = 1024;  // the most blocks k_quiet_count is launched with
constexpr int QUIET_TPB = 256;
constexpr uint32_t QUIET_ALL4 = 0x01010101u * (uint32_t)SAME_COUNT;  // four counters at rest in one dword
constexpr uint32_t QUIET_IN_CV = 0x80000000u;                        // QuietTile::n / a byte entry: the cV array, else cF

// the engine's one record, on the device
struct QuietState {
    long long next_cycle;    // the cycle of the next check: a captured graph freezes kernel arguments, so the cycle
                             // number of a check inside a replay comes from here
    long long last_all4;     // the last checked cycle with active == 0 (QUIET_NONE: none)
    long long quiescent_at;  // the first cycle found to have sent nothing, -1 = not yet; never overwritten
    long long checks;        // checks since watching was switched on
    long long active;        // counters != SAME_COUNT at the last check
    long long last_check;    // the cycle of the last check, -1 = none
};
constexpr long long QUIET_NONE = -2;  // (never c - 1 for a check after cycle c >= 1)

// Where the 2*E counters live is the layout's business; the host lists the places once (Engine::build_quiet_lists).
// Counters in the cF / cV byte arrays that fill an aligned 16-byte quad go in TILES of up to 64 consecutive quads, one
// quad per lane of a wave; the bytes left over, and the counters kept behind a message record, go through a gather list.
struct QuietTile {
    uint32_t quad;  // first quad (16-byte unit) in the array
    uint32_t n;     // quads, 1..64; QUIET_IN_CV: of cV
};
struct alignas(16) QuietQuad {
    uint32_t w[4];
};

struct QuietLists {
    const QuietTile* tiles;
    const uint32_t* gather;  // [n_bytes] byte offsets (QUIET_IN_CV: into cV), then [n_f2v] element offsets into the F->V
    int32_t n_tiles;         // buffer, then [n_v2f] into the V->F buffer
    int32_t n_bytes, n_f2v, n_v2f;
    int32_t bits;            // bits of the largest count one lane can reach with the grid of this launch
};

// bytes of x that are not SAME_COUNT
static __device__ __forceinline__ uint32_t quiet_bytes_off(uint32_t x) {
    uint32_t y = x ^ QUIET_ALL4;
    y |= y >> 4;  // (what crosses a byte border lands in bits that the mask drops)
    y |= y >> 2;
    y |= y >> 1;
    return (uint32_t)__builtin_popcount(y & 0x01010101u);
}

// Grid-stride, at most QUIET_MAX_PARTS blocks.  Waves stride over the tiles (one 16-byte load per lane, compared per
// dword), threads stride over the gather list; the lane counts are added per wave with ballots (one per bit plane, ql.bits
// of them: the same number in every wave) and per block through LDS.  part[blockIdx.x] = this block's count.
template <typename T>
static __global__ void __launch_bounds__(QUIET_TPB) k_quiet_count(QuietLists ql, const uint8_t* cF, const uint8_t* cV,
                                                                  const T* f2v, const T* v2f, uint32_t* part) {
    __shared__ uint32_t s_wave[QUIET_TPB / 64];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int waves = QUIET_TPB / 64;
    uint32_t cnt = 0;
    for (int t = (int)blockIdx.x * waves + wave; t < ql.n_tiles; t += (int)gridDim.x * waves) {
        const QuietTile tile = ql.tiles[t];
        if (lane < (int)(tile.n & ~QUIET_IN_CV)) {
            const uint8_t* base = (tile.n & QUIET_IN_CV) ? cV : cF;
            const QuietQuad q = reinterpret_cast<const QuietQuad*>(base)[(size_t)tile.quad + (size_t)lane];
            if ((q.w[0] ^ QUIET_ALL4) | (q.w[1] ^ QUIET_ALL4) | (q.w[2] ^ QUIET_ALL4) | (q.w[3] ^ QUIET_ALL4))
                cnt += quiet_bytes_off(q.w[0]) + quiet_bytes_off(q.w[1]) + quiet_bytes_off(q.w[2]) + quiet_bytes_off(q.w[3]);
        }
    }
    const int n_gather = ql.n_bytes + ql.n_f2v + ql.n_v2f;
    for (int i = (int)(blockIdx.x * QUIET_TPB + threadIdx.x); i < n_gather; i += (int)gridDim.x * QUIET_TPB) {
        const uint32_t at = ql.gather[i];
        bool off;
        if (i < ql.n_bytes) off = ((at & QUIET_IN_CV) ? cV[at & ~QUIET_IN_CV] : cF[at]) != (uint8_t)SAME_COUNT;
        else if (i < ql.n_bytes + ql.n_f2v) off = f2v[at] != (T)SAME_COUNT;
        else off = v2f[at] != (T)SAME_COUNT;
        cnt += off ? 1u : 0u;
    }
    // per wave: bit plane b of the lane counts is one ballot, worth popcount << b
    uint32_t total = 0;
    for (int b = 0; b < ql.bits; ++b) total += (uint32_t)__builtin_popcountll(__ballot((int)((cnt >> b) & 1u))) << b;
    if (lane == 0) s_wave[wave] = total;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int w = 0; w < waves; ++w) s += s_wave[w];
        part[blockIdx.x] = s;
    }
}

// One block.  The partials are staged in LDS by all threads, thread 0 adds them in index order and applies the rule.
// The check is that of cycle st->next_cycle; the next one is the next cycle c with c % every == 0 or c % every == 1.
static __global__ void __launch_bounds__(QUIET_TPB) k_quiet_final(int nb, const uint32_t* part, int every, QuietState* st) {
    __shared__ uint32_t s_part[QUIET_MAX_PARTS];
    for (int b = (int)threadIdx.x; b < nb; b += QUIET_TPB) s_part[b] = part[b];
    __syncthreads();
    if (threadIdx.x != 0) return;
    long long active = 0;
    for (int b = 0; b < nb; ++b) active += (long long)s_part[b];
    const long long c = st->next_cycle;
    st->next_cycle = (every == 1 || c % every == 0) ? c + 1 : c + every - 1;
    st->checks += 1;
    st->active = active;
    st->last_check = c;
    if (active == 0) {
        if (st->last_all4 == c - 1 && st->quiescent_at < 0) st->quiescent_at = c;
        st->last_all4 = c;
    }
}

// One thread, in stream order.  The state or the cost function has changed (or watching starts): the fixed point no
// longer holds, and the checks carry on from the first checked cycle after `cycle`.  fresh: the counters start again too.
static __global__ void k_quiet_restart(QuietState* st, long long cycle, int every, int fresh) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    long long c = cycle + 1;
    if (every > 1 && c % every > 1) c += every - c % every;
    st->next_cycle = c;
    st->last_all4 = QUIET_NONE;
    st->quiescent_at = -1;
    if (fresh) {
        st->checks = 0;
        st->active = 0;
        st->last_check = -1;
    }
}

}  // namespace mxs
