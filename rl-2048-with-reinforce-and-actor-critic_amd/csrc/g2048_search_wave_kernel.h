// g2048_search_wave_kernel.h -- search_wave_kernel and search_wave_choose_kernel, their argument checks and their
// launches, shared by g2048_search_wave.hip (the 4 x 4 game) and g2048_sized_search_wave.hip (sizes 2..8).  The
// per-step code is search::wave_partial / wave_finish of g2048_search_wave_core.h, the code the CPU tests run.
//
// Shape: search_kernel's contract (g2048_search_kernel.h: the same SearchArgs, queue, order, resume, suspension at
// `cap`, rows, per-episode outputs and suspend buffers; the policy stream is never touched) with one episode per WAVE
// instead of one per lane.  Workgroups are kScriptBlock = 256 threads = 4 waves = 4 episodes; the waves never talk to
// each other: no LDS, no barrier.  The episode's state is wave-uniform and every lane holds it.  Lane 0 claims the next
// entry of `order` with one atomicAdd and the index is broadcast; per step the lanes share the board's work items
// (wave_partial), the four int64 totals are summed over the wave with a butterfly of __shfl_xor on their halves,
// every lane finishes the choice (wave_finish) and plays G::step itself -- the same PCG64 draw and the same fp64 reward
// bits in all 64 -- and lane 0 alone stores the row, the end-of-episode outputs or the suspension.  All control flow
// outside wave_partial is wave-uniform (the claimed index and the end-of-episode flag go through readfirstlane, so the
// compiler sees it too).
// Termination: a wave that holds an episode advances it by one step per iteration (wave_partial is a bounded loop
// nest) and gives it up by termination, truncation or suspension at `cap`; the only exit is "this wave holds no
// episode and the queue is drained" (claims only grow).  Nothing spins and no wave waits on another.
// Roofline: integer VALU only, two stores per step by one lane and no loads: as search_kernel, far from HBM.  A step's
// chain of dependent work shrinks from the board's items (up to 8 (N^2 - 1)) to ceil(items / 64) of them plus the
// four top moves every lane repeats and 48 cross-lane moves, so a launch of few episodes gains up to min(items, 64);
// a launch that already fills the device one episode per lane has nothing to gain and pays for the repeated parts and
// for the lanes without an item.
#pragma once
#include "g2048_search_kernel.h"
#include "g2048_search_wave_core.h"

namespace {

constexpr int kWavesPerBlock = kScriptBlock / (int)search::kWaveLanes;

// the sum of v over the 64 lanes, in every lane
__device__ __forceinline__ int64_t wave_sum(int64_t v) {
    uint32_t lo = (uint32_t)(uint64_t)v, hi = (uint32_t)((uint64_t)v >> 32);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t olo = (uint32_t)__shfl_xor((int)lo, d, 64), ohi = (uint32_t)__shfl_xor((int)hi, d, 64);
        const uint64_t s = (((uint64_t)hi << 32) | lo) + (((uint64_t)ohi << 32) | olo);
        lo = (uint32_t)s;
        hi = (uint32_t)(s >> 32);
    }
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// choose<G, D> by the whole wave: every lane returns the action and holds q
template <class G, int D>
__device__ __forceinline__ uint32_t wave_choose(const uint64_t (&b)[G::kWords], const search::Weights& w, uint32_t lane,
                                                int64_t (&q)[4]) {
    int64_t tot[4];
    search::wave_partial<G, D>(b, w, lane, tot);
#pragma unroll
    for (int k = 0; k < 4; k++) tot[k] = wave_sum(tot[k]);
    return search::wave_finish<G>(b, w, tot, q);
}

template <class G, int D, bool TRAJ>
__global__ void __launch_bounds__(kScriptBlock) search_wave_kernel(SearchArgs a) {
    constexpr int W = G::kWords;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t ep = kNoEpisode;                          // wave-uniform, like everything below but `lane`
    scripted::Episode<G> e{};
    bool drained = false;
    while (true) {
        if (ep == kNoEpisode && !drained) {
            const ScriptArgs& q = args_per_lane();
            uint32_t idx = 0;
            if (lane == 0u) idx = atomicAdd(q.next, 1u);
            idx = (uint32_t)__builtin_amdgcn_readfirstlane((int)idx);
            if (idx < a.s.n_order) {
                ep = q.order ? (uint32_t)q.order[idx] : idx;
                ep = (uint32_t)__builtin_amdgcn_readfirstlane((int)ep);
                e.ge = load_stream(q.env_rs, q.env_inc, q.env_buf, ep);
                if (a.s.resume) {
#pragma unroll
                    for (int w = 0; w < W; w++) e.bw[w] = q.sus.board[(size_t)w * q.n + ep];
                    e.t = q.sus.meta[3 * (size_t)ep];
                    e.sc = q.sus.meta[3 * (size_t)ep + 1];
                    e.mt = q.sus.meta[3 * (size_t)ep + 2];
                    e.total = q.sus.total[ep];
                } else {
                    scripted::episode_reset<G>(e);
                }
            } else {
                drained = true;
            }
        }
        if (ep == kNoEpisode) break;                   // the loop's only exit: no episode and a drained queue
        int64_t qv[4];
        scripted::Row<G> row;
        const uint32_t t0 = e.t;
        row.action = wave_choose<G, D>(e.bw, a.w, lane, qv);
#pragma unroll
        for (int w = 0; w < W; w++) row.bw[w] = e.bw[w];
        G::step(e.bw, row.action, e.sc, e.mt, e.ge, a.s.rc, a.s.max_steps, row.reward, row.flags);
        e.sc += 1u;
        e.t += 1u;
        e.total += row.reward;
        const bool ended =
            __builtin_amdgcn_readfirstlane((int)(row.flags & (kFTerminated | kFTruncated))) != 0;
        const ScriptArgs& q = args_per_lane();
        const bool suspend = __builtin_amdgcn_readfirstlane((int)(!ended && e.t >= a.s.cap)) != 0;
        if (lane == 0u) {
            if constexpr (TRAJ) {
                const size_t r = (size_t)t0 * q.n + ep;
#pragma unroll
                for (int w = 0; w < W; w++) q.tr.boards[(size_t)w * (size_t)q.bstride + r] = row.bw[w];
                q.tr.actions[r] = (uint8_t)row.action;
                q.tr.rewards[r] = row.reward;
                q.tr.flags[r] = (uint8_t)row.flags;
            }
            if (ended) {
                q.tr.lengths[ep] = (int32_t)e.t;
                q.tr.totals[ep] = e.total;
                q.tr.max_tile[ep] = (uint8_t)e.mt;
#pragma unroll
                for (int w = 0; w < W; w++) q.tr.final_board[(size_t)w * q.n + ep] = e.bw[w];
            } else if (suspend) {                      // out of rows / at the step limit: for the host to resume
                store_stream(q.env_rs, q.env_buf, ep, e.ge);
#pragma unroll
                for (int w = 0; w < W; w++) q.sus.board[(size_t)w * q.n + ep] = e.bw[w];
                q.sus.meta[3 * (size_t)ep] = e.t;
                q.sus.meta[3 * (size_t)ep + 1] = e.sc;
                q.sus.meta[3 * (size_t)ep + 2] = e.mt;
                q.sus.total[ep] = e.total;
                q.sus.list[atomicAdd(q.sus.count, 1u)] = (int32_t)ep;
            }
        }
        if (ended || suspend) ep = kNoEpisode;
    }
}

// One board per wave, a grid-stride loop over the boards: boards are [W, n] planes of stride n; q may be NULL.
template <class G, int D>
__global__ void __launch_bounds__(kScriptBlock) search_wave_choose_kernel(search::Weights w, const uint64_t* boards,
                                                                          uint32_t n, uint8_t* actions, int64_t* q) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = blockIdx.x * (uint32_t)kWavesPerBlock + (threadIdx.x >> 6);
    const uint32_t waves = gridDim.x * (uint32_t)kWavesPerBlock;
    for (uint32_t i = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave); i < n; i += waves) {
        uint64_t b[G::kWords];
#pragma unroll
        for (int k = 0; k < G::kWords; k++) b[k] = boards[(size_t)k * n + i];
        int64_t qv[4];
        const uint32_t act = wave_choose<G, D>(b, w, lane, qv);
        if (lane == 0u) {
            actions[i] = (uint8_t)act;
            if (q) {
#pragma unroll
                for (int k = 0; k < 4; k++) q[4 * (size_t)i + k] = qv[k];
            }
        }
    }
}

// there is nothing to spread at depth 0: after the siblings' checks, before any HIP call
int wave_depth(const char* who, const g2048_search* sp) {
    if (sp->depth < 1)
        return sfail(G2048_EINVAL, std::string(who) + ": depth must be 1 or 2 (depth 0 has no chance level to spread "
                                                      "over a wave: use the one-episode-per-lane call)");
    return G2048_OK;
}

// one workgroup per kWavesPerBlock units (episodes or boards), at most 8 per CU, at most max_workgroups when > 0
int wave_grid(int64_t units, int max_workgroups) {
    int64_t grid = (units + kWavesPerBlock - 1) / kWavesPerBlock;
    const int64_t per_dev = 8 * (int64_t)device_cus();
    if (grid > per_dev) grid = per_dev;
    if (max_workgroups > 0 && grid > max_workgroups) grid = max_workgroups;
    return (int)grid;
}

template <class G, bool TRAJ>
int launch_search_wave(int depth, const SearchArgs& a, int max_workgroups, void* stream) {
    const dim3 grid(wave_grid(a.s.n_order, max_workgroups)), block(kScriptBlock);
    if (depth == 1)
        hipLaunchKernelGGL((search_wave_kernel<G, 1, TRAJ>), grid, block, 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL((search_wave_kernel<G, 2, TRAJ>), grid, block, 0, (hipStream_t)stream, a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? G2048_OK : sfail(G2048_EHIP, hipGetErrorString(e));
}

template <class G>
int launch_wave_choose(int depth, const search::Weights& w, const uint64_t* boards, int64_t n, uint8_t* actions,
                       int64_t* q, void* stream) {
    const dim3 grid(wave_grid(n, 0)), block(kScriptBlock);
    if (depth == 1)
        hipLaunchKernelGGL((search_wave_choose_kernel<G, 1>), grid, block, 0, (hipStream_t)stream, w, boards,
                           (uint32_t)n, actions, q);
    else
        hipLaunchKernelGGL((search_wave_choose_kernel<G, 2>), grid, block, 0, (hipStream_t)stream, w, boards,
                           (uint32_t)n, actions, q);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? G2048_OK : sfail(G2048_EHIP, hipGetErrorString(e));
}

}  // namespace
