// g2048_sized_rollout_kernel.h -- sized_rollout_kernel and its launch helpers, shared by the two translation units
// that instantiate it: g2048_sized_rollout.hip (TRAJ = true: the trajectory form, 42 kernels) and g2048_sized_eval.hip
// (TRAJ = false: the score-only form, 42 more), so that the two sets compile side by side.  What the kernel does, how
// it ends and why it is instantiated per size is described at the top of g2048_sized_rollout.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "g2048.h"
#include "g2048_sized_core.h"
#include "g2048_deep_fwd.h"
#include "g2048_sized_fwd.h"

using namespace g2048;

namespace g2048_internal {   // g2048.hip
int set_error(int code, const char* msg);
int check_env_cfg(const g2048_env_cfg* c);
g2048::RewardCfg reward_cfg_of(const g2048_env_cfg& c);
}  // namespace g2048_internal

namespace {

struct SizedRollArgs {
    DeepNet net;
    const float* packed;
    RewardCfg rc;
    int64_t max_steps;
    float obs_scale;
    int size;
    int use_mask, greedy;
    uint64_t* env_rs;
    const uint64_t* env_inc;
    uint64_t* env_buf;
    uint64_t* pol_rs;
    const uint64_t* pol_inc;
    uint64_t* pol_buf;
    uint32_t* next;
    const int32_t* order;
    uint32_t n_order;
    int resume;
    g2048_suspend sus;
    g2048_traj tr;     // score-only form: lengths, totals, max_tile and final_board only (the row pointers stay NULL)
    int64_t bstride;   // plane stride of tr.boards (>= cap * n); final_board / sus.board planes have stride n
    uint32_t n, cap;   // cap: trajectory rows; score-only form: the step count at which a running episode is suspended
};

// load_stream / store_stream of g2048_deep.hip
__device__ __forceinline__ Pcg64 load_stream(const uint64_t* rs, const uint64_t* inc, const uint64_t* buf, uint32_t e) {
    Pcg64 g;
    const ulonglong2 s = reinterpret_cast<const ulonglong2*>(rs)[e];
    const ulonglong2 c = reinterpret_cast<const ulonglong2*>(inc)[e];
    const uint64_t bf = buf[e];
    g.s_lo = s.x;
    g.s_hi = s.y;
    g.i_lo = c.x;
    g.i_hi = c.y;
    g.has_uint32 = (uint32_t)(bf >> 32);
    g.uinteger = (uint32_t)bf;
    return g;
}

__device__ __forceinline__ void store_stream(uint64_t* rs, uint64_t* buf, uint32_t e, const Pcg64& g) {
    reinterpret_cast<ulonglong2*>(rs)[e] = make_ulonglong2(g.s_lo, g.s_hi);
    buf[e] = ((uint64_t)g.has_uint32 << 32) | g.uinteger;
}

// The kernel's argument struct where the dispatch put it (the kernarg segment: the struct is the kernel's only
// parameter, at offset 0).  Read as `a.x`, every argument is a scalar load hoisted to the kernel's start and held in
// scalar registers for the whole loop, and the owners' tail, which nests its own lane masks, then spills scalar
// registers (66..70 of them).  So the owners read the arguments of their tail through a per-lane pointer (vector loads
// where the value is used), and the forward reads the net through a pointer that is opaque once per iteration (its
// scalar loads stay inside the iteration and their registers are free again in the tail).
typedef const __attribute__((address_space(4))) SizedRollArgs* KernArgs;
__device__ __forceinline__ const SizedRollArgs& args_per_lane() {
    KernArgs p = (KernArgs)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+v"(p));
    return *(const SizedRollArgs*)p;
}
__device__ __forceinline__ const SizedRollArgs& args_reloaded() {
    KernArgs p = (KernArgs)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *(const SizedRollArgs*)p;
}

constexpr uint32_t kNoEpisode = 0xFFFFFFFFu;

// Game2048.reset (src/game2048.py:26-34) on the episode's env stream: two spawns on an empty board
template <int N>
__device__ __forceinline__ void fresh_words(uint64_t (&bw)[4], Pcg64& g) {
    sz::Board<N> b;
#pragma unroll
    for (int w = 0; w < sz::Dim<N>::kWords; w++) b.w[w] = 0ull;
    sz::spawn_pcg<N>(b, g);
    sz::spawn_pcg<N>(b, g);
#pragma unroll
    for (int w = 0; w < 4; w++) bw[w] = w < sz::Dim<N>::kWords ? b.w[w < sz::Dim<N>::kWords ? w : 0] : 0ull;
}

// one Game2048Env.step of the board held in bw (sized::env_step on the PCG64 stream, no merged list)
template <int N>
__device__ __forceinline__ void step_words(uint64_t (&bw)[4], uint32_t act, uint32_t sc, uint32_t& mt, Pcg64& g,
                                           const RewardCfg& rc, int64_t max_steps, double& reward, uint32_t& flags) {
    sz::Board<N> b;
#pragma unroll
    for (int w = 0; w < sz::Dim<N>::kWords; w++) b.w[w] = bw[w];
    const sz::StepValues<N> o = sz::env_step<N, G2048_RNG_PCG64, false>(b, act, sc, mt, g, 0ull, 0ull, rc, max_steps, nullptr);
#pragma unroll
    for (int w = 0; w < sz::Dim<N>::kWords; w++) bw[w] = o.board.w[w];
    reward = o.reward;
    flags = o.flags;
}

// TRAJ = false is the score-only form: the same code without the trajectory row (its stores and the row index); the
// episode's end and the suspension at `cap` steps are unchanged.
template <int OBS, int ACT, int N, bool TRAJ>
__global__ void __launch_bounds__(kDeepBlock, 2) sized_rollout_kernel(SizedRollArgs a) {
    __shared__ SizedSmem S;
    __shared__ int go;
    const int tid = threadIdx.x;
    const int cells = a.size * a.size, words = (cells + 15) >> 4;
    const bool owner = tid < 32;
    uint32_t ep = kNoEpisode, t = 0, sc = 0, mt = 2;
    uint64_t bw[4] = {0ull, 0ull, 0ull, 0ull};         // the slot's board; words >= W stay 0
    double total = 0.0;
    Pcg64 ge{}, gp{};
    bool drained = false;                              // wave-0-uniform: the queue is empty (claims only grow)
    const auto start = [&](const SizedRollArgs& q, uint32_t e) {
        ep = e;
        ge = load_stream(q.env_rs, q.env_inc, q.env_buf, e);
        gp = load_stream(q.pol_rs, q.pol_inc, q.pol_buf, e);
        if (per_lane(q.resume)) {
#pragma unroll
            for (int w = 0; w < 4; w++) bw[w] = w < words ? q.sus.board[(size_t)w * q.n + e] : 0ull;
            t = q.sus.meta[3 * (size_t)e];
            sc = q.sus.meta[3 * (size_t)e + 1];
            mt = q.sus.meta[3 * (size_t)e + 2];
            total = q.sus.total[e];
        } else {
            fresh_words<N>(bw, ge);
            t = 0;
            sc = 0;
            mt = 2;                                   // max_tile_seen = 4 (src/env.py:188)
            total = 0.0;
        }
    };
    const auto claim = [&](const SizedRollArgs& q) {                         // wave 0 only
        if (drained) return;
        const bool need = owner && ep == kNoEpisode;
        const uint64_t bal = __ballot(need);
        if (!bal) return;
        const int leader = __builtin_ctzll(bal);
        uint32_t base = 0;
        if ((int)(threadIdx.x & 63) == leader) base = atomicAdd(q.next, (uint32_t)__popcll(bal));
        base = (uint32_t)__shfl((int)base, leader, 64);
        const uint32_t idx =
            base + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
        if (need && idx < q.n_order) start(q, q.order ? (uint32_t)q.order[idx] : idx);
        drained = __ballot(need && idx >= q.n_order) != 0ull;
    };
    if (tid < 64) claim(args_per_lane());
    while (true) {
        if (tid < 64) {
            const uint64_t live = __ballot(owner && ep != kNoEpisode);
            if (tid == 0) go = live != 0ull;
            if (owner) {
#pragma unroll
                for (int w = 0; w < 4; w++)
                    if (w < words) S.board[w][tid] = ep != kNoEpisode ? bw[w] : 0ull;
            }
        }
        __syncthreads();
        if (!go) break;                                // block-uniform: the loop's only exit
        {
            const SizedRollArgs& f = args_reloaded();
            sized_forward<OBS, ACT>(f.net, f.packed, S, cells, words, f.obs_scale);
        }
        if (owner && ep != kNoEpisode) {
            const SizedRollArgs& q = args_per_lane();
            float lg[4];
            deep_logits(q.net, q.packed, S, tid, lg);
            const int use_mask = per_lane(q.use_mask), greedy = per_lane(q.greedy);
            const uint32_t mb = mask_bits_of<N>(bw);   // sized_mask_word of the kernel's own size
            const uint32_t mw = use_mask ? (mb & 1u) | ((mb & 2u) << 7) | ((mb & 4u) << 14) | ((mb & 8u) << 21) : 0x01010101u;
            const double u = greedy ? 0.0 : pcg_random(gp);
            float p[4];
            const uint32_t act = softmax_select(lg, mw, use_mask != 0, greedy != 0, u, p);
            uint64_t pb[4];                            // the board before the step: the row's state
#pragma unroll
            for (int w = 0; w < 4; w++) pb[w] = bw[w];
            sc += 1;                                   // the step count after this step
            double reward;
            uint32_t fl;
            step_words<N>(bw, act, sc, mt, ge, q.rc, q.max_steps, reward, fl);
            if constexpr (TRAJ) {
                const size_t row = (size_t)t * q.n + ep;
#pragma unroll
                for (int w = 0; w < 4; w++)
                    if (w < words) q.tr.boards[(size_t)w * (size_t)q.bstride + row] = pb[w];
                q.tr.actions[row] = (uint8_t)act;
                q.tr.rewards[row] = reward;
                q.tr.flags[row] = (uint8_t)fl;
                if (q.tr.probs) reinterpret_cast<float4*>(q.tr.probs)[row] = make_float4(p[0], p[1], p[2], p[3]);
            }
            total += reward;                           // total_reward += float(reward) (src/reinforce_agent.py:233)
            t += 1;
            if ((fl & (kFTerminated | kFTruncated)) != 0u) {
                q.tr.lengths[ep] = (int32_t)t;
                q.tr.totals[ep] = total;
                q.tr.max_tile[ep] = (uint8_t)mt;
#pragma unroll
                for (int w = 0; w < 4; w++)
                    if (w < words) q.tr.final_board[(size_t)w * q.n + ep] = bw[w];
                ep = kNoEpisode;
            } else if (t >= q.cap) {                   // out of trajectory rows: suspend for the host to resume
                store_stream(q.env_rs, q.env_buf, ep, ge);
                store_stream(q.pol_rs, q.pol_buf, ep, gp);
#pragma unroll
                for (int w = 0; w < 4; w++)
                    if (w < words) q.sus.board[(size_t)w * q.n + ep] = bw[w];
                q.sus.meta[3 * (size_t)ep] = t;
                q.sus.meta[3 * (size_t)ep + 1] = sc;
                q.sus.meta[3 * (size_t)ep + 2] = mt;
                q.sus.total[ep] = total;
                q.sus.list[atomicAdd(q.sus.count, 1u)] = (int32_t)ep;
                ep = kNoEpisode;
            }
        }
        // S.board is rewritten by threads 0..31 only, after they finished with S.part; every other LDS buffer is
        // rewritten only after the next iteration's first barrier
        if (tid < 64) claim(args_per_lane());
    }
}

int device_cus() {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) {
        int c = 0;
        if (hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && c > 0) cus = c;
    }
    return cus;
}

template <int OBS, int ACT, bool TRAJ>
void launch_roll_size(const SizedRollArgs& a, int grid, hipStream_t s) {
#define G2048_ROLL(NN) \
    hipLaunchKernelGGL((sized_rollout_kernel<OBS, ACT, NN, TRAJ>), dim3(grid), dim3(kDeepBlock), 0, s, a)
    switch (a.size) {
        case 2: G2048_ROLL(2); break;
        case 3: G2048_ROLL(3); break;
        case 4: G2048_ROLL(4); break;
        case 5: G2048_ROLL(5); break;
        case 6: G2048_ROLL(6); break;
        case 7: G2048_ROLL(7); break;
        default: G2048_ROLL(8); break;
    }
#undef G2048_ROLL
}

template <int OBS, bool TRAJ>
void launch_roll_act(const SizedRollArgs& a, int act, int grid, hipStream_t s) {
    if (act == G2048_ACT_RELU) launch_roll_size<OBS, 0, TRAJ>(a, grid, s);
    else launch_roll_size<OBS, 1, TRAJ>(a, grid, s);
}

// the grid of both forms (persistent; the slots refill from the queue) and the launch by obs mode
template <bool TRAJ>
void launch_sized_roll(const SizedRollArgs& a, int obs, int activation, int64_t n_order, int max_workgroups,
                       hipStream_t s) {
    int64_t grid = (n_order + 31) / 32;
    const int64_t per_dev = 2 * (int64_t)device_cus();   // two workgroups per CU
    if (grid > per_dev) grid = per_dev;
    if (max_workgroups > 0 && grid > max_workgroups) grid = max_workgroups;
    if (obs == G2048_OBS_ONEHOT) launch_roll_act<G2048_OBS_ONEHOT, TRAJ>(a, activation, (int)grid, s);
    else if (obs == G2048_OBS_LOG2) launch_roll_act<G2048_OBS_LOG2, TRAJ>(a, activation, (int)grid, s);
    else launch_roll_act<G2048_OBS_RAW, TRAJ>(a, activation, (int)grid, s);
}

}  // namespace
