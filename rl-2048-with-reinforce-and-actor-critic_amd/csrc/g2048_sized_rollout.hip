// g2048_sized_rollout.hip -- g2048_deep_rollout for N x N boards, 2 <= N <= 8 (include/g2048_sized.h): the whole
// batched rollout (ReinforceAgent.run_episode, src/reinforce_agent.py:195-252, for n (env_seed, policy_seed) pairs) in
// persistent launches, for a net packed by g2048_sized_pack (part of libg2048.so).
//
// The kernel is the NB = 32 form of deep_rollout_kernel (g2048_deep.hip): 256 threads (4 waves), two workgroups per
// CU, 32 episode slots owned by lanes 0..31 of wave 0.  Every iteration the owners put their boards' words into
// SizedSmem::board[word][slot] (zeros for an empty slot), the workgroup runs sized_forward (g2048_sized_fwd.h, the
// code of g2048_sized_policy), and the owners then add the logits (deep_logits), take the action mask, draw on the
// slot's policy stream, choose (softmax_select), step the env in registers (sized::env_step, plain-ALU line moves: no
// row table, so g2048_init is not needed), write the trajectory row and finish, suspend or keep the episode.  A free
// slot takes the next episode from the queue (one atomicAdd per ballot of wave 0).  An episode that reaches row `cap`
// without ending is SUSPENDED -- board, counters, running total and both streams written back per episode, the
// episode listed -- and the host grows the trajectory buffer and resumes the listed episodes (resume = 1).
// Termination: the loop's only exit is the block-uniform "no live slot" test after a barrier; every live slot
// advances one row per iteration and ends by termination, truncation or suspension at `cap`; nothing spins and no
// workgroup waits on another.
// Instantiation: {raw, log2, one-hot} x {ReLU, Sigmoid} x N in 2..8 = 42 kernels.  The forward takes the cell and
// word counts as runtime values, exactly as in g2048_sized_policy; N is a template parameter for the owners' tail
// only (fresh board, mask, env step).  The 6-kernel form -- a kernel-uniform switch (size) around template <int N>
// tail functions, as sized_mask_word has -- was built first and spilled 18..22 scalar registers in every kernel: the
// seven tails' literal masks (about 50 scalar registers of them) are hoisted out of the persistent loop together,
// and the 64-bit ones are not rematerialised.  With one tail per kernel nothing spills, and the whole unit still
// compiles faster than g2048_deep.hip, itself well below g2048_policy.hip, the unit that build() from an empty cache
// waits for.
// Every kernel-uniform flag the owners test is held per lane (per_lane) so that it does not live as a scalar lane
// mask across the forward.
// Roofline: the forward is g2048_sized_policy's (dense layers fp32-MFMA bound); the owners' tail is serial ALU on 32
// lanes of one wave (N line moves of N - 1 steps each) and is what a step costs beyond the forward at N = 8.
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

int rfail(int code, const std::string& msg) { return g2048_internal::set_error(code, msg.c_str()); }

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
    g2048_traj tr;
    int64_t bstride;   // plane stride of tr.boards (>= cap * n); final_board / sus.board planes have stride n
    uint32_t n, cap;
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

template <int OBS, int ACT, int N>
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
            const size_t row = (size_t)t * q.n + ep;
#pragma unroll
            for (int w = 0; w < 4; w++)
                if (w < words) q.tr.boards[(size_t)w * (size_t)q.bstride + row] = pb[w];
            q.tr.actions[row] = (uint8_t)act;
            q.tr.rewards[row] = reward;
            q.tr.flags[row] = (uint8_t)fl;
            if (q.tr.probs) reinterpret_cast<float4*>(q.tr.probs)[row] = make_float4(p[0], p[1], p[2], p[3]);
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

template <int OBS, int ACT>
void launch_roll_size(const SizedRollArgs& a, int grid, hipStream_t s) {
#define G2048_ROLL(NN) hipLaunchKernelGGL((sized_rollout_kernel<OBS, ACT, NN>), dim3(grid), dim3(kDeepBlock), 0, s, a)
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

template <int OBS>
void launch_roll_act(const SizedRollArgs& a, int act, int grid, hipStream_t s) {
    if (act == G2048_ACT_RELU) launch_roll_size<OBS, 0>(a, grid, s);
    else launch_roll_size<OBS, 1>(a, grid, s);
}

}  // namespace

extern "C" {

int g2048_sized_rollout(int size, const float* packed, int n_hidden, const int32_t* hidden, int activation,
                        const g2048_env_cfg* cfg, int greedy, uint64_t* env_state, const uint64_t* env_inc,
                        uint64_t* env_buf, uint64_t* pol_state, const uint64_t* pol_inc, uint64_t* pol_buf,
                        uint32_t* queue, const int32_t* order, int64_t n_order, int resume, const g2048_suspend* sus,
                        int64_t n, int64_t cap, const g2048_traj* traj, int64_t board_stride, int max_workgroups,
                        void* stream) {
    // every check precedes every HIP call
    if (size < 2 || size > 8) return rfail(G2048_EINVAL, "size must be in 2..8 (got " + std::to_string(size) + ")");
    int rc = g2048_internal::check_env_cfg(cfg);
    if (rc) return rc;
    if (n < 0 || n > (int64_t)0x7FFFFFFF) return rfail(G2048_EINVAL, "n out of range");
    if (n_order < 0 || n_order > n || (!order && n_order != n) || (resume && !order))
        return rfail(G2048_EINVAL,
                     "sized rollout: order must list n_order <= n episodes (all n when NULL; resume needs a list)");
    if (cap < 1 || cap > (int64_t)0x7FFFFFFF || n * cap > ((int64_t)1 << 40))
        return rfail(G2048_EINVAL, "sized rollout: bad cap");
    if (board_stride < cap * n)
        return rfail(G2048_EINVAL, "sized rollout: board_stride " + std::to_string(board_stride) + " < cap * n = " +
                                       std::to_string(cap * n));
    if (max_workgroups < 0) return rfail(G2048_EINVAL, "sized rollout: max_workgroups < 0");
    DeepNet net;
    if (!obs_ok(cfg->obs_mode) || !sized_layout(size, n_hidden, hidden, cfg->obs_mode == G2048_OBS_ONEHOT, net))
        return rfail(G2048_EINVAL, "sized policy: obs raw / log2 / onehot, 1..4 hidden layers of 1..256 units");
    if (activation != G2048_ACT_RELU && activation != G2048_ACT_SIGMOID)
        return rfail(G2048_EINVAL, "Unsupported activation");
    if (!packed || !env_state || !env_inc || !env_buf || !pol_state || !pol_inc || !pol_buf || !queue || !sus || !traj ||
        !sus->board || !sus->meta || !sus->total || !sus->list || !sus->count || !traj->boards || !traj->actions ||
        !traj->rewards || !traj->flags || !traj->lengths || !traj->totals || !traj->max_tile || !traj->final_board)
        return rfail(G2048_EINVAL, "sized rollout: a required buffer is NULL");
    if (n_order == 0) return G2048_OK;
    SizedRollArgs a;
    a.net = net;
    a.packed = packed;
    a.rc = g2048_internal::reward_cfg_of(*cfg);
    a.max_steps = cfg->max_steps;
    a.obs_scale = cfg->obs_log2_scale;
    a.size = size;
    a.use_mask = cfg->use_action_mask;
    a.greedy = greedy;
    a.env_rs = env_state;
    a.env_inc = env_inc;
    a.env_buf = env_buf;
    a.pol_rs = pol_state;
    a.pol_inc = pol_inc;
    a.pol_buf = pol_buf;
    a.next = queue;
    a.order = order;
    a.n_order = (uint32_t)n_order;
    a.resume = resume;
    a.sus = *sus;
    a.tr = *traj;
    a.bstride = board_stride;
    a.n = (uint32_t)n;
    a.cap = (uint32_t)cap;
    int64_t grid = (n_order + 31) / 32;                 // persistent; the slots refill from the queue
    const int64_t per_dev = 2 * (int64_t)device_cus();   // two workgroups per CU
    if (grid > per_dev) grid = per_dev;
    if (max_workgroups > 0 && grid > max_workgroups) grid = max_workgroups;
    hipStream_t s = (hipStream_t)stream;
    const int obs = cfg->obs_mode;
    if (obs == G2048_OBS_ONEHOT) launch_roll_act<G2048_OBS_ONEHOT>(a, activation, (int)grid, s);
    else if (obs == G2048_OBS_LOG2) launch_roll_act<G2048_OBS_LOG2>(a, activation, (int)grid, s);
    else launch_roll_act<G2048_OBS_RAW>(a, activation, (int)grid, s);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? G2048_OK : rfail(G2048_EHIP, hipGetErrorString(e));
}

}  // extern "C"
