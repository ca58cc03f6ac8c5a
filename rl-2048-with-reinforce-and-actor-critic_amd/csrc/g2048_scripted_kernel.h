// g2048_scripted_kernel.h -- scripted_kernel, its argument checks and its launch, shared by the two translation units
// that instantiate it: g2048_scripted.hip (the 4 x 4 game, g2048_core.h) and g2048_sized_scripted.hip (sizes 2..8,
// g2048_sized_core.h).  The per-step code is episode_step of g2048_scripted_core.h, the code the CPU tests run.
//
// Shape: one episode per lane, persistent.  A workgroup is kScriptBlock = 256 threads = 4 waves that never talk to
// each other: no LDS, no barrier.  Each wave loops: lanes without an episode claim the next entries of `order` from
// the queue (one atomicAdd per ballot), the wave leaves when none of its lanes holds an episode (claims only grow, so
// a drained queue stays drained), and every lane that holds one plays one step -- mask, choice, env step in registers,
// the trajectory row (TRAJ), then end / suspend / keep.  Lanes of a wave sit at different steps of different episodes,
// so a row is four (W + 3) scattered stores per lane; everything else lives in registers.
// Termination: every live lane advances its episode by one step per iteration and gives it up by termination,
// truncation or suspension at `cap`; nothing spins and no wave waits on another.
// Roofline: no net, so neither MFMA nor LDS; the loop is integer / fp64 VALU latency (two 128-bit PCG64 multiplies and
// an fp64 reward per step), far from both the HBM and the VALU peak with one wave per SIMD -- the launch fills the
// device only from about 64 episodes per SIMD up.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "g2048.h"
#include "g2048_scripted_core.h"

using namespace g2048;

namespace g2048_internal {   // g2048.hip
int set_error(int code, const char* msg);
int check_env_cfg(const g2048_env_cfg* c);
g2048::RewardCfg reward_cfg_of(const g2048_env_cfg& c);
}  // namespace g2048_internal

namespace {

constexpr int kScriptBlock = G2048_SCRIPT_BLOCK;
static_assert(scripted::kPriority == G2048_SCRIPT_PRIORITY && scripted::kUniform == G2048_SCRIPT_UNIFORM, "script kinds");

struct ScriptArgs {
    scripted::Script script;
    RewardCfg rc;
    int64_t max_steps;
    int use_mask;
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

constexpr uint32_t kNoEpisode = 0xFFFFFFFFu;

// The kernel's argument struct where the dispatch put it (the kernarg segment: the struct is the kernel's only
// parameter, at offset 0), through a per-lane pointer, as in g2048_sized_rollout_kernel.h: read as `a.x`, every buffer
// pointer is a scalar load hoisted to the kernel's start and held across the loop, and the step's own scalars (the
// reward config, literal masks, nested lane masks) then spill.  The claim and the stores read their pointers through
// this (vector loads where the value is used); the step reads the script and the reward config from `a`.
typedef const __attribute__((address_space(4))) ScriptArgs* KernArgs;
__device__ __forceinline__ const ScriptArgs& args_per_lane() {
    KernArgs p = (KernArgs)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+v"(p));
    return *(const ScriptArgs*)p;
}

// The player of scripted_kernel: the script of the launch.  A player of play_episodes says whether it draws from the
// episode's policy stream (kernel-uniform: loaded at the claim and stored at a suspension only then) and plays one
// step of an episode (episode_step's contract).
template <class G>
struct ScriptPlayer {
    const ScriptArgs& a;
    __device__ __forceinline__ bool policy_stream() const { return a.script.kind == scripted::kUniform; }
    __device__ __forceinline__ bool step(scripted::Episode<G>& e, scripted::Row<G>& row) const {
        return scripted::episode_step<G>(e, a.script, a.rc, a.max_steps, a.use_mask != 0, row);
    }
};

// The persistent loop of every one-episode-per-lane kernel (scripted_kernel here, search_kernel of
// g2048_search_kernel.h): claim / refill, resume, one step of the player, the row, end / suspend / keep.
// G: scripted::Game4 or scripted::GameN<N>.  TRAJ = false is the score-only form: the same code without the
// trajectory row; the episode's end and the suspension at `cap` steps are unchanged.  The kernel's ScriptArgs are at
// offset 0 of its kernarg segment (args_per_lane).
template <class G, bool TRAJ, class Player>
__device__ __forceinline__ void play_episodes(const Player& player) {
    constexpr int W = G::kWords;
    const int lane = (int)(threadIdx.x & 63);
    const bool uniform = player.policy_stream();
    uint32_t ep = kNoEpisode;
    scripted::Episode<G> e{};
    bool drained = false;                              // wave-uniform: the queue is empty (claims only grow)
    while (true) {
        if (!drained) {
            const ScriptArgs& q = args_per_lane();
            const bool need = ep == kNoEpisode;
            const uint64_t bal = __ballot(need);
            if (bal) {
                const int leader = __builtin_ctzll(bal);
                uint32_t base = 0;
                if (lane == leader) base = atomicAdd(q.next, (uint32_t)__popcll(bal));
                base = (uint32_t)__shfl((int)base, leader, 64);
                const uint32_t idx =
                    base + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
                if (need && idx < q.n_order) {
                    ep = q.order ? (uint32_t)q.order[idx] : idx;
                    e.ge = load_stream(q.env_rs, q.env_inc, q.env_buf, ep);
                    if (uniform) e.gp = load_stream(q.pol_rs, q.pol_inc, q.pol_buf, ep);
                    if (q.resume) {
#pragma unroll
                        for (int w = 0; w < W; w++) e.bw[w] = q.sus.board[(size_t)w * q.n + ep];
                        e.t = q.sus.meta[3 * (size_t)ep];
                        e.sc = q.sus.meta[3 * (size_t)ep + 1];
                        e.mt = q.sus.meta[3 * (size_t)ep + 2];
                        e.total = q.sus.total[ep];
                    } else {
                        scripted::episode_reset<G>(e);
                    }
                }
                drained = __ballot(need && idx >= q.n_order) != 0ull;
            }
        }
        if (__ballot(ep != kNoEpisode) == 0ull) break;   // wave-uniform: the loop's only exit
        if (ep != kNoEpisode) {
            scripted::Row<G> row;
            const uint32_t t0 = e.t;
            const bool ended = player.step(e, row);
            const ScriptArgs& q = args_per_lane();
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
                ep = kNoEpisode;
            } else if (e.t >= q.cap) {                 // out of rows / at the step limit: suspend for the host to resume
                store_stream(q.env_rs, q.env_buf, ep, e.ge);
                if (uniform) store_stream(q.pol_rs, q.pol_buf, ep, e.gp);
#pragma unroll
                for (int w = 0; w < W; w++) q.sus.board[(size_t)w * q.n + ep] = e.bw[w];
                q.sus.meta[3 * (size_t)ep] = e.t;
                q.sus.meta[3 * (size_t)ep + 1] = e.sc;
                q.sus.meta[3 * (size_t)ep + 2] = e.mt;
                q.sus.total[ep] = e.total;
                q.sus.list[atomicAdd(q.sus.count, 1u)] = (int32_t)ep;
                ep = kNoEpisode;
            }
        }
    }
}

// The script's kind is kernel-uniform.  Under PRIORITY the policy stream is neither read nor written.
template <class G, bool TRAJ>
__global__ void __launch_bounds__(kScriptBlock) scripted_kernel(ScriptArgs a) {
    play_episodes<G, TRAJ>(ScriptPlayer<G>{a});
}

int sfail(int code, const std::string& msg) { return g2048_internal::set_error(code, msg.c_str()); }

int device_cus() {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) {
        int c = 0;
        if (hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && c > 0) cus = c;
    }
    return cus;
}

// The checks common to the four entry points (every one precedes every HIP call) and the kernel's arguments.  `rows`:
// the trajectory form (cap = row count, traj required, probs must be NULL); otherwise cap = step_limit and the four
// per-episode outputs come from out.  Returns G2048_OK with `a` filled, or the error.
int script_args(const char* who, const g2048_script* script, const g2048_env_cfg* cfg, uint64_t* env_state,
                const uint64_t* env_inc, uint64_t* env_buf, uint64_t* pol_state, const uint64_t* pol_inc,
                uint64_t* pol_buf, uint32_t* queue, const int32_t* order, int64_t n_order, int resume,
                const g2048_suspend* sus, int64_t n, int64_t cap, bool rows, const g2048_traj* traj, int64_t board_stride,
                const g2048_eval_out* out, int max_workgroups, ScriptArgs& a) {
    const std::string w = std::string(who) + ": ";
    if (!script) return sfail(G2048_EINVAL, w + "script is NULL");
    if (script->kind != G2048_SCRIPT_PRIORITY && script->kind != G2048_SCRIPT_UNIFORM)
        return sfail(G2048_EINVAL, w + "script kind must be G2048_SCRIPT_PRIORITY or G2048_SCRIPT_UNIFORM");
    if (script->kind == G2048_SCRIPT_PRIORITY && !scripted::order_ok(script->order))
        return sfail(G2048_EINVAL, w + "order must be a permutation of (0, 1, 2, 3)");
    int rc = g2048_internal::check_env_cfg(cfg);
    if (rc) return rc;
    if (script->kind == G2048_SCRIPT_PRIORITY && !cfg->use_action_mask)
        return sfail(G2048_EINVAL, w + "a priority script needs use_action_mask (its choice is read off the mask)");
    if (n < 0 || n > (int64_t)0x7FFFFFFF) return sfail(G2048_EINVAL, w + "n out of range");
    if (n_order < 0 || n_order > n || (!order && n_order != n) || (resume && !order))
        return sfail(G2048_EINVAL, w + "order must list n_order <= n episodes (all n when NULL; resume needs a list)");
    if (rows) {
        if (cap < 1 || cap > (int64_t)0x7FFFFFFF || n * cap > ((int64_t)1 << 40)) return sfail(G2048_EINVAL, w + "bad cap");
        if (board_stride < cap * n)
            return sfail(G2048_EINVAL, w + "board_stride " + std::to_string(board_stride) + " < cap * n = " +
                                           std::to_string(cap * n));
    } else if (cap < 1 || cap > (int64_t)0x7FFFFFFF) {
        return sfail(G2048_EINVAL, w + "step_limit must be in 1..2^31-1");
    }
    if (max_workgroups < 0) return sfail(G2048_EINVAL, w + "max_workgroups < 0");
    if (!env_state || !env_inc || !env_buf || !pol_state || !pol_inc || !pol_buf || !queue || !sus || !sus->board ||
        !sus->meta || !sus->total || !sus->list || !sus->count)
        return sfail(G2048_EINVAL, w + "a required buffer is NULL");
    a.tr = g2048_traj{};
    if (rows) {
        if (!traj || !traj->boards || !traj->actions || !traj->rewards || !traj->flags || !traj->lengths ||
            !traj->totals || !traj->max_tile || !traj->final_board)
            return sfail(G2048_EINVAL, w + "a required buffer is NULL");
        if (traj->probs) return sfail(G2048_EINVAL, w + "traj->probs must be NULL (a script has no probabilities to record)");
        a.tr = *traj;
    } else {
        if (!out || !out->lengths || !out->totals || !out->max_tile || !out->final_board)
            return sfail(G2048_EINVAL, w + "a required buffer is NULL");
        a.tr.lengths = out->lengths;
        a.tr.totals = out->totals;
        a.tr.max_tile = out->max_tile;
        a.tr.final_board = out->final_board;
    }
    a.script.kind = script->kind;
    a.script.order = script->kind == G2048_SCRIPT_PRIORITY ? scripted::order_word(script->order) : 0u;
    a.rc = g2048_internal::reward_cfg_of(*cfg);
    a.max_steps = cfg->max_steps;
    a.use_mask = cfg->use_action_mask;
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
    a.bstride = rows ? board_stride : 0;
    a.n = (uint32_t)n;
    a.cap = (uint32_t)cap;
    return G2048_OK;
}

// lanes = min(n_order, what max_workgroups allows): one workgroup per kScriptBlock episodes, at most 8 per CU (8 waves
// per SIMD, the most that can be resident; workgroups past that would only queue behind a persistent loop)
int script_grid(int64_t n_order, int max_workgroups) {
    int64_t grid = (n_order + kScriptBlock - 1) / kScriptBlock;
    const int64_t per_dev = 8 * (int64_t)device_cus();
    if (grid > per_dev) grid = per_dev;
    if (max_workgroups > 0 && grid > max_workgroups) grid = max_workgroups;
    return (int)grid;
}

template <class G, bool TRAJ>
int launch_script(const ScriptArgs& a, int max_workgroups, void* stream) {
    hipLaunchKernelGGL((scripted_kernel<G, TRAJ>), dim3(script_grid(a.n_order, max_workgroups)), dim3(kScriptBlock), 0,
                       (hipStream_t)stream, a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? G2048_OK : sfail(G2048_EHIP, hipGetErrorString(e));
}

}  // namespace
