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
// The kernel and its launch helpers are in g2048_sized_rollout_kernel.h, which g2048_sized_eval.hip instantiates
// once more without the trajectory row (the score-only form); this unit instantiates the trajectory form.
#include "g2048_sized_rollout_kernel.h"

namespace {

int rfail(int code, const std::string& msg) { return g2048_internal::set_error(code, msg.c_str()); }

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
    launch_sized_roll<true>(a, cfg->obs_mode, activation, n_order, max_workgroups, (hipStream_t)stream);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? G2048_OK : rfail(G2048_EHIP, hipGetErrorString(e));
}

}  // extern "C"
