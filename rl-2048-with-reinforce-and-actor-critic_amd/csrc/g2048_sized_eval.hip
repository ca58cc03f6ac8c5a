// g2048_sized_eval.hip -- g2048_sized_eval (include/g2048_sized.h): score-only rollouts for N x N boards, 2 <= N <= 8
// (part of libg2048.so).  Evaluation reads only an episode's length, total reward, max tile and final board, so this
// unit instantiates sized_rollout_kernel (g2048_sized_rollout_kernel.h, described in g2048_sized_rollout.hip) with
// TRAJ = false: the same code -- forward, choice, policy draw, env step, fp64 total in step order, end-of-episode
// stores, queue claim and the suspend path -- without the trajectory row's stores and its row index.  The episodes are
// the ones g2048_sized_rollout plays, and nothing the launch touches grows with their lengths.
// `cap` is then no row count: it is the absolute step count at which an episode still running is suspended in this
// launch (step_limit), which keeps every launch bounded -- an episode that never ends (max_steps None with invalid
// actions allowed) is suspended every step_limit steps and the host decides when to give up.
// Instantiation: the 42 kernels of the trajectory form once more, in a unit of their own so that the two sets compile
// side by side.
// Roofline: as g2048_sized_rollout.hip (forward fp32-MFMA bound, then the owners' serial tail); no kernel speed-up is
// claimed -- what goes away is the row buffers' allocation, clearing and growth on the host side.
#include "g2048_sized_rollout_kernel.h"

namespace {

int efail(int code, const std::string& msg) { return g2048_internal::set_error(code, msg.c_str()); }

}  // namespace

extern "C" {

int g2048_sized_eval(int size, const float* packed, int n_hidden, const int32_t* hidden, int activation,
                     const g2048_env_cfg* cfg, int greedy, uint64_t* env_state, const uint64_t* env_inc,
                     uint64_t* env_buf, uint64_t* pol_state, const uint64_t* pol_inc, uint64_t* pol_buf,
                     uint32_t* queue, const int32_t* order, int64_t n_order, int resume, const g2048_suspend* sus,
                     int64_t n, int64_t step_limit, const g2048_eval_out* out, int max_workgroups, void* stream) {
    // every check precedes every HIP call
    if (size < 2 || size > 8) return efail(G2048_EINVAL, "size must be in 2..8 (got " + std::to_string(size) + ")");
    int rc = g2048_internal::check_env_cfg(cfg);
    if (rc) return rc;
    if (n < 0 || n > (int64_t)0x7FFFFFFF) return efail(G2048_EINVAL, "n out of range");
    if (n_order < 0 || n_order > n || (!order && n_order != n) || (resume && !order))
        return efail(G2048_EINVAL,
                     "sized eval: order must list n_order <= n episodes (all n when NULL; resume needs a list)");
    if (step_limit < 1 || step_limit > (int64_t)0x7FFFFFFF)
        return efail(G2048_EINVAL, "sized eval: step_limit must be in 1..2^31-1");
    if (max_workgroups < 0) return efail(G2048_EINVAL, "sized eval: max_workgroups < 0");
    DeepNet net;
    if (!obs_ok(cfg->obs_mode) || !sized_layout(size, n_hidden, hidden, cfg->obs_mode == G2048_OBS_ONEHOT, net))
        return efail(G2048_EINVAL, "sized policy: obs raw / log2 / onehot, 1..4 hidden layers of 1..256 units");
    if (activation != G2048_ACT_RELU && activation != G2048_ACT_SIGMOID)
        return efail(G2048_EINVAL, "Unsupported activation");
    if (!packed || !env_state || !env_inc || !env_buf || !pol_state || !pol_inc || !pol_buf || !queue || !sus || !out ||
        !sus->board || !sus->meta || !sus->total || !sus->list || !sus->count || !out->lengths || !out->totals ||
        !out->max_tile || !out->final_board)
        return efail(G2048_EINVAL, "sized eval: a required buffer is NULL");
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
    a.tr = g2048_traj{};                                // no rows: the score-only kernels never read these
    a.tr.lengths = out->lengths;
    a.tr.totals = out->totals;
    a.tr.max_tile = out->max_tile;
    a.tr.final_board = out->final_board;
    a.bstride = 0;
    a.n = (uint32_t)n;
    a.cap = (uint32_t)step_limit;
    launch_sized_roll<false>(a, cfg->obs_mode, activation, n_order, max_workgroups, (hipStream_t)stream);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? G2048_OK : efail(G2048_EHIP, hipGetErrorString(e));
}

}  // extern "C"
