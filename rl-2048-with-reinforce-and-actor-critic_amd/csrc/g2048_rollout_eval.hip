// g2048_rollout_eval.hip -- g2048_rollout_eval (include/g2048_eval.h): the score-only form of g2048_rollout, the
// two-layer family's persistent whole-rollout kernel (part of libg2048.so).  This unit instantiates rollout_kernel
// (g2048_policy_roll.h, described in g2048_policy.hip) with TRAJ = false: the same code -- the MLP split over the
// workgroup's four waves, choice, policy draw, env step, fp64 total in step order, end-of-episode stores and the queue
// claim -- without the trajectory row's stores and its row index.  The episodes are the ones g2048_rollout plays and
// the launch touches O(n) memory whatever max_steps is.  The kernel has no suspend path: as in g2048_rollout a finite
// cfg->max_steps is required and bounds the launch (cap = max(max_steps, 1), by which every episode has ended).
// Instantiation: the 64 kernels of the trajectory form ({1, 2, 4, 8}^2 hidden tiles x {ReLU, Sigmoid} x {log2, raw})
// once more, in a unit of their own so that they compile beside g2048_policy.hip, the unit a build from an empty cache
// waits for.
// Roofline: as the rollout kernel of g2048_policy.hip; no kernel speed-up is claimed.
#include "g2048_policy_roll.h"

namespace g2048_internal {   // g2048.hip
int set_error(int code, const char* msg);
int device_tables(const uint8_t*& tab, int& cus);
int check_env_cfg(const g2048_env_cfg* c);
g2048::RewardCfg reward_cfg_of(const g2048_env_cfg& c);
}  // namespace g2048_internal

namespace {
int efail(int code, const char* msg) { return g2048_internal::set_error(code, msg); }
}  // namespace

extern "C" {

int g2048_rollout_eval(const float* packed, int h1, int h2, int activation, const g2048_env_cfg* cfg, int greedy,
                       const uint64_t* env_state, const uint64_t* env_inc, const uint64_t* env_buf,
                       const uint64_t* pol_state, const uint64_t* pol_inc, const uint64_t* pol_buf, uint32_t* queue,
                       int64_t n, const g2048_eval_out* out, void* stream) {
    int rc = g2048_internal::check_env_cfg(cfg);
    if (rc) return rc;
    if (n < 0 || n > (int64_t)0x7FFFFFFF) return efail(G2048_EINVAL, "n out of range");
    if (cfg->obs_mode != G2048_OBS_LOG2 && cfg->obs_mode != G2048_OBS_RAW)
        return efail(G2048_EINVAL, "fused rollout: obs_mode must be log2 or raw");
    if (cfg->max_steps < 0) return efail(G2048_EINVAL, "fused rollout: max_steps must be set (>= 0)");
    if (g2048_policy_packed_size(h1, h2) < 0) return efail(G2048_EINVAL, "fused policy: hidden sizes must be in 1..256");
    if (activation != G2048_ACT_RELU && activation != G2048_ACT_SIGMOID)
        return efail(G2048_EINVAL, "Unsupported activation");
    if (!packed || !env_state || !env_inc || !env_buf || !pol_state || !pol_inc || !pol_buf || !queue || !out ||
        !out->lengths || !out->totals || !out->max_tile || !out->final_board)
        return efail(G2048_EINVAL, "rollout eval: a required buffer is NULL");
    if (n == 0) return G2048_OK;
    const uint8_t* tab = nullptr;
    int cus = 256;
    if ((rc = g2048_internal::device_tables(tab, cus))) return rc;
    RolloutArgs a{};                                    // no rows: the score-only kernels never read their pointers
    a.net = packed;
    a.tab = tab;
    a.rc = g2048_internal::reward_cfg_of(*cfg);
    a.max_steps = cfg->max_steps;
    a.obs_scale = cfg->obs_log2_scale;
    a.use_mask = cfg->use_action_mask;
    a.greedy = greedy;
    a.env_rs = env_state;
    a.env_inc = env_inc;
    a.env_buf = env_buf;
    a.pol_rs = pol_state;
    a.pol_inc = pol_inc;
    a.pol_buf = pol_buf;
    a.next = queue;
    a.lengths = out->lengths;
    a.totals = out->totals;
    a.max_tile = out->max_tile;
    a.final_board = out->final_board;
    a.n = (uint32_t)n;
    a.cap = (uint32_t)(cfg->max_steps > 1 ? cfg->max_steps : 1);
    launch_rollout_form<false>(a, h1, h2, activation, cfg->obs_mode, n, cus, (hipStream_t)stream);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return efail(G2048_EHIP, hipGetErrorString(e));
    return G2048_OK;
}

}  // extern "C"
