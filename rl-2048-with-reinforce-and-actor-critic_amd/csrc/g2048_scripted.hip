// g2048_scripted.hip -- g2048_scripted_rollout / g2048_scripted_eval (include/g2048_scripted.h): whole 4 x 4 episodes
// of a scripted player (a priority order over the valid moves, or a uniform draw among them) in persistent launches,
// one episode per lane (part of libg2048.so).  The kernel, its shape, its termination argument and its roofline are
// in g2048_scripted_kernel.h; the per-step code is g2048_scripted_core.h, which the CPU tests run too.
// The move: board_move_alu (g2048_core.h), not the LDS row tables.  With one episode per lane the four actions of a
// wave differ, board_move_alu is branch-free straight-line code for that case, and it needs neither row tables in
// LDS (a fill per workgroup, and LDS that limits the waves per CU in a kernel that otherwise uses none) nor
// g2048_init.  The table-through-L1/L2 form the MFMA rollouts use would add eight dependent global loads per step to
// a loop that has no other memory latency.
// Instantiation: {trajectory, score-only} = 2 kernels.
#include "g2048_scripted_kernel.h"

extern "C" {

int g2048_scripted_rollout(const g2048_script* script, const g2048_env_cfg* cfg, uint64_t* env_state,
                           const uint64_t* env_inc, uint64_t* env_buf, uint64_t* pol_state, const uint64_t* pol_inc,
                           uint64_t* pol_buf, uint32_t* queue, const int32_t* order, int64_t n_order, int resume,
                           const g2048_suspend* sus, int64_t n, int64_t cap, const g2048_traj* traj, int max_workgroups,
                           void* stream) {
    ScriptArgs a;
    const int64_t stride = cap > 0 && n > 0 ? cap * n : 0;   // one plane: [cap, n]
    const int rc = script_args("scripted rollout", script, cfg, env_state, env_inc, env_buf, pol_state, pol_inc, pol_buf,
                               queue, order, n_order, resume, sus, n, cap, true, traj, stride, nullptr, max_workgroups, a);
    if (rc) return rc;
    if (n_order == 0) return G2048_OK;
    return launch_script<scripted::Game4, true>(a, max_workgroups, stream);
}

int g2048_scripted_eval(const g2048_script* script, const g2048_env_cfg* cfg, uint64_t* env_state,
                        const uint64_t* env_inc, uint64_t* env_buf, uint64_t* pol_state, const uint64_t* pol_inc,
                        uint64_t* pol_buf, uint32_t* queue, const int32_t* order, int64_t n_order, int resume,
                        const g2048_suspend* sus, int64_t n, int64_t step_limit, const g2048_eval_out* out,
                        int max_workgroups, void* stream) {
    ScriptArgs a;
    const int rc = script_args("scripted eval", script, cfg, env_state, env_inc, env_buf, pol_state, pol_inc, pol_buf,
                               queue, order, n_order, resume, sus, n, step_limit, false, nullptr, 0, out, max_workgroups,
                               a);
    if (rc) return rc;
    if (n_order == 0) return G2048_OK;
    return launch_script<scripted::Game4, false>(a, max_workgroups, stream);
}

}  // extern "C"
