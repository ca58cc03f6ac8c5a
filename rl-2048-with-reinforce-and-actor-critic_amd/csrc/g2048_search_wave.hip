// g2048_search_wave.hip -- g2048_search_wave_rollout / g2048_search_wave_eval / g2048_search_wave_choose
// (include/g2048_search_wave.h): g2048_search.hip's three calls for the 4 x 4 game with one episode, or one board, per
// wave instead of per lane (part of libg2048.so).  The kernels, their shape, termination argument and roofline are in
// g2048_search_wave_kernel.h; the split player is g2048_search_wave_core.h, which the CPU tests run too.
// Instantiation: depth 1 / 2 x {trajectory, score-only} = 4 kernels, and 2 search_wave_choose_kernel.
#include "g2048_search_wave_kernel.h"

extern "C" {

int g2048_search_wave_rollout(const g2048_search* sp, const g2048_env_cfg* cfg, uint64_t* env_state,
                              const uint64_t* env_inc, uint64_t* env_buf, uint64_t* pol_state, const uint64_t* pol_inc,
                              uint64_t* pol_buf, uint32_t* queue, const int32_t* order, int64_t n_order, int resume,
                              const g2048_suspend* sus, int64_t n, int64_t cap, const g2048_traj* traj,
                              int max_workgroups, void* stream) {
    SearchArgs a;
    const int64_t stride = cap > 0 && n > 0 ? cap * n : 0;   // one plane: [cap, n]
    int rc = search_args("search wave rollout", sp, cfg, env_state, env_inc, env_buf, pol_state, pol_inc, pol_buf, queue,
                         order, n_order, resume, sus, n, cap, true, traj, stride, nullptr, max_workgroups, a);
    if (!rc) rc = wave_depth("search wave rollout", sp);
    if (rc) return rc;
    if (n_order == 0) return G2048_OK;
    return launch_search_wave<scripted::Game4, true>(sp->depth, a, max_workgroups, stream);
}

int g2048_search_wave_eval(const g2048_search* sp, const g2048_env_cfg* cfg, uint64_t* env_state,
                           const uint64_t* env_inc, uint64_t* env_buf, uint64_t* pol_state, const uint64_t* pol_inc,
                           uint64_t* pol_buf, uint32_t* queue, const int32_t* order, int64_t n_order, int resume,
                           const g2048_suspend* sus, int64_t n, int64_t step_limit, const g2048_eval_out* out,
                           int max_workgroups, void* stream) {
    SearchArgs a;
    int rc = search_args("search wave eval", sp, cfg, env_state, env_inc, env_buf, pol_state, pol_inc, pol_buf, queue,
                         order, n_order, resume, sus, n, step_limit, false, nullptr, 0, out, max_workgroups, a);
    if (!rc) rc = wave_depth("search wave eval", sp);
    if (rc) return rc;
    if (n_order == 0) return G2048_OK;
    return launch_search_wave<scripted::Game4, false>(sp->depth, a, max_workgroups, stream);
}

int g2048_search_wave_choose(const g2048_search* sp, const uint64_t* boards, int64_t n, uint8_t* actions, int64_t* q,
                             void* stream) {
    search::Weights w;
    int rc = choose_args("search wave choose", sp, boards, n, actions, w);
    if (!rc) rc = wave_depth("search wave choose", sp);
    if (rc) return rc;
    if (n == 0) return G2048_OK;
    return launch_wave_choose<scripted::Game4>(sp->depth, w, boards, n, actions, q, stream);
}

}  // extern "C"
