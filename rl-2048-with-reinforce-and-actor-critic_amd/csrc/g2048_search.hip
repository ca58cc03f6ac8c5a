// g2048_search.hip -- g2048_search_rollout / g2048_search_eval / g2048_search_choose (include/g2048_search.h): whole
// 4 x 4 episodes of the expectimax player in persistent launches, one episode per lane, and its choice on arbitrary
// boards (part of libg2048.so).  The kernels, their shape, termination argument and roofline are in
// g2048_search_kernel.h; the player is g2048_search_core.h, which the CPU tests run too.  The move is board_move_alu,
// for g2048_scripted.hip's reasons -- here it runs 4 .. thousands of times per step instead of once.
// Instantiation: depth 0 / 1 / 2 x {trajectory, score-only} = 6 kernels, and 3 search_choose_kernel.
#include "g2048_search_kernel.h"

extern "C" {

int g2048_search_rollout(const g2048_search* sp, const g2048_env_cfg* cfg, uint64_t* env_state, const uint64_t* env_inc,
                         uint64_t* env_buf, uint64_t* pol_state, const uint64_t* pol_inc, uint64_t* pol_buf,
                         uint32_t* queue, const int32_t* order, int64_t n_order, int resume, const g2048_suspend* sus,
                         int64_t n, int64_t cap, const g2048_traj* traj, int max_workgroups, void* stream) {
    SearchArgs a;
    const int64_t stride = cap > 0 && n > 0 ? cap * n : 0;   // one plane: [cap, n]
    const int rc = search_args("search rollout", sp, cfg, env_state, env_inc, env_buf, pol_state, pol_inc, pol_buf,
                               queue, order, n_order, resume, sus, n, cap, true, traj, stride, nullptr, max_workgroups, a);
    if (rc) return rc;
    if (n_order == 0) return G2048_OK;
    return launch_search<scripted::Game4, true>(sp->depth, a, max_workgroups, stream);
}

int g2048_search_eval(const g2048_search* sp, const g2048_env_cfg* cfg, uint64_t* env_state, const uint64_t* env_inc,
                      uint64_t* env_buf, uint64_t* pol_state, const uint64_t* pol_inc, uint64_t* pol_buf, uint32_t* queue,
                      const int32_t* order, int64_t n_order, int resume, const g2048_suspend* sus, int64_t n,
                      int64_t step_limit, const g2048_eval_out* out, int max_workgroups, void* stream) {
    SearchArgs a;
    const int rc = search_args("search eval", sp, cfg, env_state, env_inc, env_buf, pol_state, pol_inc, pol_buf, queue,
                               order, n_order, resume, sus, n, step_limit, false, nullptr, 0, out, max_workgroups, a);
    if (rc) return rc;
    if (n_order == 0) return G2048_OK;
    return launch_search<scripted::Game4, false>(sp->depth, a, max_workgroups, stream);
}

int g2048_search_choose(const g2048_search* sp, const uint64_t* boards, int64_t n, uint8_t* actions, int64_t* q,
                        void* stream) {
    search::Weights w;
    const int rc = choose_args("search choose", sp, boards, n, actions, w);
    if (rc) return rc;
    if (n == 0) return G2048_OK;
    return launch_choose<scripted::Game4>(sp->depth, w, boards, n, actions, q, stream);
}

}  // extern "C"
