// g2048_ntuple.hip -- g2048_ntuple_rollout / _eval / _choose / _values / _td_update (include/g2048_ntuple.h): the
// n-tuple value network on the 4 x 4 game -- whole episodes of its player in persistent launches, one episode per lane,
// its choice and value on arbitrary boards and the batched TD(0) update (part of libg2048.so).  The kernels, their
// shape, termination argument and roofline are in g2048_ntuple_kernel.h; the model is g2048_ntuple_core.h, which the
// CPU tests run too.  The move is board_move_alu, for g2048_scripted.hip's reasons.
// Instantiation: depth 0 / 1 x {trajectory, score-only} = 4 kernels, 2 ntuple_choose_kernel, 1 ntuple_values_kernel
// and the two passes of the update.
#include "g2048_ntuple_kernel.h"

extern "C" {

int g2048_ntuple_rollout(const g2048_ntuple* nt, const g2048_env_cfg* cfg, uint64_t* env_state, const uint64_t* env_inc,
                         uint64_t* env_buf, uint64_t* pol_state, const uint64_t* pol_inc, uint64_t* pol_buf,
                         uint32_t* queue, const int32_t* order, int64_t n_order, int resume, const g2048_suspend* sus,
                         int64_t n, int64_t cap, const g2048_traj* traj, int max_workgroups, void* stream) {
    NtArgs a;
    const int64_t stride = cap > 0 && n > 0 ? cap * n : 0;   // one plane: [cap, n]
    const int rc = ntuple_args("ntuple rollout", 4, nt, cfg, env_state, env_inc, env_buf, pol_state, pol_inc, pol_buf,
                               queue, order, n_order, resume, sus, n, cap, true, traj, stride, nullptr, max_workgroups, a);
    if (rc) return rc;
    if (n_order == 0) return G2048_OK;
    return launch_ntuple<scripted::Game4, true>(nt->depth, a, max_workgroups, stream);
}

int g2048_ntuple_eval(const g2048_ntuple* nt, const g2048_env_cfg* cfg, uint64_t* env_state, const uint64_t* env_inc,
                      uint64_t* env_buf, uint64_t* pol_state, const uint64_t* pol_inc, uint64_t* pol_buf, uint32_t* queue,
                      const int32_t* order, int64_t n_order, int resume, const g2048_suspend* sus, int64_t n,
                      int64_t step_limit, const g2048_eval_out* out, int max_workgroups, void* stream) {
    NtArgs a;
    const int rc = ntuple_args("ntuple eval", 4, nt, cfg, env_state, env_inc, env_buf, pol_state, pol_inc, pol_buf, queue,
                               order, n_order, resume, sus, n, step_limit, false, nullptr, 0, out, max_workgroups, a);
    if (rc) return rc;
    if (n_order == 0) return G2048_OK;
    return launch_ntuple<scripted::Game4, false>(nt->depth, a, max_workgroups, stream);
}

int g2048_ntuple_choose(const g2048_ntuple* nt, const uint64_t* boards, int64_t n, uint8_t* actions, int64_t* q,
                        void* stream) {
    NtBoardArgs a;
    const int rc = board_args("ntuple choose", 4, nt, boards, n, actions, a);
    if (rc) return rc;
    if (n == 0) return G2048_OK;
    a.actions = actions;
    a.q = q;
    return launch_nt_choose<scripted::Game4>(nt->depth, a, stream);
}

int g2048_ntuple_values(const g2048_ntuple* nt, const uint64_t* boards, int64_t n, int64_t* values, void* stream) {
    NtBoardArgs a;
    const int rc = board_args("ntuple values", 4, nt, boards, n, values, a);
    if (rc) return rc;
    if (n == 0) return G2048_OK;
    a.actions = nullptr;
    a.q = values;
    return launch_nt_values<scripted::Game4>(a, stream);
}

int g2048_ntuple_td_update(const g2048_ntuple* nt, const uint64_t* boards, const uint8_t* actions, const uint8_t* flags,
                           const int32_t* lengths, int64_t n, int64_t T, int32_t lr_num, int32_t lr_shift,
                           int64_t* scratch, int64_t* stats, void* stream) {
    NtTdArgs a;
    const int64_t stride = n > 0 && T > 0 && n <= (int64_t)0x7FFFFFFF && T <= (int64_t)0x7FFFFFFF ? n * T : 0;
    const int rc = td_args("ntuple td_update", 4, nt, boards, stride, actions, flags, lengths, n, T, lr_num, lr_shift,
                           scratch, stats, a);
    if (rc) return rc;
    if (n == 0 || T == 0) return G2048_OK;
    return launch_td<scripted::Game4>(a, stream);
}

}  // extern "C"
