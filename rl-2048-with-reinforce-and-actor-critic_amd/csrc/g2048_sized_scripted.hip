// g2048_sized_scripted.hip -- g2048_sized_scripted_rollout / g2048_sized_scripted_eval (include/g2048_scripted.h):
// g2048_scripted.hip for N x N boards, 2 <= N <= 8 (part of libg2048.so).  The same kernel (g2048_scripted_kernel.h)
// over scripted::GameN<N>: the board is W = ceil(N*N / 16) words per lane in registers, the move, mask and spawn are
// g2048_sized_core.h's plain-ALU code, and board buffers are word planes ([W, cap, n] rows, [W, n] final / suspended).
// Instantiation: N in 2..8 x {trajectory, score-only} = 14 kernels; N is a template parameter, as in
// g2048_sized_rollout.hip and for its reason (one size's literal masks per kernel).
#include "g2048_scripted_kernel.h"

namespace {

template <bool TRAJ>
int launch_sized_script(int size, const ScriptArgs& a, int max_workgroups, void* stream) {
    switch (size) {
        case 2: return launch_script<scripted::GameN<2>, TRAJ>(a, max_workgroups, stream);
        case 3: return launch_script<scripted::GameN<3>, TRAJ>(a, max_workgroups, stream);
        case 4: return launch_script<scripted::GameN<4>, TRAJ>(a, max_workgroups, stream);
        case 5: return launch_script<scripted::GameN<5>, TRAJ>(a, max_workgroups, stream);
        case 6: return launch_script<scripted::GameN<6>, TRAJ>(a, max_workgroups, stream);
        case 7: return launch_script<scripted::GameN<7>, TRAJ>(a, max_workgroups, stream);
        default: return launch_script<scripted::GameN<8>, TRAJ>(a, max_workgroups, stream);
    }
}

}  // namespace

extern "C" {

int g2048_sized_scripted_rollout(int size, const g2048_script* script, const g2048_env_cfg* cfg, uint64_t* env_state,
                                 const uint64_t* env_inc, uint64_t* env_buf, uint64_t* pol_state,
                                 const uint64_t* pol_inc, uint64_t* pol_buf, uint32_t* queue, const int32_t* order,
                                 int64_t n_order, int resume, const g2048_suspend* sus, int64_t n, int64_t cap,
                                 const g2048_traj* traj, int64_t board_stride, int max_workgroups, void* stream) {
    if (size < 2 || size > 8) return sfail(G2048_EINVAL, "size must be in 2..8 (got " + std::to_string(size) + ")");
    ScriptArgs a;
    const int rc = script_args("sized scripted rollout", script, cfg, env_state, env_inc, env_buf, pol_state, pol_inc,
                               pol_buf, queue, order, n_order, resume, sus, n, cap, true, traj, board_stride, nullptr,
                               max_workgroups, a);
    if (rc) return rc;
    if (n_order == 0) return G2048_OK;
    return launch_sized_script<true>(size, a, max_workgroups, stream);
}

int g2048_sized_scripted_eval(int size, const g2048_script* script, const g2048_env_cfg* cfg, uint64_t* env_state,
                              const uint64_t* env_inc, uint64_t* env_buf, uint64_t* pol_state, const uint64_t* pol_inc,
                              uint64_t* pol_buf, uint32_t* queue, const int32_t* order, int64_t n_order, int resume,
                              const g2048_suspend* sus, int64_t n, int64_t step_limit, const g2048_eval_out* out,
                              int max_workgroups, void* stream) {
    if (size < 2 || size > 8) return sfail(G2048_EINVAL, "size must be in 2..8 (got " + std::to_string(size) + ")");
    ScriptArgs a;
    const int rc = script_args("sized scripted eval", script, cfg, env_state, env_inc, env_buf, pol_state, pol_inc,
                               pol_buf, queue, order, n_order, resume, sus, n, step_limit, false, nullptr, 0, out,
                               max_workgroups, a);
    if (rc) return rc;
    if (n_order == 0) return G2048_OK;
    return launch_sized_script<false>(size, a, max_workgroups, stream);
}

}  // extern "C"
