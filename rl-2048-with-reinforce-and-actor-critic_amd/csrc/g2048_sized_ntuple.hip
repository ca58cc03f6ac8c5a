// g2048_sized_ntuple.hip -- g2048_sized_ntuple_rollout / _eval / _choose / _values / _td_update
// (include/g2048_ntuple.h): g2048_ntuple.hip for N x N boards, 2 <= N <= 8 (part of libg2048.so).  The same kernels
// (g2048_ntuple_kernel.h) over scripted::GameN<N>: W = ceil(N*N / 16) board words per lane in registers, the move is
// g2048_sized_core.h's plain-ALU board_move, board buffers are word planes.
// Instantiation: N in 2..8 x (depth 0 / 1 x {trajectory, score-only} = 4 kernels, 2 ntuple_choose_kernel, 1
// ntuple_values_kernel, the two passes of the update) = 63 kernels; N is a template parameter, as in
// g2048_sized_scripted.hip.
#include "g2048_ntuple_kernel.h"

namespace {

// f.template operator()<GameN<size>>(): one switch for the five entry points
template <class F>
int with_size(int size, const F& f) {
    switch (size) {
        case 2: return f.template operator()<scripted::GameN<2>>();
        case 3: return f.template operator()<scripted::GameN<3>>();
        case 4: return f.template operator()<scripted::GameN<4>>();
        case 5: return f.template operator()<scripted::GameN<5>>();
        case 6: return f.template operator()<scripted::GameN<6>>();
        case 7: return f.template operator()<scripted::GameN<7>>();
        default: return f.template operator()<scripted::GameN<8>>();
    }
}

template <bool TRAJ>
struct LaunchPlay {
    int depth;
    const NtArgs& a;
    int max_workgroups;
    void* stream;
    template <class G>
    int operator()() const { return launch_ntuple<G, TRAJ>(depth, a, max_workgroups, stream); }
};

struct LaunchChoose {
    int depth;
    const NtBoardArgs& a;
    void* stream;
    template <class G>
    int operator()() const { return launch_nt_choose<G>(depth, a, stream); }
};

struct LaunchValues {
    const NtBoardArgs& a;
    void* stream;
    template <class G>
    int operator()() const { return launch_nt_values<G>(a, stream); }
};

struct LaunchTd {
    const NtTdArgs& a;
    void* stream;
    template <class G>
    int operator()() const { return launch_td<G>(a, stream); }
};

int bad_size(int size) { return sfail(G2048_EINVAL, "size must be in 2..8 (got " + std::to_string(size) + ")"); }

}  // namespace

extern "C" {

int g2048_sized_ntuple_rollout(int size, const g2048_ntuple* nt, const g2048_env_cfg* cfg, uint64_t* env_state,
                               const uint64_t* env_inc, uint64_t* env_buf, uint64_t* pol_state, const uint64_t* pol_inc,
                               uint64_t* pol_buf, uint32_t* queue, const int32_t* order, int64_t n_order, int resume,
                               const g2048_suspend* sus, int64_t n, int64_t cap, const g2048_traj* traj,
                               int64_t board_stride, int max_workgroups, void* stream) {
    if (size < 2 || size > 8) return bad_size(size);
    NtArgs a;
    const int rc = ntuple_args("sized ntuple rollout", size, nt, cfg, env_state, env_inc, env_buf, pol_state, pol_inc,
                               pol_buf, queue, order, n_order, resume, sus, n, cap, true, traj, board_stride, nullptr,
                               max_workgroups, a);
    if (rc) return rc;
    if (n_order == 0) return G2048_OK;
    return with_size(size, LaunchPlay<true>{nt->depth, a, max_workgroups, stream});
}

int g2048_sized_ntuple_eval(int size, const g2048_ntuple* nt, const g2048_env_cfg* cfg, uint64_t* env_state,
                            const uint64_t* env_inc, uint64_t* env_buf, uint64_t* pol_state, const uint64_t* pol_inc,
                            uint64_t* pol_buf, uint32_t* queue, const int32_t* order, int64_t n_order, int resume,
                            const g2048_suspend* sus, int64_t n, int64_t step_limit, const g2048_eval_out* out,
                            int max_workgroups, void* stream) {
    if (size < 2 || size > 8) return bad_size(size);
    NtArgs a;
    const int rc = ntuple_args("sized ntuple eval", size, nt, cfg, env_state, env_inc, env_buf, pol_state, pol_inc,
                               pol_buf, queue, order, n_order, resume, sus, n, step_limit, false, nullptr, 0, out,
                               max_workgroups, a);
    if (rc) return rc;
    if (n_order == 0) return G2048_OK;
    return with_size(size, LaunchPlay<false>{nt->depth, a, max_workgroups, stream});
}

int g2048_sized_ntuple_choose(int size, const g2048_ntuple* nt, const uint64_t* boards, int64_t n, uint8_t* actions,
                              int64_t* q, void* stream) {
    if (size < 2 || size > 8) return bad_size(size);
    NtBoardArgs a;
    const int rc = board_args("sized ntuple choose", size, nt, boards, n, actions, a);
    if (rc) return rc;
    if (n == 0) return G2048_OK;
    a.actions = actions;
    a.q = q;
    return with_size(size, LaunchChoose{nt->depth, a, stream});
}

int g2048_sized_ntuple_values(int size, const g2048_ntuple* nt, const uint64_t* boards, int64_t n, int64_t* values,
                              void* stream) {
    if (size < 2 || size > 8) return bad_size(size);
    NtBoardArgs a;
    const int rc = board_args("sized ntuple values", size, nt, boards, n, values, a);
    if (rc) return rc;
    if (n == 0) return G2048_OK;
    a.actions = nullptr;
    a.q = values;
    return with_size(size, LaunchValues{a, stream});
}

int g2048_sized_ntuple_td_update(int size, const g2048_ntuple* nt, const uint64_t* boards, int64_t board_stride,
                                 const uint8_t* actions, const uint8_t* flags, const int32_t* lengths, int64_t n,
                                 int64_t T, int32_t lr_num, int32_t lr_shift, int64_t* scratch, int64_t* stats,
                                 void* stream) {
    if (size < 2 || size > 8) return bad_size(size);
    NtTdArgs a;
    const int rc = td_args("sized ntuple td_update", size, nt, boards, board_stride, actions, flags, lengths, n, T,
                           lr_num, lr_shift, scratch, stats, a);
    if (rc) return rc;
    if (n == 0 || T == 0) return G2048_OK;
    return with_size(size, LaunchTd{a, stream});
}

}  // extern "C"
