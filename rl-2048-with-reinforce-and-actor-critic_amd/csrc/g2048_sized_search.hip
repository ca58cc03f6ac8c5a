// g2048_sized_search.hip -- g2048_sized_search_rollout / g2048_sized_search_eval / g2048_sized_search_choose
// (include/g2048_search.h): g2048_search.hip for N x N boards, 2 <= N <= 8 (part of libg2048.so).  The same kernels
// (g2048_search_kernel.h) over scripted::GameN<N>: W = ceil(N*N / 16) board words per lane and per search level in
// registers, the move is g2048_sized_core.h's plain-ALU board_move, board buffers are word planes.
// Instantiation: N in 2..8 x depth 0 / 1 / 2 x {trajectory, score-only} = 42 kernels, and 21 search_choose_kernel; N
// is a template parameter, as in g2048_sized_scripted.hip.
#include "g2048_search_kernel.h"

namespace {

// f.template operator()<GameN<size>>(): one switch for the three entry points
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
struct LaunchSearch {
    int depth;
    const SearchArgs& a;
    int max_workgroups;
    void* stream;
    template <class G>
    int operator()() const { return launch_search<G, TRAJ>(depth, a, max_workgroups, stream); }
};

struct LaunchChoose {
    int depth;
    const search::Weights& w;
    const uint64_t* boards;
    int64_t n;
    uint8_t* actions;
    int64_t* q;
    void* stream;
    template <class G>
    int operator()() const { return launch_choose<G>(depth, w, boards, n, actions, q, stream); }
};

int bad_size(int size) { return sfail(G2048_EINVAL, "size must be in 2..8 (got " + std::to_string(size) + ")"); }

}  // namespace

extern "C" {

int g2048_sized_search_rollout(int size, const g2048_search* sp, const g2048_env_cfg* cfg, uint64_t* env_state,
                               const uint64_t* env_inc, uint64_t* env_buf, uint64_t* pol_state, const uint64_t* pol_inc,
                               uint64_t* pol_buf, uint32_t* queue, const int32_t* order, int64_t n_order, int resume,
                               const g2048_suspend* sus, int64_t n, int64_t cap, const g2048_traj* traj,
                               int64_t board_stride, int max_workgroups, void* stream) {
    if (size < 2 || size > 8) return bad_size(size);
    SearchArgs a;
    const int rc = search_args("sized search rollout", sp, cfg, env_state, env_inc, env_buf, pol_state, pol_inc, pol_buf,
                               queue, order, n_order, resume, sus, n, cap, true, traj, board_stride, nullptr,
                               max_workgroups, a);
    if (rc) return rc;
    if (n_order == 0) return G2048_OK;
    return with_size(size, LaunchSearch<true>{sp->depth, a, max_workgroups, stream});
}

int g2048_sized_search_eval(int size, const g2048_search* sp, const g2048_env_cfg* cfg, uint64_t* env_state,
                            const uint64_t* env_inc, uint64_t* env_buf, uint64_t* pol_state, const uint64_t* pol_inc,
                            uint64_t* pol_buf, uint32_t* queue, const int32_t* order, int64_t n_order, int resume,
                            const g2048_suspend* sus, int64_t n, int64_t step_limit, const g2048_eval_out* out,
                            int max_workgroups, void* stream) {
    if (size < 2 || size > 8) return bad_size(size);
    SearchArgs a;
    const int rc = search_args("sized search eval", sp, cfg, env_state, env_inc, env_buf, pol_state, pol_inc, pol_buf,
                               queue, order, n_order, resume, sus, n, step_limit, false, nullptr, 0, out, max_workgroups,
                               a);
    if (rc) return rc;
    if (n_order == 0) return G2048_OK;
    return with_size(size, LaunchSearch<false>{sp->depth, a, max_workgroups, stream});
}

int g2048_sized_search_choose(int size, const g2048_search* sp, const uint64_t* boards, int64_t n, uint8_t* actions,
                              int64_t* q, void* stream) {
    if (size < 2 || size > 8) return bad_size(size);
    search::Weights w;
    const int rc = choose_args("sized search choose", sp, boards, n, actions, w);
    if (rc) return rc;
    if (n == 0) return G2048_OK;
    return with_size(size, LaunchChoose{sp->depth, w, boards, n, actions, q, stream});
}

}  // extern "C"
