// g2048_sized_search_wave.hip -- g2048_sized_search_wave_rollout / g2048_sized_search_wave_eval /
// g2048_sized_search_wave_choose (include/g2048_search_wave.h): g2048_search_wave.hip for N x N boards, 2 <= N <= 8
// (part of libg2048.so).  The same kernels (g2048_search_wave_kernel.h) over scripted::GameN<N>; board buffers are word
// planes.  Instantiation: N in 2..8 x depth 1 / 2 x {trajectory, score-only} = 28 kernels, and 14
// search_wave_choose_kernel; N is a template parameter, as in g2048_sized_search.hip.
#include "g2048_search_wave_kernel.h"

namespace {

// f.template operator()<GameN<size>>(): one switch for the three entry points (g2048_sized_search.hip's)
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
struct LaunchSearchWave {
    int depth;
    const SearchArgs& a;
    int max_workgroups;
    void* stream;
    template <class G>
    int operator()() const { return launch_search_wave<G, TRAJ>(depth, a, max_workgroups, stream); }
};

struct LaunchWaveChoose {
    int depth;
    const search::Weights& w;
    const uint64_t* boards;
    int64_t n;
    uint8_t* actions;
    int64_t* q;
    void* stream;
    template <class G>
    int operator()() const { return launch_wave_choose<G>(depth, w, boards, n, actions, q, stream); }
};

int bad_size(int size) { return sfail(G2048_EINVAL, "size must be in 2..8 (got " + std::to_string(size) + ")"); }

}  // namespace

extern "C" {

int g2048_sized_search_wave_rollout(int size, const g2048_search* sp, const g2048_env_cfg* cfg, uint64_t* env_state,
                                    const uint64_t* env_inc, uint64_t* env_buf, uint64_t* pol_state,
                                    const uint64_t* pol_inc, uint64_t* pol_buf, uint32_t* queue, const int32_t* order,
                                    int64_t n_order, int resume, const g2048_suspend* sus, int64_t n, int64_t cap,
                                    const g2048_traj* traj, int64_t board_stride, int max_workgroups, void* stream) {
    if (size < 2 || size > 8) return bad_size(size);
    SearchArgs a;
    int rc = search_args("sized search wave rollout", sp, cfg, env_state, env_inc, env_buf, pol_state, pol_inc, pol_buf,
                         queue, order, n_order, resume, sus, n, cap, true, traj, board_stride, nullptr, max_workgroups,
                         a);
    if (!rc) rc = wave_depth("sized search wave rollout", sp);
    if (rc) return rc;
    if (n_order == 0) return G2048_OK;
    return with_size(size, LaunchSearchWave<true>{sp->depth, a, max_workgroups, stream});
}

int g2048_sized_search_wave_eval(int size, const g2048_search* sp, const g2048_env_cfg* cfg, uint64_t* env_state,
                                 const uint64_t* env_inc, uint64_t* env_buf, uint64_t* pol_state,
                                 const uint64_t* pol_inc, uint64_t* pol_buf, uint32_t* queue, const int32_t* order,
                                 int64_t n_order, int resume, const g2048_suspend* sus, int64_t n, int64_t step_limit,
                                 const g2048_eval_out* out, int max_workgroups, void* stream) {
    if (size < 2 || size > 8) return bad_size(size);
    SearchArgs a;
    int rc = search_args("sized search wave eval", sp, cfg, env_state, env_inc, env_buf, pol_state, pol_inc, pol_buf,
                         queue, order, n_order, resume, sus, n, step_limit, false, nullptr, 0, out, max_workgroups, a);
    if (!rc) rc = wave_depth("sized search wave eval", sp);
    if (rc) return rc;
    if (n_order == 0) return G2048_OK;
    return with_size(size, LaunchSearchWave<false>{sp->depth, a, max_workgroups, stream});
}

int g2048_sized_search_wave_choose(int size, const g2048_search* sp, const uint64_t* boards, int64_t n,
                                   uint8_t* actions, int64_t* q, void* stream) {
    if (size < 2 || size > 8) return bad_size(size);
    search::Weights w;
    int rc = choose_args("sized search wave choose", sp, boards, n, actions, w);
    if (!rc) rc = wave_depth("sized search wave choose", sp);
    if (rc) return rc;
    if (n == 0) return G2048_OK;
    return with_size(size, LaunchWaveChoose{sp->depth, w, boards, n, actions, q, stream});
}

}  // extern "C"
