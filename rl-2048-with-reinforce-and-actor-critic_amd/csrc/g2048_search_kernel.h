// g2048_search_kernel.h -- search_kernel and search_choose_kernel, their argument checks and their launches, shared
// by the two translation units that instantiate them: g2048_search.hip (the 4 x 4 game) and g2048_sized_search.hip
// (sizes 2..8).  The per-step code is search::episode_step of g2048_search_core.h, the code the CPU tests run.
//
// Shape: scripted_kernel's -- the same loop, play_episodes of g2048_scripted_kernel.h, with another player (and that
// file's argument checks and grid): one episode per lane, persistent, workgroups of 256 threads = 4 waves that never
// talk to each other, no LDS, no barrier.  What differs is the choice: an integer expectimax of depth D per lane, in registers -- for each
// of the four moves, slide, and at D >= 1 put a 2 and a 4 into every empty cell of the afterstate and recurse.  The
// four-action and empty-cell loops stay rolled, so the lanes of a wave walk them together and a lane whose board has
// fewer valid moves or empty cells idles for the others' iterations; the cost of a step is the wave's slowest lane.
// Termination: as scripted_kernel -- every live lane advances its episode by one step per iteration (the search is a
// bounded loop nest: at most 4 (2 N^2 4)^D moves) and gives it up by termination, truncation or suspension at `cap`.
// Roofline (an estimate from the loop nest; the measured rates are in DESIGN.md): integer VALU only; with E empty
// cells in an afterstate a depth-0 step is 4 moves, a depth-1 step 4 + 4 * (2 E * 4) moves, a depth-2 step
// 4 + 4 * (2 E * (4 + 4 * (2 E * 4))) -- each level multiplies the work by about 8 E -- against two stores and no loads
// per step: far from HBM, bound by VALU issue, and by instruction latency while the launch has few waves per SIMD.
// The wave-cooperative form (one episode's children spread over the lanes of a wave) is g2048_search_wave_kernel.h.
#pragma once
#include "g2048_scripted_kernel.h"
#include "g2048_search_core.h"

namespace {

static_assert(search::kMaxDepth == G2048_SEARCH_MAX_DEPTH && search::kMaxWeight == G2048_SEARCH_MAX_WEIGHT,
              "search limits");

// ScriptArgs first, so that args_per_lane() (the kernarg segment read as a ScriptArgs at offset 0) serves this kernel
struct SearchArgs {
    ScriptArgs s;       // s.script is not read
    search::Weights w;
};

// The search player of depth D for play_episodes: the policy stream is neither read nor written.
template <class G, int D>
struct SearchPlayer {
    const SearchArgs& a;
    __device__ __forceinline__ bool policy_stream() const { return false; }
    __device__ __forceinline__ bool step(scripted::Episode<G>& e, scripted::Row<G>& row) const {
        return search::episode_step<G, D>(e, a.w, a.s.rc, a.s.max_steps, row);
    }
};

// scripted_kernel's loop (play_episodes) with the search player of depth D
template <class G, int D, bool TRAJ>
__global__ void __launch_bounds__(kScriptBlock) search_kernel(SearchArgs a) {
    play_episodes<G, TRAJ>(SearchPlayer<G, D>{a});
}

// One board per thread: boards are [W, n] planes of stride n (W = 1: n bitboards); q may be NULL.
template <class G, int D>
__global__ void __launch_bounds__(kScriptBlock) search_choose_kernel(search::Weights w, const uint64_t* boards,
                                                                     uint32_t n, uint8_t* actions, int64_t* q) {
    const uint32_t i = blockIdx.x * (uint32_t)kScriptBlock + threadIdx.x;
    if (i >= n) return;
    uint64_t b[G::kWords];
#pragma unroll
    for (int k = 0; k < G::kWords; k++) b[k] = boards[(size_t)k * n + i];
    int64_t qv[4];
    actions[i] = (uint8_t)search::choose<G, D>(b, w, qv);
    if (q) {
#pragma unroll
        for (int k = 0; k < 4; k++) q[4 * (size_t)i + k] = qv[k];
    }
}

// depth in 0..2 and every weight <= 4096
int search_player(const char* who, const g2048_search* sp, search::Weights& w) {
    const std::string p = std::string(who) + ": ";
    if (!sp) return sfail(G2048_EINVAL, p + "search is NULL");
    if (sp->depth < 0 || sp->depth > G2048_SEARCH_MAX_DEPTH)
        return sfail(G2048_EINVAL, p + "depth must be in 0..2 (got " + std::to_string(sp->depth) + ")");
    if (sp->w_merge > G2048_SEARCH_MAX_WEIGHT || sp->w_empty > G2048_SEARCH_MAX_WEIGHT ||
        sp->w_smooth > G2048_SEARCH_MAX_WEIGHT || sp->w_corner > G2048_SEARCH_MAX_WEIGHT)
        return sfail(G2048_EINVAL, p + "every weight must be in 0..4096");
    w = search::Weights{sp->w_merge, sp->w_empty, sp->w_smooth, sp->w_corner};
    return G2048_OK;
}

// The player's checks, then script_args' for everything the scripted entry points check besides the script: they run
// on a UNIFORM script, the kind that asks nothing of the config.
int search_args(const char* who, const g2048_search* sp, const g2048_env_cfg* cfg, uint64_t* env_state,
                const uint64_t* env_inc, uint64_t* env_buf, uint64_t* pol_state, const uint64_t* pol_inc,
                uint64_t* pol_buf, uint32_t* queue, const int32_t* order, int64_t n_order, int resume,
                const g2048_suspend* sus, int64_t n, int64_t cap, bool rows, const g2048_traj* traj, int64_t board_stride,
                const g2048_eval_out* out, int max_workgroups, SearchArgs& a) {
    const int rc = search_player(who, sp, a.w);
    if (rc) return rc;
    const g2048_script any = {G2048_SCRIPT_UNIFORM, {0, 1, 2, 3}};
    return script_args(who, &any, cfg, env_state, env_inc, env_buf, pol_state, pol_inc, pol_buf, queue, order, n_order,
                       resume, sus, n, cap, rows, traj, board_stride, out, max_workgroups, a.s);
}

template <class G, int D, bool TRAJ>
int launch_search_d(const SearchArgs& a, int max_workgroups, void* stream) {
    hipLaunchKernelGGL((search_kernel<G, D, TRAJ>), dim3(script_grid(a.s.n_order, max_workgroups)), dim3(kScriptBlock),
                       0, (hipStream_t)stream, a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? G2048_OK : sfail(G2048_EHIP, hipGetErrorString(e));
}

template <class G, bool TRAJ>
int launch_search(int depth, const SearchArgs& a, int max_workgroups, void* stream) {
    switch (depth) {
        case 0: return launch_search_d<G, 0, TRAJ>(a, max_workgroups, stream);
        case 1: return launch_search_d<G, 1, TRAJ>(a, max_workgroups, stream);
        default: return launch_search_d<G, 2, TRAJ>(a, max_workgroups, stream);
    }
}

template <class G, int D>
int launch_choose_d(const search::Weights& w, const uint64_t* boards, int64_t n, uint8_t* actions, int64_t* q,
                    void* stream) {
    hipLaunchKernelGGL((search_choose_kernel<G, D>), dim3((unsigned)((n + kScriptBlock - 1) / kScriptBlock)),
                       dim3(kScriptBlock), 0, (hipStream_t)stream, w, boards, (uint32_t)n, actions, q);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? G2048_OK : sfail(G2048_EHIP, hipGetErrorString(e));
}

template <class G>
int launch_choose(int depth, const search::Weights& w, const uint64_t* boards, int64_t n, uint8_t* actions, int64_t* q,
                  void* stream) {
    switch (depth) {
        case 0: return launch_choose_d<G, 0>(w, boards, n, actions, q, stream);
        case 1: return launch_choose_d<G, 1>(w, boards, n, actions, q, stream);
        default: return launch_choose_d<G, 2>(w, boards, n, actions, q, stream);
    }
}

// the checks of the two choose entry points, before any HIP call
int choose_args(const char* who, const g2048_search* sp, const uint64_t* boards, int64_t n, const uint8_t* actions,
                search::Weights& w) {
    const int rc = search_player(who, sp, w);
    if (rc) return rc;
    if (n < 0 || n > (int64_t)0x7FFFFFFF) return sfail(G2048_EINVAL, std::string(who) + ": n out of range");
    if (!boards || !actions) return sfail(G2048_EINVAL, std::string(who) + ": a required buffer is NULL");
    return G2048_OK;
}

}  // namespace
