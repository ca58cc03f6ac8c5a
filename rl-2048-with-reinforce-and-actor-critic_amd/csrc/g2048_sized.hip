// g2048_sized.hip -- gfx950 kernels and C ABI for N x N boards, 2 <= N <= 8 (include/g2048.h "sized" entry points).
//
// The arithmetic is csrc/g2048_sized_core.h: W = ceil(N*N/16) words per board, line moves in plain ALU (no row
// table: one does not exist for lines of 5..8 cells, so these kernels need no g2048_init table and no LDS table).
// One lane per thread, 256 threads per workgroup.  Board buffers are plane-major -- word w of lane i at
// buf[w * plane_stride + i] -- so every plane access of a wave is one contiguous run of 8-byte words.
// Observations are written by the whole workgroup: each thread parks its final board in LDS, then the workgroup
// walks its contiguous obs region float4 by float4 (every store instruction covers 4 KiB of contiguous obs).
// Instantiation: N (and the RNG, for the step and reset kernels) are template parameters -- the trip counts and
// the cell -> word / nibble maps must be compile-time for the boards to stay in registers; the observation mode
// and the optional outputs are runtime branches (they guard stores, not arithmetic).  The 4 x 4 product path
// (g2048.hip) never calls into this file.
#include <hip/hip_runtime.h>

#include <string>

#include "g2048.h"
#include "g2048_sized_core.h"

using namespace g2048;
namespace sz = g2048::sized;

namespace g2048_internal {   // g2048.hip
int set_error(int code, const char* msg);
int check_env_cfg(const g2048_env_cfg* c);
g2048::RewardCfg reward_cfg_of(const g2048_env_cfg& c);
}  // namespace g2048_internal

namespace {

constexpr int kBlock = 256;

int sfail(int code, const std::string& msg) { return g2048_internal::set_error(code, msg.c_str()); }

#define G2048_SIZED_HIP(x)                                                                              \
    do {                                                                                                \
        hipError_t e_ = (x);                                                                            \
        if (e_ != hipSuccess) return sfail(G2048_EHIP, std::string(#x) + ": " + hipGetErrorString(e_)); \
    } while (0)

template <int N>
__device__ __forceinline__ sz::Board<N> load_board(const uint64_t* __restrict__ p, int64_t stride, int64_t i) {
    sz::Board<N> b;
#pragma unroll
    for (int w = 0; w < sz::Dim<N>::kWords; w++) b.w[w] = p[(int64_t)w * stride + i];
    return b;
}

template <int N>
__device__ __forceinline__ void store_board(uint64_t* __restrict__ p, int64_t stride, int64_t i, const sz::Board<N>& b) {
#pragma unroll
    for (int w = 0; w < sz::Dim<N>::kWords; w++) p[(int64_t)w * stride + i] = b.w[w];
}

__device__ __forceinline__ uint32_t mask_word(uint32_t m) {
    // int8[4] per board as one 32-bit word: byte a = bit a
    return (m & 1u) | ((m & 2u) << 7) | ((m & 4u) << 14) | ((m & 8u) << 21);
}

// ------------------------------------------------------------------------------------- observation writer
// The workgroup's boards (thread t = lane first + t; `wr` = this lane's obs is to be written) -> the obs rows
// [first, first + nb).  sb: [W][kBlock] board words, sf: [kBlock] write flags (LDS).  Every thread of the
// workgroup must call it (barrier).  MODE: G2048_OBS_RAW / LOG2 / ONEHOT (17 channels at (r*N+c)*17 + e).
template <int N, int MODE>
__device__ __forceinline__ void write_obs_mode(float* __restrict__ obs, int64_t first, uint32_t nb, float scale,
                                               const uint64_t* sb, const uint8_t* sf) {
    constexpr uint32_t OW = MODE == G2048_OBS_ONEHOT ? N * N * 17 : N * N;
    const uint32_t total = nb * OW;
    float* dst = obs + first * (int64_t)OW;   // first % 256 == 0: 16-byte aligned when obs is
    for (uint32_t q = threadIdx.x * 4u; q < total; q += kBlock * 4u) {
        float v[4];
        bool f[4];
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const uint32_t idx = q + t < total ? q + t : total - 1u;
            const uint32_t ln = idx / OW, within = idx - ln * OW;
            const uint32_t cell = MODE == G2048_OBS_ONEHOT ? within / 17u : within;
            const uint32_t e = (uint32_t)(sb[(cell >> 4) * kBlock + ln] >> (4u * (cell & 15u))) & 15u;
            if (MODE == G2048_OBS_ONEHOT) v[t] = e == within - cell * 17u ? 1.0f : 0.0f;
            else if (MODE == G2048_OBS_LOG2) v[t] = (float)e * scale;
            else v[t] = e ? (float)(1u << e) : 0.0f;
            f[t] = q + t < total && sf[ln] != 0;
        }
        if (f[0] && f[1] && f[2] && f[3]) {
            *reinterpret_cast<float4*>(dst + q) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int t = 0; t < 4; t++)
                if (f[t]) dst[q + t] = v[t];
        }
    }
}

template <int N>
__device__ __forceinline__ void write_obs_block(float* __restrict__ obs, int obs_mode, int64_t first, int64_t n,
                                                float scale, const sz::Board<N>& b, bool wr, uint64_t* sb,
                                                uint8_t* sf) {
#pragma unroll
    for (int w = 0; w < sz::Dim<N>::kWords; w++) sb[w * kBlock + threadIdx.x] = b.w[w];
    sf[threadIdx.x] = wr ? 1 : 0;
    __syncthreads();
    const uint32_t nb = (uint32_t)(n - first < kBlock ? n - first : kBlock);
    if (obs_mode == G2048_OBS_ONEHOT) write_obs_mode<N, G2048_OBS_ONEHOT>(obs, first, nb, scale, sb, sf);
    else if (obs_mode == G2048_OBS_LOG2) write_obs_mode<N, G2048_OBS_LOG2>(obs, first, nb, scale, sb, sf);
    else write_obs_mode<N, G2048_OBS_RAW>(obs, first, nb, scale, sb, sf);
}

// ------------------------------------------------------------------------------------- RNG state
__device__ __forceinline__ Pcg64 load_pcg(const g2048_lanes& L, int64_t i, uint32_t st) {
    Pcg64 g;
    const ulonglong2 s = reinterpret_cast<const ulonglong2*>(L.rng_state)[i];
    const ulonglong2 c = reinterpret_cast<const ulonglong2*>(L.rng_inc)[i];
    g.s_lo = s.x;
    g.s_hi = s.y;
    g.i_lo = c.x;
    g.i_hi = c.y;
    g.has_uint32 = (st & G2048_LS_HAS_U32) ? 1u : 0u;
    g.uinteger = L.rng_uint[i];
    return g;
}

__device__ __forceinline__ void store_pcg(const g2048_lanes& L, int64_t i, const Pcg64& g, bool with_inc) {
    reinterpret_cast<ulonglong2*>(L.rng_state)[i] = make_ulonglong2(g.s_lo, g.s_hi);
    if (with_inc) reinterpret_cast<ulonglong2*>(L.rng_inc)[i] = make_ulonglong2(g.i_lo, g.i_hi);
    L.rng_uint[i] = g.uinteger;
}

// a fresh episode's state word: step 0, max_tile_seen 4 (src/env.py:183), active, the PCG64 buffer flag
__device__ __forceinline__ uint32_t fresh_state(const Pcg64& g) {
    return (2u << G2048_LS_MAXT_SHIFT) | G2048_LS_ACTIVE | (g.has_uint32 ? G2048_LS_HAS_U32 : 0u);
}

// ------------------------------------------------------------------------------------- step
struct SizedStepArgs {
    g2048_lanes L;
    int64_t bstride;
    const uint8_t* actions;
    g2048_sized_step_out out;
    RewardCfg rc;
    float obs_scale;
    int obs_mode;    // G2048_OBS_NONE when out.obs is NULL
    int auto_reset;
    int64_t max_steps;
    uint64_t stride, key;
    int64_t n;
};

// Game2048Env.step (src/env.py:264-302) of every lane, with everything step_kernel does for 4 x 4 boards: inactive
// and bad-action lanes are reported and left untouched; an episode that ends is auto-reset in place (seed +=
// stride) when asked.
template <int N, int RNG>
__global__ void __launch_bounds__(kBlock, 4) sized_step_kernel(SizedStepArgs a) {
    constexpr int W = sz::Dim<N>::kWords, LEN = sz::Dim<N>::kListLen;
    __shared__ uint64_t sb[W * kBlock];
    __shared__ uint8_t sf[kBlock];
    const g2048_lanes& L = a.L;
    const int64_t first = (int64_t)blockIdx.x * kBlock;
    const int64_t i = first + threadIdx.x;
    sz::Board<N> b;
#pragma unroll
    for (int w = 0; w < W; w++) b.w[w] = 0ull;
    bool wobs = false;
    if (i < a.n) {
        b = load_board<N>(L.board, a.bstride, i);
        const uint32_t st = L.state[i];
        const uint32_t act = a.actions[i];
        if (a.out.prev_board) store_board<N>(a.out.prev_board, a.out.prev_stride, i, b);
        uint8_t* list = a.out.merged ? a.out.merged + i * LEN : nullptr;
        if (!(st & G2048_LS_ACTIVE) || act > 3u) {
            a.out.reward[i] = 0.0f;
            if (a.out.reward64) a.out.reward64[i] = 0.0;
            a.out.flags[i] = (uint8_t)((st & G2048_LS_ACTIVE) ? G2048_F_BADACTION : G2048_F_INACTIVE);
            if (list)
                for (int k = 0; k < LEN; k++) list[k] = 0;
            if (a.out.score_add) a.out.score_add[i] = 0u;
        } else {
            const uint32_t sc0 = st & G2048_LS_STEP_MASK;
            const uint32_t sc = sc0 + (sc0 < G2048_LS_STEP_MASK ? 1u : 0u);   // saturating 20-bit step count
            uint32_t mt = (st >> G2048_LS_MAXT_SHIFT) & 31u;
            Pcg64 g;
            g.has_uint32 = 0u;
            uint64_t seed = 0;
            if constexpr (RNG == G2048_RNG_PCG64) g = load_pcg(L, i, st);
            else seed = L.seed[i];
            sz::StepValues<N> o;
            if (list) o = sz::env_step<N, RNG, true>(b, act, sc, mt, g, a.key, seed, a.rc, a.max_steps, list);
            else o = sz::env_step<N, RNG, false>(b, act, sc, mt, g, a.key, seed, a.rc, a.max_steps, nullptr);
            const bool ended = (o.flags & (G2048_F_TERMINATED | G2048_F_TRUNCATED)) != 0u;
            const bool reset = ended && a.auto_reset;
            a.out.reward[i] = (float)o.reward;
            if (a.out.reward64) a.out.reward64[i] = o.reward;
            if (a.out.score_add) a.out.score_add[i] = o.score_add;
            a.out.flags[i] = (uint8_t)(o.flags | (reset ? G2048_F_RESET : 0u));
            b = o.board;
            uint32_t mbits = o.mask;
            uint32_t nst = sc | (mt << G2048_LS_MAXT_SHIFT) | (ended ? 0u : G2048_LS_ACTIVE) |
                           (g.has_uint32 ? G2048_LS_HAS_U32 : 0u);
            if (reset) {   // Game2048Env.reset with seed = previous seed + stride
                if constexpr (RNG == G2048_RNG_PCG64) seed = L.seed[i];
                seed += a.stride;
                g.has_uint32 = 0u;
                b = sz::fresh_board<N, RNG>(seed, a.key, g);
                L.seed[i] = seed;
                nst = fresh_state(g);
                mbits = sz::action_mask<N>(b);
            }
            store_board<N>(L.board, a.bstride, i, b);
            L.state[i] = nst;
            if constexpr (RNG == G2048_RNG_PCG64) store_pcg(L, i, g, reset);
            if (a.out.mask) reinterpret_cast<uint32_t*>(a.out.mask)[i] = mask_word(mbits);
            if (a.out.mask_bits) a.out.mask_bits[i] = (uint8_t)mbits;
            wobs = true;
        }
    }
    if (a.obs_mode != G2048_OBS_NONE)   // kernel-uniform
        write_obs_block<N>(a.out.obs, a.obs_mode, first, a.n, a.obs_scale, b, wobs, sb, sf);
}

// ------------------------------------------------------------------------------------- reset / obs / move / sym
struct SizedResetArgs {
    g2048_lanes L;
    int64_t bstride;
    const uint64_t* seeds;
    const uint8_t* reset_mask;
    int8_t* mask_out;
    float* obs_out;
    float obs_scale;
    int obs_mode;
    uint64_t key;
    int64_t n;
};

template <int N, int RNG>
__global__ void __launch_bounds__(kBlock) sized_reset_kernel(SizedResetArgs a) {
    constexpr int W = sz::Dim<N>::kWords;
    __shared__ uint64_t sb[W * kBlock];
    __shared__ uint8_t sf[kBlock];
    const int64_t first = (int64_t)blockIdx.x * kBlock;
    const int64_t i = first + threadIdx.x;
    sz::Board<N> b;
#pragma unroll
    for (int w = 0; w < W; w++) b.w[w] = 0ull;
    bool wr = false;
    if (i < a.n && (!a.reset_mask || a.reset_mask[i])) {
        const uint64_t seed = a.seeds ? a.seeds[i] : a.L.seed[i];
        Pcg64 g;
        g.has_uint32 = 0u;
        b = sz::fresh_board<N, RNG>(seed, a.key, g);
        a.L.seed[i] = seed;
        store_board<N>(a.L.board, a.bstride, i, b);
        a.L.state[i] = fresh_state(g);
        if constexpr (RNG == G2048_RNG_PCG64) store_pcg(a.L, i, g, true);
        if (a.mask_out) reinterpret_cast<uint32_t*>(a.mask_out)[i] = mask_word(sz::action_mask<N>(b));
        wr = true;
    }
    if (a.obs_mode != G2048_OBS_NONE)
        write_obs_block<N>(a.obs_out, a.obs_mode, first, a.n, a.obs_scale, b, wr, sb, sf);
}

template <int N>
__global__ void __launch_bounds__(kBlock) sized_obs_kernel(const uint64_t* __restrict__ boards, int64_t stride,
                                                           int obs_mode, float scale, float* obs, int8_t* mask,
                                                           int64_t n) {
    constexpr int W = sz::Dim<N>::kWords;
    __shared__ uint64_t sb[W * kBlock];
    __shared__ uint8_t sf[kBlock];
    const int64_t first = (int64_t)blockIdx.x * kBlock;
    const int64_t i = first + threadIdx.x;
    sz::Board<N> b;
#pragma unroll
    for (int w = 0; w < W; w++) b.w[w] = 0ull;
    if (i < n) {
        b = load_board<N>(boards, stride, i);
        if (mask) reinterpret_cast<uint32_t*>(mask)[i] = mask_word(sz::action_mask<N>(b));
    }
    if (obs_mode != G2048_OBS_NONE) write_obs_block<N>(obs, obs_mode, first, n, scale, b, i < n, sb, sf);
}

// pre-spawn move only: Game2048._move (src/game2048.py:158-165) for known-answer tests
template <int N>
__global__ void __launch_bounds__(kBlock, 4) sized_move_kernel(const uint64_t* __restrict__ boards, int64_t stride,
                                                            const uint8_t* __restrict__ actions, uint64_t* out,
                                                            int64_t out_stride, uint8_t* merged, uint8_t* flags,
                                                            int64_t n) {
    constexpr int LEN = sz::Dim<N>::kListLen;
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const sz::Board<N> b = load_board<N>(boards, stride, i);
    const uint32_t act = actions[i];
    if (act > 3u) {
        store_board<N>(out, out_stride, i, b);
        if (merged)
            for (int k = 0; k < LEN; k++) merged[i * LEN + k] = 0;
        if (flags) flags[i] = (uint8_t)G2048_F_BADACTION;
        return;
    }
    MoveSummary s;
    sz::Board<N> m;
    if (merged) m = sz::board_move<N, true>(b, act, s, merged + i * LEN);
    else m = sz::board_move<N, false>(b, act, s, nullptr);
    store_board<N>(out, out_stride, i, m);
    if (flags)
        flags[i] = (uint8_t)((sz::board_eq<N>(m, b) ? 0u : G2048_F_CHANGED) | (s.overflow ? G2048_F_OVERFLOW : 0u));
}

template <int N>
__global__ void __launch_bounds__(kBlock) sized_sym_kernel(const uint64_t* __restrict__ boards, int64_t stride,
                                                           const uint8_t* __restrict__ act, uint64_t* ob,
                                                           int64_t out_stride, uint8_t* oa, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const sz::Board<N> x = load_board<N>(boards, stride, i);
    const uint32_t a = act ? act[i] : 0u;
    sz::symmetry_chain<N>(x, [&](int k, const sz::Board<N>& y) {
        store_board<N>(ob, out_stride, (int64_t)k * n + i, y);
        if (act && oa) oa[(int64_t)k * n + i] = (uint8_t)symmetry_action(a, k);
    });
}

// ------------------------------------------------------------------------------------- host helpers
int check_size(int size) {
    if (size < 2 || size > 8) return sfail(G2048_EINVAL, "size must be in 2..8 (got " + std::to_string(size) + ")");
    return G2048_OK;
}

int check_n_stride(int64_t n, int64_t stride, int64_t need, const char* what) {
    if (n < 0) return sfail(G2048_EINVAL, "n < 0");
    if (n > (int64_t(1) << 30)) return sfail(G2048_EINVAL, "n must be <= 2^30 per call");
    if (stride < need)
        return sfail(G2048_EINVAL, std::string(what) + " plane_stride " + std::to_string(stride) + " < " +
                                       std::to_string(need) + " lanes per plane");
    return G2048_OK;
}

int check_lanes(const g2048_lanes* L, int rng_mode) {
    if (rng_mode != G2048_RNG_PCG64 && rng_mode != G2048_RNG_PHILOX)
        return sfail(G2048_EINVAL, "Unsupported rng_mode: " + std::to_string(rng_mode));
    if (!L || !L->board || !L->state || !L->seed) return sfail(G2048_EINVAL, "lanes: a required buffer is NULL");
    if (rng_mode == G2048_RNG_PCG64 && (!L->rng_state || !L->rng_inc || !L->rng_uint))
        return sfail(G2048_EINVAL, "lanes: PCG64 mode needs rng_state / rng_inc / rng_uint");
    return G2048_OK;
}

int check_obs_ptr(const float* obs) {
    if (obs && (reinterpret_cast<uintptr_t>(obs) & 15u)) return sfail(G2048_EINVAL, "obs must be 16-byte aligned");
    return G2048_OK;
}

inline dim3 grid_of(int64_t n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }

#define G2048_SIZED_SWITCH(size, CALL) \
    switch (size) {                    \
        case 2: CALL(2); break;        \
        case 3: CALL(3); break;        \
        case 4: CALL(4); break;        \
        case 5: CALL(5); break;        \
        case 6: CALL(6); break;        \
        case 7: CALL(7); break;        \
        default: CALL(8); break;       \
    }

}  // namespace

extern "C" {

int g2048_sized_words(int size) { return size < 2 || size > 8 ? -1 : (size * size + 15) / 16; }

int g2048_sized_reset(int size, const g2048_lanes* lanes, int64_t plane_stride, const uint64_t* seeds,
                      const uint8_t* reset_mask, const g2048_env_cfg* cfg, int rng_mode, uint64_t philox_key,
                      int8_t* mask_out, float* obs_out, int64_t n, void* stream) {
    int rc = check_size(size);
    if (!rc) rc = g2048_internal::check_env_cfg(cfg);
    if (!rc) rc = check_lanes(lanes, rng_mode);
    if (!rc) rc = check_n_stride(n, plane_stride, n, "board");
    if (!rc) rc = check_obs_ptr(obs_out);
    if (rc) return rc;
    if (n == 0) return G2048_OK;
    SizedResetArgs a{*lanes, plane_stride, seeds, reset_mask, mask_out, obs_out, cfg->obs_log2_scale,
                     obs_out ? cfg->obs_mode : G2048_OBS_NONE, philox_key, n};
    hipStream_t s = (hipStream_t)stream;
#define CALL(NN)                                                                                                     \
    if (rng_mode == G2048_RNG_PCG64)                                                                                 \
        hipLaunchKernelGGL((sized_reset_kernel<NN, G2048_RNG_PCG64>), grid_of(n), dim3(kBlock), 0, s, a);            \
    else                                                                                                             \
        hipLaunchKernelGGL((sized_reset_kernel<NN, G2048_RNG_PHILOX>), grid_of(n), dim3(kBlock), 0, s, a)
    G2048_SIZED_SWITCH(size, CALL)
#undef CALL
    G2048_SIZED_HIP(hipGetLastError());
    return G2048_OK;
}

int g2048_sized_step(int size, const g2048_lanes* lanes, int64_t plane_stride, const uint8_t* actions,
                     const g2048_env_cfg* cfg, const g2048_sized_step_out* out, int rng_mode, uint64_t philox_key,
                     int auto_reset, uint64_t reset_stride, int64_t n, void* stream) {
    int rc = check_size(size);
    if (!rc) rc = g2048_internal::check_env_cfg(cfg);
    if (!rc) rc = check_lanes(lanes, rng_mode);
    if (!rc) rc = check_n_stride(n, plane_stride, n, "board");
    if (rc) return rc;
    if (!actions) return sfail(G2048_EINVAL, "actions is NULL");
    if (!out || !out->reward || !out->flags) return sfail(G2048_EINVAL, "out.reward / out.flags are required");
    if (out->prev_board && (rc = check_n_stride(n, out->prev_stride, n, "prev_board"))) return rc;
    if ((rc = check_obs_ptr(out->obs))) return rc;
    if (rng_mode == G2048_RNG_PHILOX && cfg->max_steps < 0)
        return sfail(G2048_EINVAL, "Philox mode needs a finite max_steps: its draw counter is the 20-bit lane step count");
    if (n == 0) return G2048_OK;
    SizedStepArgs a;
    a.L = *lanes;
    a.bstride = plane_stride;
    a.actions = actions;
    a.out = *out;
    a.rc = g2048_internal::reward_cfg_of(*cfg);
    a.obs_scale = cfg->obs_log2_scale;
    a.obs_mode = out->obs ? cfg->obs_mode : G2048_OBS_NONE;
    a.auto_reset = auto_reset;
    a.max_steps = cfg->max_steps;
    a.stride = reset_stride;
    a.key = philox_key;
    a.n = n;
    hipStream_t s = (hipStream_t)stream;
#define CALL(NN)                                                                                                    \
    if (rng_mode == G2048_RNG_PCG64)                                                                                \
        hipLaunchKernelGGL((sized_step_kernel<NN, G2048_RNG_PCG64>), grid_of(n), dim3(kBlock), 0, s, a);            \
    else                                                                                                            \
        hipLaunchKernelGGL((sized_step_kernel<NN, G2048_RNG_PHILOX>), grid_of(n), dim3(kBlock), 0, s, a)
    G2048_SIZED_SWITCH(size, CALL)
#undef CALL
    G2048_SIZED_HIP(hipGetLastError());
    return G2048_OK;
}

int g2048_sized_obs(int size, const uint64_t* boards, int64_t plane_stride, int obs_mode, float obs_log2_scale,
                    float* obs, int8_t* mask, int64_t n, void* stream) {
    int rc = check_size(size);
    if (!rc) rc = check_n_stride(n, plane_stride, n, "board");
    if (!rc) rc = check_obs_ptr(obs);
    if (rc) return rc;
    if (!boards) return sfail(G2048_EINVAL, "boards is NULL");
    if (obs_mode < G2048_OBS_NONE || obs_mode > G2048_OBS_ONEHOT)
        return sfail(G2048_EINVAL, "Unsupported obs_mode: " + std::to_string(obs_mode));
    if (n == 0) return G2048_OK;
    const int mode = obs ? obs_mode : G2048_OBS_NONE;
    hipStream_t s = (hipStream_t)stream;
#define CALL(NN)                                                                                                 \
    hipLaunchKernelGGL((sized_obs_kernel<NN>), grid_of(n), dim3(kBlock), 0, s, boards, plane_stride, mode,       \
                       obs_log2_scale, obs, mask, n)
    G2048_SIZED_SWITCH(size, CALL)
#undef CALL
    G2048_SIZED_HIP(hipGetLastError());
    return G2048_OK;
}

int g2048_sized_move(int size, const uint64_t* boards, int64_t plane_stride, const uint8_t* actions,
                     uint64_t* out_board, int64_t out_stride, uint8_t* merged, uint8_t* flags, int64_t n,
                     void* stream) {
    int rc = check_size(size);
    if (!rc) rc = check_n_stride(n, plane_stride, n, "board");
    if (!rc) rc = check_n_stride(n, out_stride, n, "out_board");
    if (rc) return rc;
    if (!boards || !actions || !out_board) return sfail(G2048_EINVAL, "NULL buffer");
    if (n == 0) return G2048_OK;
    hipStream_t s = (hipStream_t)stream;
#define CALL(NN)                                                                                                  \
    hipLaunchKernelGGL((sized_move_kernel<NN>), grid_of(n), dim3(kBlock), 0, s, boards, plane_stride, actions,    \
                       out_board, out_stride, merged, flags, n)
    G2048_SIZED_SWITCH(size, CALL)
#undef CALL
    G2048_SIZED_HIP(hipGetLastError());
    return G2048_OK;
}

int g2048_sized_symmetries(int size, const uint64_t* boards, int64_t plane_stride, const uint8_t* actions,
                           uint64_t* out_boards, int64_t out_stride, uint8_t* out_actions, int64_t n, void* stream) {
    int rc = check_size(size);
    if (!rc) rc = check_n_stride(n, plane_stride, n, "board");
    if (!rc && n > (int64_t(1) << 27)) rc = sfail(G2048_EINVAL, "n must be <= 2^27 per call");
    if (!rc) rc = check_n_stride(n, out_stride, 8 * n, "out_boards");
    if (rc) return rc;
    if (!boards || !out_boards) return sfail(G2048_EINVAL, "NULL buffer");
    if (n == 0) return G2048_OK;
    hipStream_t s = (hipStream_t)stream;
#define CALL(NN)                                                                                                  \
    hipLaunchKernelGGL((sized_sym_kernel<NN>), grid_of(n), dim3(kBlock), 0, s, boards, plane_stride, actions,     \
                       out_boards, out_stride, out_actions, n)
    G2048_SIZED_SWITCH(size, CALL)
#undef CALL
    G2048_SIZED_HIP(hipGetLastError());
    return G2048_OK;
}

}  // extern "C"
