// g2048_policy_roll.h -- the two-layer family's persistent rollout kernel (rollout_kernel), its launch helpers and the
// pieces of g2048_policy.hip it is built from (packed layout, NetSmem, activation, obs and mask helpers), shared by the
// two translation units that instantiate it: g2048_policy.hip (TRAJ = true: g2048_rollout, 64 kernels) and
// g2048_rollout_eval.hip (TRAJ = false: the score-only g2048_rollout_eval, 64 more), so that the two sets compile side
// by side.  The net, its packed layout and the forward are described at the top of g2048_policy.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "g2048.h"
#include "g2048_core.h"

using namespace g2048;

namespace {

typedef float floatx16 __attribute__((ext_vector_type(16)));

#ifndef G2048_DIAG
#define G2048_DIAG 0
#endif
#if G2048_DIAG
// diag build only: per-workgroup sums of rollout phase durations (s_memrealtime ticks): layer 1 + barrier,
// layer 2 + barrier, logits + choice + env step, claims; [4] = steps.  The trajectory form only: the read-out
// (g2048_diag_rollout_phases) is in g2048_policy.hip and reads that unit's copy, so the score-only form takes no
// stamps (ROLL_PH compiles to nothing for TRAJ = false) rather than stamps nobody can read.
constexpr int kRollDiagBlocks = 4096;
__device__ unsigned long long g_roll_ph[kRollDiagBlocks * 5];
#endif

constexpr int kPolBlock = 256;   // 4 waves; two workgroups per CU (2 waves per SIMD)

// packed layout (floats), nt1 / nt2 = hidden tiles of 32:
//   w1f [nt1][8][64]         lane l of k-step s: W1[2s + (l>>5)][32t + (l&31)]
//   b1p [nt1][2][16]         half h, register r: b1[32t + row(r, h)]
//   w2f [nt2][nt1][4][64][4] lane l, k-step (t, r = 4q + u) at [o][t][q][l][u]: W2[32t + row(r, l>>5)][32o + (l&31)]
//                            (one 16-B load per lane fetches four consecutive k-steps)
//   b2p [nt2][2][16]
//   w3p [nt2][2][16][4]      W3[32o + row(r, h)][a]
//   b3  [4]
// row(r, h) = (r & 3) + 8 (r >> 2) + 4 h: the hidden unit held by accumulator register r in lane half h.
__host__ __device__ inline int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

struct PolLayout {
    int64_t w1f, b1p, w2f, b2p, w3p, b3, total;
};

__host__ __device__ constexpr PolLayout pol_layout(int nt1, int nt2) {
    PolLayout L{};
    L.w1f = 0;
    L.b1p = L.w1f + (int64_t)nt1 * 8 * 64;
    L.w2f = L.b1p + (int64_t)nt1 * 32;
    L.b2p = L.w2f + (int64_t)nt2 * nt1 * 16 * 64;
    L.w3p = L.b2p + (int64_t)nt2 * 32;
    L.b3 = L.w3p + (int64_t)nt2 * 32 * 4;
    L.total = L.b3 + 4;
    return L;
}

template <int ACT>
__device__ __forceinline__ float activate(float z) {
    if constexpr (ACT == 0) return fmaxf(z, 0.0f);
    else return 1.0f / (1.0f + expf(-z));
}

template <int OBS>
__device__ __forceinline__ float obs_value(uint64_t b, int cell, float scale) {
    const uint32_t e = (uint32_t)(b >> (4 * cell)) & 15u;
    if constexpr (OBS == G2048_OBS_LOG2) return (float)e * scale;
    else return e ? (float)(1u << e) : 0.0f;
}

// Small tensors of the packed net staged in LDS (layer-1 fragments, biases, layer 3: <= 22.5 KB); the
// layer-2 fragments (the bulk, up to 256 KB) stay in L2 and are streamed by mlp_logits.
template <int NT1, int NT2>
struct NetSmem {
    static constexpr PolLayout L = pol_layout(NT1, NT2);
    static constexpr int kFloats = (int)(L.w2f - L.w1f) + (int)(L.total - L.b2p);
    float v[kFloats];
    __device__ void load(const float* net) {   // whole workgroup; caller syncs
        for (int k = threadIdx.x; k < kFloats; k += blockDim.x) v[k] = k < (int)L.w2f ? net[k] : net[L.b2p + (k - (int)L.w2f)];
    }
    __device__ const float* w1f() const { return v; }
    __device__ const float* b1p() const { return v + L.b1p; }
    __device__ const float* b2p() const { return v + L.w2f; }
    __device__ const float* w3p() const { return v + L.w2f + (L.w3p - L.b2p); }
    __device__ const float* b3() const { return v + L.w2f + (L.b3 - L.b2p); }
};

__device__ __forceinline__ uint32_t mask_word_of(uint64_t b) {
    const uint32_t m = action_mask(b);   // int8[4] as one word: byte a = bit a
    return (m & 1u) | ((m & 2u) << 7) | ((m & 4u) << 14) | ((m & 8u) << 21);
}

// ---------------------------------------------------------------------------------------------------- rollout
// The whole batched rollout (ReinforceAgent.run_episode, src/reinforce_agent.py:195-252, for n (env_seed,
// policy_seed) pairs) in one persistent launch: each wave runs 32 episode slots; per step the MLP above picks
// every slot's action (Generator.choice on the slot's policy stream, or greedy), Game2048Env.step runs in
// registers (env_step_pcg, row tables read through L1/L2), and the step's trajectory row is written.  A slot
// whose episode ends writes the episode's results and takes the next episode from a.next (one atomic per
// episode), so no work is spent on finished episodes and there is no per-step host round trip.  Both lane halves
// carry every slot (the MFMA layout); the lower half writes.
struct RolloutArgs {
    const float* net;
    const uint8_t* tab;
    RewardCfg rc;
    int64_t max_steps;
    float obs_scale;
    int use_mask, greedy;
    const uint64_t *env_rs, *env_inc, *env_buf;   // default_rng(env_seed) per episode (g2048_seed_pcg64)
    const uint64_t *pol_rs, *pol_inc, *pol_buf;   // default_rng(policy_seed) per episode
    uint32_t* next;                               // episode queue (zero before the launch)
    uint64_t* boards;                             // [cap, n] time-major trajectory rows
    uint8_t* actions;
    double* rewards;                              // fp64: the Python float run_episode records
    uint8_t* flags;
    float* probs;                                 // [cap, n, 4] or NULL
    int32_t* lengths;                             // per episode
    double* totals;
    uint8_t* max_tile;
    uint64_t* final_board;
    uint32_t n, cap;
};

__device__ __forceinline__ Pcg64 load_stream(const uint64_t* rs, const uint64_t* inc, const uint64_t* buf, uint32_t e) {
    Pcg64 g;
    const ulonglong2 s = reinterpret_cast<const ulonglong2*>(rs)[e];
    const ulonglong2 c = reinterpret_cast<const ulonglong2*>(inc)[e];
    const uint64_t bf = buf[e];
    g.s_lo = s.x;
    g.s_hi = s.y;
    g.i_lo = c.x;
    g.i_hi = c.y;
    g.has_uint32 = (uint32_t)(bf >> 32);
    g.uinteger = (uint32_t)bf;
    return g;
}

struct GLine {
    const uint16_t* p;
    __device__ uint32_t operator()(uint32_t o) const { return p[o]; }
};
struct GCode {
    const uint8_t* p;
    __device__ uint32_t operator()(uint32_t o) const { return (p[o >> 1] >> ((o & 1u) << 2)) & 15u; }
};

// LDS of one rollout workgroup: the small net tensors, the layer-1 activations of the current step in
// layer-2 B-fragment order, the per-wave partial logits and the episode-claim broadcast.
template <int NT1, int NT2>
struct RollSmem {
    NetSmem<NT1, NT2> net;
    float4 h1f[NT1][4][64];      // [k-tile t][r / 4][lane]: registers 4q..4q+3 of layer-1 tile t
    float part[4][32][4];        // [wave][slot][action]
    uint32_t claim[32];
};

// One workgroup = 32 episode slots, TWO workgroups per CU; its 4 waves split every step's MLP: wave w computes the
// layer-1 tiles and the layer-2 output tiles congruent to w mod 4 (a quarter of the MFMAs), exchanging the layer-1
// activations and the partial logits through LDS (two barriers per step), so a step takes about a quarter of the
// one-wave latency.  Each wave streams its quarter of the layer-2 weight fragments from L2 every step (the next k-tile
// in flight; the first issued before layer 1), which leaves the registers for a second workgroup per CU: the
// two workgroups' steps interleave on every SIMD, so one's MFMAs run while the other's env step, layer 1 and
// barriers do (one workgroup per CU with the weights resident in registers left the MFMAs idle for those phases).
// Every wave holds the same logits and runs the same choice and env step on the same slot state (so no per-slot
// state is broadcast); wave 0 writes the trajectory and claims episodes for the workgroup.
constexpr int kRollBlocksPerCU = 2;

// TRAJ = false (g2048_rollout_eval): the score-only form -- the same code without the trajectory row (its stores and the
// row index), so the same episodes; the row pointers of RolloutArgs stay NULL and cap is max(max_steps, 1).
template <int NT1, int NT2, int ACT, int OBS, bool TRAJ>
__global__ void __launch_bounds__(kPolBlock, kRollBlocksPerCU) rollout_kernel(RolloutArgs a) {
    const int lane = threadIdx.x & 63, h = lane >> 5, col = lane & 31, w = threadIdx.x >> 6;
    __shared__ RollSmem<NT1, NT2> S;
    S.net.load(a.net);
    const GLine lut{reinterpret_cast<const uint16_t*>(a.tab)};
    const GCode code{a.tab + 2 * 65536};
    // this wave's layer-2 fragment stream: output tiles o = w + 4 k2 (those < NT2), k-tiles tt; stream index
    // i = k2 * NT1 + tt; the index past the end re-reads the first k-tile (unused)
    constexpr int kOwn = (NT2 + 3) / 4;
    // Loads through a buffer resource: this lane's voffset (lane * 16) plus a scalar k-tile offset -- 64-bit
    // per-fragment addresses were hoisted out of the step loop (128 registers) and spilled.
    const int ws = __builtin_amdgcn_readfirstlane(w);
    const int nown = (NT2 - ws + 3) / 4;                  // own output tiles (0 when w >= NT2)
    const int nkt = nown * NT1;
    const __amdgpu_buffer_rsrc_t rw2 = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(a.net + NetSmem<NT1, NT2>::L.w2f), 0, NT2 * NT1 * 1024 * 4, 0x00020000);
    const uint32_t fvo = (uint32_t)lane * 16u;
    const auto frag = [&](int i, float4 f[4]) {
        const int ii = i < nkt ? i : 0;
        const int o = ws + 4 * (ii / NT1), tt = ii % NT1;
        const uint32_t base = __builtin_amdgcn_readfirstlane((uint32_t)(((o < NT2 ? o : 0) * NT1 + tt) * 4096));
        typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rw2, (int)fvo, (int)(base + 1024u * q), 0);
            f[q] = make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
        }
    };
    // episode claims for the slots that need one (identical `need` in all waves): wave 0 takes them with one
    // atomic and publishes them; every wave must call this together (it contains barriers)
    const auto claim = [&](bool need, uint32_t cur) -> uint32_t {
        if (w == 0) {
            const uint64_t bal = __ballot(need && h == 0);
            uint32_t base = 0;
            if (bal) {
                const int leader = __builtin_ctzll(bal);
                if (lane == leader) base = atomicAdd(a.next, (uint32_t)__popcll(bal));
                base = (uint32_t)__shfl((int)base, leader, 64);
            }
            const uint32_t rank =
                __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
            if (h == 0) S.claim[col] = need ? base + rank : cur;
        }
        __syncthreads();
        const uint32_t v = S.claim[col];
        __syncthreads();
        return v;
    };
    uint32_t ep = claim(true, 0u);
    bool drained = __ballot(ep >= a.n) != 0ull;           // block-uniform: the queue is empty (claims only grow)
    uint32_t t = 0, sc = 0, mt = 2;
    uint64_t b = 0;
    double total = 0.0;
    Pcg64 ge{}, gp{};
    const auto start = [&]() {
        if (ep < a.n) {
            ge = load_stream(a.env_rs, a.env_inc, a.env_buf, ep);
            gp = load_stream(a.pol_rs, a.pol_inc, a.pol_buf, ep);
            b = spawn_pcg(spawn_pcg(0ull, ge), ge);       // Game2048.reset (src/game2048.py:26-34)
            t = 0;
            sc = 0;
            mt = 2;                                       // max_tile_seen = 4 (src/env.py:188)
            total = 0.0;
        }
    };
    start();
#if G2048_DIAG
    unsigned long long ph[5] = {0, 0, 0, 0, 0};
    unsigned long long tp = __builtin_amdgcn_s_memrealtime();
#define ROLL_PH(k)                                                            \
    do {                                                                      \
        if constexpr (TRAJ) {                                                 \
            const unsigned long long tn = __builtin_amdgcn_s_memrealtime();  \
            ph[k] += tn - tp;                                                 \
            tp = tn;                                                          \
        }                                                                     \
    } while (0)
#else
#define ROLL_PH(k) \
    do {           \
    } while (0)
#endif
    while (__ballot(ep < a.n)) {                         // block-uniform (all waves hold the same slot state)
        float4 fa[4];                                     // layer-2 k-tile 0, in flight through layer 1
        frag(0, fa);
        // ---- layer 1: this wave's tiles -> LDS
        float x[8];
#pragma unroll
        for (int s2 = 0; s2 < 8; s2++) x[s2] = obs_value<OBS>(b, 2 * s2 + h, a.obs_scale);
        const float* w1f = S.net.w1f();
#pragma unroll
        for (int tt = 0; tt < NT1; tt++) {
            if ((tt & 3) != w) continue;
            floatx16 acc = {};
#pragma unroll
            for (int s2 = 0; s2 < 8; s2++)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w1f[(tt * 8 + s2) * 64 + lane], x[s2], acc, 0, 0, 0);
            const float4* bb = reinterpret_cast<const float4*>(S.net.b1p() + (tt * 2 + h) * 16);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const float4 bv = bb[q];
                S.h1f[tt][q][lane] = make_float4(activate<ACT>(acc[4 * q + 0] + bv.x), activate<ACT>(acc[4 * q + 1] + bv.y),
                                                 activate<ACT>(acc[4 * q + 2] + bv.z), activate<ACT>(acc[4 * q + 3] + bv.w));
            }
        }
        __syncthreads();
        ROLL_PH(0);
        // ---- layer 2: this wave's output tiles (B from LDS, A streamed), folded into partial logits
        float lgp[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int k2 = 0; k2 < kOwn; k2++) {
            const int o = ws + 4 * k2;
            if (o >= NT2) continue;                         // wave-uniform
            // a compiler memory barrier: otherwise the layer-1 activations' LDS reads (the same for every own
            // tile) are kept from the first tile for the next, 128 registers, which spill at 2 waves per SIMD
            asm volatile("" ::: "memory");
            floatx16 acc = {};
#pragma unroll
            for (int tt = 0; tt < NT1; tt++) {
                asm volatile("" ::: "memory");              // (the same per k-tile: its 4 LDS reads stay here)
                float4 fb[4];                               // k-tile i + 1 of the stream
                frag(k2 * NT1 + tt + 1, fb);
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const float4 hb = S.h1f[tt][q][lane];
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q].x, hb.x, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q].y, hb.y, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q].z, hb.z, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q].w, hb.w, acc, 0, 0, 0);
                }
#pragma unroll
                for (int q = 0; q < 4; q++) fa[q] = fb[q];
            }
            const float4* bb = reinterpret_cast<const float4*>(S.net.b2p() + (o * 2 + h) * 16);
            const float4* w3 = reinterpret_cast<const float4*>(S.net.w3p() + (o * 2 + h) * 64);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const float4 bv = bb[q];
                const float hv[4] = {activate<ACT>(acc[4 * q + 0] + bv.x), activate<ACT>(acc[4 * q + 1] + bv.y),
                                     activate<ACT>(acc[4 * q + 2] + bv.z), activate<ACT>(acc[4 * q + 3] + bv.w)};
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const float4 wv = w3[4 * q + u];
                    lgp[0] = fmaf(hv[u], wv.x, lgp[0]);
                    lgp[1] = fmaf(hv[u], wv.y, lgp[1]);
                    lgp[2] = fmaf(hv[u], wv.z, lgp[2]);
                    lgp[3] = fmaf(hv[u], wv.w, lgp[3]);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 4; k++) lgp[k] += __shfl_xor(lgp[k], 32, 64);
        if (h == 0) {
#pragma unroll
            for (int k = 0; k < 4; k++) S.part[w][col][k] = lgp[k];
        }
        __syncthreads();
        ROLL_PH(1);
        // ---- every wave: the same logits, choice and env step
        const float* b3 = S.net.b3();
        float lg[4];
#pragma unroll
        for (int k = 0; k < 4; k++) lg[k] = (((S.part[0][col][k] + S.part[1][col][k]) + S.part[2][col][k]) + S.part[3][col][k]) + b3[k];
        if (ep < a.n) {
            const uint32_t mw = a.use_mask ? mask_word_of(b) : 0x01010101u;
            const double u = a.greedy ? 0.0 : pcg_random(gp);
            float p[4];
            const uint32_t act = softmax_select(lg, mw, a.use_mask != 0, a.greedy != 0, u, p);
            const StepValues ov = env_step_pcg(b, act, sc, mt, ge, a.rc, a.max_steps, lut, code);
            const double r = ov.reward;
            total += r;                            // total_reward += float(reward) (src/reinforce_agent.py:233)
            if constexpr (TRAJ) {
                if (w == 0 && h == 0) {
                    const size_t row = (size_t)t * a.n + ep;
                    a.boards[row] = b;
                    a.actions[row] = (uint8_t)act;
                    a.rewards[row] = r;
                    a.flags[row] = (uint8_t)ov.flags;
                    if (a.probs) reinterpret_cast<float4*>(a.probs)[row] = make_float4(p[0], p[1], p[2], p[3]);
                }
            }
            b = ov.board;
            t += 1;
            if ((ov.flags & (kFTerminated | kFTruncated)) != 0u || t >= a.cap) {
                if (w == 0 && h == 0) {
                    a.lengths[ep] = (int32_t)t;
                    a.totals[ep] = total;
                    a.max_tile[ep] = (uint8_t)mt;
                    a.final_board[ep] = b;
                }
                ep = a.n;
            }
        }
        ROLL_PH(2);
        const bool need = ep >= a.n;
        if (!drained && __ballot(need)) {                // block-uniform
            const uint32_t fresh = claim(need, ep);
            if (need && fresh < a.n) {
                ep = fresh;
                start();
            }
            drained = __ballot(need && fresh >= a.n) != 0ull;
        }
        ROLL_PH(3);
#if G2048_DIAG
        ph[4] += 1;
#endif
    }
#if G2048_DIAG
    if constexpr (TRAJ) {
        if (threadIdx.x == 0 && blockIdx.x < kRollDiagBlocks)
            for (int k = 0; k < 5; k++) g_roll_ph[blockIdx.x * 5 + k] = ph[k];
    }
#endif
}

template <int NT1, int NT2, int ACT, bool TRAJ>
void launch_roll_obs(const RolloutArgs& a, int obs, int grid, hipStream_t s) {
    if (obs == G2048_OBS_LOG2) hipLaunchKernelGGL((rollout_kernel<NT1, NT2, ACT, G2048_OBS_LOG2, TRAJ>), dim3(grid), dim3(kPolBlock), 0, s, a);
    else hipLaunchKernelGGL((rollout_kernel<NT1, NT2, ACT, G2048_OBS_RAW, TRAJ>), dim3(grid), dim3(kPolBlock), 0, s, a);
}

template <int NT1, int NT2, bool TRAJ>
void launch_roll_act(const RolloutArgs& a, int act, int obs, int grid, hipStream_t s) {
    if (act == G2048_ACT_RELU) launch_roll_obs<NT1, NT2, 0, TRAJ>(a, obs, grid, s);
    else launch_roll_obs<NT1, NT2, 1, TRAJ>(a, obs, grid, s);
}

template <int NT1, bool TRAJ>
void launch_roll_nt2(const RolloutArgs& a, int nt2, int act, int obs, int grid, hipStream_t s) {
    switch (nt2) {
        case 1: launch_roll_act<NT1, 1, TRAJ>(a, act, obs, grid, s); break;
        case 2: launch_roll_act<NT1, 2, TRAJ>(a, act, obs, grid, s); break;
        case 4: launch_roll_act<NT1, 4, TRAJ>(a, act, obs, grid, s); break;
        default: launch_roll_act<NT1, 8, TRAJ>(a, act, obs, grid, s); break;
    }
}

int tiles_for(int hsize) {   // hidden units -> 32-unit tiles, rounded up to 1, 2, 4 or 8
    const int t = (hsize + 31) / 32;
    return t <= 1 ? 1 : t <= 2 ? 2 : t <= 4 ? 4 : 8;
}

// the grid of both forms (one workgroup per 32 episode slots, persistent: the slots refill from the queue) and the
// launch by tile counts, activation and obs mode
template <bool TRAJ>
void launch_rollout_form(const RolloutArgs& a, int h1, int h2, int activation, int obs, int64_t n, int cus,
                         hipStream_t s) {
    const int nt1 = tiles_for(h1), nt2 = tiles_for(h2);
    int64_t grid = (n + 31) / 32;
    if (grid > kRollBlocksPerCU * cus) grid = kRollBlocksPerCU * cus;
    switch (nt1) {
        case 1: launch_roll_nt2<1, TRAJ>(a, nt2, activation, obs, (int)grid, s); break;
        case 2: launch_roll_nt2<2, TRAJ>(a, nt2, activation, obs, (int)grid, s); break;
        case 4: launch_roll_nt2<4, TRAJ>(a, nt2, activation, obs, (int)grid, s); break;
        default: launch_roll_nt2<8, TRAJ>(a, nt2, activation, obs, (int)grid, s); break;
    }
}

}  // namespace
