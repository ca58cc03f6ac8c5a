// g2048_sized_grad.hip -- g2048_deep_grad and g2048_onehot_dw1 for N x N boards, 2 <= N <= 8 (include/g2048_sized.h):
// update_batch's actor or critic gradient of a chunk of samples in one fused launch, straight from the plane-major
// board words -- no observation row, no GEMM, no torch backward (part of libg2048.so).
//
// The kernel is the 32-sample form of deep_grad_kernel (g2048_deep.hip): one 8-wave workgroup per CU takes groups of
// 32 samples; every hidden layer's activations stay in LDS as [unit][33] in a region of their own, the deltas
// overwrite them top down, the dense dW tiles (32 x 32, v_mfma_f32_32x32x2_f32 over the 32 samples) sit in
// accumulators across all groups of the workgroup, the output layer's and the biases' partial sums in registers /
// LDS, and each workgroup writes one complete partial slab at its end (zeros when it got no group).  The dense
// forward is frag_chain without a k-split, i.e. sized_forward's arithmetic.  What depends on the board size:
//   * boards: the group's words in LDS as [word][sample], all four words (words >= W and ragged samples as 0).
//   * layer 0 forward: sized_forward's (g2048_sized_fwd.h) on 8 waves -- raw / log2 by ceil(N*N / 2) k-steps word by
//     word, one-hot cell by cell on W_0's three bf16 planes.
//   * dW_0, raw / log2: per unit tile one (N*N <= 32) or two 32-feature tiles, A = delta_0 [unit][sample], B = the
//     obs value of cell 32 ft + col of sample 2 s + h rebuilt from the LDS words; features >= N*N multiply zeros.
//   * dW_0, one-hot: delta_0 goes out as d0_out [n][H0p] through a buffer resource (ragged rows fall outside
//     num_records) and g2048_sized_onehot_dw1 forms the 17 N*N rows from the board planes.
//   * the actor's mask: sized_mask_word (a kernel-uniform switch over the 7 sizes).
// The board size is a runtime value: {raw, log2, one-hot} x {ReLU, Sigmoid} = 6 kernels.  One-hot kernels hold 5 dense
// tiles per wave (40 per launch), raw / log2 ones 4 (32 per launch) next to the two dW_0 tiles; a net past that, or
// past 160 KiB of LDS, is not covered (g2048_sized_grad_slab returns -1): there is no multi-launch form.
//
// g2048_sized_onehot_dw1 is onehot_dw1_mfma_kernel (g2048_deep.hip) run once per board word: workgroup (x, y) takes
// sample range x and word y, i.e. the 16 cells 16 y .. 16 y + 15 as 8 cell pairs, one accumulator tile each, and
// writes their 17-row blocks of the slab; word 0's workgroups also write db.  Same arithmetic: the exact one-hot A
// operand against each delta's three exact bf16 planes (split3_bf16), fp32 accumulation in a fixed order.
#include <hip/hip_runtime.h>

#include <atomic>
#include <string>

#include "g2048.h"
#include "g2048_sized_core.h"
#include "g2048_deep_fwd.h"
#include "g2048_sized_fwd.h"   // sized_layout, obs_ok, word_of, sized_mask_word

using namespace g2048;

namespace g2048_internal {   // g2048.hip
int set_error(int code, const char* msg);
}  // namespace g2048_internal

namespace {

int gfail(int code, const std::string& msg) { return g2048_internal::set_error(code, msg.c_str()); }

constexpr int kGradWaves = 8;
constexpr int kGradBlock = 64 * kGradWaves;
constexpr int kNB = 32;          // samples per group
constexpr int kSS = kNB + 1;     // LDS row stride in floats: [unit][32 samples + 1]
constexpr int kTilesOneHot = 5;  // dense dW tiles per wave
constexpr int kTilesDense = 4;   // raw / log2: next to the two dW_0 tiles
// LDS behind the activations (floats): output partials [8][32][4], g [32][4], boards [4][32] uint64, db sums
// [kMaxHidden][256], output weights [256][4] + bias [4], per-sample inputs [3][32], db_out sums [32][4]
constexpr int kTailFloats = 8 * kNB * 4 + kNB * 4 + 2 * 4 * kNB + kMaxHidden * 256 + 256 * 4 + 4 + 3 * kNB + kNB * 4;

struct SizedGradArgs {
    DeepNet net;
    const float* packed;          // forward layout (g2048_sized_pack)
    const float* bpacked;         // backward fragments (g2048_deep_grad_pack)
    int64_t boff[kMaxHidden];     // per dense layer l >= 1: offset of its backward fragments
    int64_t pw[kMaxHidden + 1], pb[kMaxHidden + 1];   // partial-slab offsets: dW_l, db_l (l = L: the output layer)
    int64_t pslab;                // floats per partial slab
    const uint64_t* boards;
    int64_t bstride;              // plane stride of boards
    const uint8_t* actions;
    const float* coef;            // actor: advantage x step weight; critic: step weight
    int critic, huber;
    float huber_delta;
    const float* target;          // critic: r + gamma V(s') m
    float* delta_out;             // critic: target - V (NULL ok)
    float* v_out;                 // critic: V (NULL ok)
    float* d0_out;                // one-hot: delta_0 [n][H0p] for g2048_sized_onehot_dw1
    float* hidden_out[kMaxHidden];   // layer l's activations [n][H_l p] as the forward computed them (NULL ok)
    int want_hidden;              // any hidden_out entry set
    float* part;                  // [gridDim.x][pslab]
    float obs_scale;
    uint32_t n;
    int use_mask;
    int size;
    int ntiles;                   // dense dW tiles in all
    int tile_begin[kMaxHidden];   // flattened tile index of layer l's first tile (l >= 1)
    int aoff[kMaxHidden];         // LDS float offset of layer l's activations / deltas
    int lds_tail;                 // LDS float offset of the output partials, g, boards and bias sums
};

// LDS-only barrier, fresh_tid and the lane ids of a phase: see g2048_deep.hip (lds_barrier, fresh_tid,
// DEEP_LANE_IDS) for why the gradient kernel orders its phases this way
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

template <int ACT>
__device__ __forceinline__ float act_deriv(float a) {   // from the activation (src/reinforce_agent.py:624-636)
    if constexpr (ACT == 0) return a > 0.0f ? 1.0f : 0.0f;
    else return a * (1.0f - a);
}

// The kernel's arguments read again from the kernarg segment through a pointer the compiler cannot see through: what a
// phase needs is loaded (scalar loads) in that phase.  Read from the by-value parameter, hipcc loads every field in
// the prologue and keeps what it derives from them -- above all every kernel-uniform test (critic, use_mask, N*N > 32, a hidden_out
// entry set, ...) as a 64-bit lane mask -- across the group loop, spilling ~30 scalar registers to VGPR lanes.
typedef const __attribute__((address_space(4))) SizedGradArgs* SizedGradArgsK;
__device__ __forceinline__ SizedGradArgsK fresh_args() {
    SizedGradArgsK p = (SizedGradArgsK)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p;
}

__device__ __forceinline__ int fresh_tid() {
    int t = (int)threadIdx.x;
    asm volatile("" : "+v"(t));
    return t;
}
#define SIZED_LANE_IDS                                                            \
    const SizedGradArgsK A = fresh_args();                                        \
    (void)A;                                                                      \
    const int tid = fresh_tid(), lane = tid & 63, h = lane >> 5, col = lane & 31; \
    (void)lane;                                                                   \
    (void)h;                                                                      \
    (void)col

template <int OBS>
__device__ __forceinline__ float obs_of_exp(uint32_t e, float scale) {
    if constexpr (OBS == G2048_OBS_LOG2) return (float)e * scale;
    else return e ? (float)(1u << e) : 0.0f;
}

template <int OBS, int ACT>
__global__ void __launch_bounds__(kGradBlock, 1) sized_grad_kernel(SizedGradArgs a) {
    constexpr int NW = kGradWaves, NB = kNB, SS = kSS, kBlock = kGradBlock;
    constexpr int TPW = OBS == G2048_OBS_ONEHOT ? kTilesOneHot : kTilesDense;
    extern __shared__ float dyn[];
    const int L = a.net.L;
    const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, col = lane & 31,
              w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const auto actl = [&](SizedGradArgsK A, int l) { return dyn + A->aoff[l]; };
    float* lds_end = dyn + a.lds_tail;
    float (*part)[NB][4] = reinterpret_cast<float (*)[NB][4]>(lds_end);          // [8][NB][4]
    float (*gs)[4] = reinterpret_cast<float (*)[4]>(lds_end + 8 * NB * 4);       // [NB][4]
    uint64_t* bds = reinterpret_cast<uint64_t*>(lds_end + 8 * NB * 4 + NB * 4);  // [4 words][NB]
    float* dbs = lds_end + 8 * NB * 4 + NB * 4 + 2 * 4 * NB;                     // [kMaxHidden][256]: db_l of unit tid
    float* wol = dbs + kMaxHidden * 256;                                         // [HL][4] output weights, then [4] bias
    float* smp_in = wol + 256 * 4 + 4;                                           // [3][NB]: coef, action, target
    float* dbo_l = smp_in + 3 * NB;                                              // [NB][4]: db_out sums per sample slot
    if (tid < 256)
        for (int l = 0; l < kMaxHidden; l++) dbs[l * 256 + tid] = 0.0f;
    if (tid < 4 * NB) dbo_l[tid] = 0.0f;
    {   // the output layer's weights and bias in LDS for the whole launch
        const float* P = a.packed;
        const DeepNet& net = a.net;
        const int HLw = 32 * net.nt[L - 1] * 4;
        for (int i = tid; i < HLw + 4; i += kBlock) wol[i] = i < HLw ? P[net.w[L] + i] : P[net.b[L] + (i - HLw)];
    }
    floatx16 acc[TPW];
#pragma unroll
    for (int k = 0; k < TPW; k++) acc[k] = floatx16{};
    // raw / log2: dW_0^T of unit tile w, feature tiles 0 (features 0..31) and 1 (32..63, N >= 6)
    floatx16 acc0[2];
    acc0[0] = acc0[1] = floatx16{};
    float dwo[4] = {0.f, 0.f, 0.f, 0.f}, dbl = 0.f;
    const int HL = 32 * a.net.nt[L - 1];   // (oq = 512 / HL sample ranges of the output layer: per phase)
    const float4* wout = reinterpret_cast<const float4*>(wol);
    const float* bo = wol + 4 * HL;
    const uint32_t groups = (a.n + (uint32_t)(NB - 1)) / (uint32_t)NB;
    for (uint32_t gi = blockIdx.x; gi < groups; gi += gridDim.x) {
        {
            SIZED_LANE_IDS;
            const uint32_t j = gi * (uint32_t)NB + (uint32_t)(tid & (NB - 1));
            const bool valid = j < A->n;
            const uint32_t jc = valid ? j : A->n - 1u;
            const int words = (A->size * A->size + 15) >> 4;
            // thread (word tid >> 5, sample tid & 31): all four words written, absent ones as 0
            uint64_t bw = 0ull;
            if (tid < 4 * NB && (tid >> 5) < words && valid) bw = A->boards[(int64_t)(tid >> 5) * A->bstride + j];
            const float cf = (tid < NB && valid) ? A->coef[jc] : 0.0f;
            const uint32_t act_j = (tid < NB && !A->critic) ? A->actions[jc] : 0u;
            const float tg = (tid < NB && A->critic) ? A->target[jc] : 0.0f;
            if (tid < 4 * NB) bds[tid] = bw;
            __syncthreads();   // (a fence: vmcnt(0) -- the loads above have arrived)
            if (tid < NB) {    // read back at the logits: their registers are free until then
                smp_in[tid] = cf;
                smp_in[NB + tid] = __uint_as_float(act_j);
                smp_in[2 * NB + tid] = tg;
            }
        }
        // ---- forward: layer 0 (sized_forward's, unit tiles w, w + 8, ...)
        {
            SIZED_LANE_IDS;
            float* out = actl(A, 0);
            const float* P = A->packed;
            const int nt0 = A->net.nt[0], cells = A->size * A->size, words = (cells + 15) >> 4;
            uint64_t bw[4];
#pragma unroll
            for (int wi = 0; wi < 4; wi++) bw[wi] = bds[wi * NB + col];
            if constexpr (OBS == G2048_OBS_ONEHOT) {
                typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
                const u32x4* fr = reinterpret_cast<const u32x4*>(P + A->net.wpl) + lane;
                for (int t = w; t < nt0; t += NW) {   // wave-uniform
                    const u32x4* ft = fr + (int64_t)t * cells * (3 * 64);
                    float bv[16];
#pragma unroll
                    for (int i = 0; i < 16; i++) bv[i] = P[A->net.b[0] + 32 * t + tile_row(i, h)];
                    u32x4 f[3][3];
#pragma unroll
                    for (int q = 0; q < 2; q++)   // cells >= 4: cells 0 and 1 exist
#pragma unroll
                        for (int pl = 0; pl < 3; pl++) f[q][pl] = ft[(q * 3 + pl) * 64];
                    floatx16 hi = {}, lo = {};
                    for (int c0 = 0; c0 < cells; c0 += 3) {
#pragma unroll
                        for (int j = 0; j < 3; j++) {
                            const int c = c0 + j;
                            if (c < cells) {   // wave-uniform
                                const int cn = c + 2 < cells ? c + 2 : cells - 1;
#pragma unroll
                                for (int pl = 0; pl < 3; pl++) f[(j + 2) % 3][pl] = ft[(cn * 3 + pl) * 64];
                                __builtin_amdgcn_sched_barrier(0);
                                const uint32_t nib = (uint32_t)(word_of(bw, c >> 4) >> (4 * (c & 15))) & 15u;
                                u32x4 dv;
#pragma unroll
                                for (int jj = 0; jj < 4; jj++)
                                    dv[jj] = (nib == (uint32_t)(8 * h + 2 * jj) ? 0x3F80u : 0u) |
                                             (nib == (uint32_t)(8 * h + 2 * jj + 1) ? 0x3F800000u : 0u);
                                const bf16x8 bvv = __builtin_bit_cast(bf16x8, dv);
                                hi = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, f[j][0]), bvv, hi, 0, 0, 0);
                                lo = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, f[j][1]), bvv, lo, 0, 0, 0);
                                lo = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, f[j][2]), bvv, lo, 0, 0, 0);
                            }
                        }
                    }
#pragma unroll
                    for (int i = 0; i < 16; i++)
                        out[(32 * t + tile_row(i, h)) * SS + col] = activate<ACT>((hi[i] + lo[i]) + bv[i]);
                }
            } else {
                const int ks = (cells + 1) >> 1;
                const float* w1f = P + A->net.w[0];
                for (int t = w; t < nt0; t += NW) {
                    floatx16 c = {};
#pragma unroll 1
                    for (int wi = 0; wi < words; wi++) {   // kernel-uniform trip count
                        const uint64_t b = word_of(bw, wi);
                        const float* wf = w1f + ((int64_t)t * ks + 8 * wi) * 64 + lane;
                        const int left = ks - 8 * wi;      // k-steps of this word: 8, fewer in the last word
                        float wv[8], x[8];
#pragma unroll
                        for (int u = 0; u < 8; u++) {
                            wv[u] = wf[(u < left ? u : left - 1) * 64];
                            x[u] = obs_of_exp<OBS>((uint32_t)(b >> (4 * (2 * u + h))) & 15u, A->obs_scale);
                        }
#pragma unroll
                        for (int u = 0; u < 8; u++)
                            if (u < left) c = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[u], x[u], c, 0, 0, 0);
                    }
                    const float* bb = P + A->net.b[0] + 32 * t;
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        const int u = tile_row(r, h);
                        out[(32 * t + u) * SS + col] = activate<ACT>(c[r] + bb[u]);
                    }
                }
            }
        }
        lds_barrier();
        // ---- forward: dense layers (each into its own region; sized_forward's chain)
        for (int l = 1; l < L; l++) {
            SIZED_LANE_IDS;
            const float* in = actl(A, l - 1);
            float* out = actl(A, l);
            const float* P = A->packed;
            const int ntin = A->net.nt[l - 1], ntout = A->net.nt[l];
            const float4* __restrict__ frag = reinterpret_cast<const float4*>(P + A->net.w[l]) + lane;
            for (int o = w; o < ntout; o += NW) {
                const floatx16 c = frag_chain<SS>(frag + (int64_t)o * ntin * 256, in, 0, ntin, h, col);
                const float* bb = P + A->net.b[l] + 32 * o;
                float bv[16];
#pragma unroll
                for (int r = 0; r < 16; r++) bv[r] = bb[tile_row(r, h)];
#pragma unroll
                for (int r = 0; r < 16; r++) out[(32 * o + tile_row(r, h)) * SS + col] = activate<ACT>(c[r] + bv[r]);
            }
            lds_barrier();
        }
        // ---- output layer partials (as sized_forward; threads 0..255)
        {
            SIZED_LANE_IDS;
            if (tid < 8 * NB) {
                const float* in = actl(A, L - 1);
                const int pp = tid >> 5, bb = tid & (NB - 1), per = HL >> 3;
                float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
                for (int u = pp * per; u < (pp + 1) * per; u++) {
                    const float x = in[u * SS + bb];
                    const float4 wv = wout[u];
                    s0 = fmaf(x, wv.x, s0);
                    s1 = fmaf(x, wv.y, s1);
                    s2 = fmaf(x, wv.z, s2);
                    s3 = fmaf(x, wv.w, s3);
                }
                part[pp][bb][0] = s0;
                part[pp][bb][1] = s1;
                part[pp][bb][2] = s2;
                part[pp][bb][3] = s3;
            }
            lds_barrier();
        }
        // ---- logits -> g (threads 0..31, one sample each); the activations out for hidden_out (diagnostics)
        {
            SIZED_LANE_IDS;
            const uint32_t j = gi * (uint32_t)NB + (uint32_t)(tid & (NB - 1));
            const bool valid = j < A->n;
            if (A->want_hidden) {   // kernel-uniform; production calls pass no hidden_out
                const uint32_t left = A->n - gi * (uint32_t)NB < (uint32_t)NB ? A->n - gi * (uint32_t)NB : (uint32_t)NB;
                for (int l = 0; l < L; l++) {
                    float* ho = A->hidden_out[l];
                    if (!ho) continue;
                    const int Hp = 32 * A->net.nt[l];
                    const float* src = actl(A, l);
                    for (int i = tid; i < NB * Hp; i += kBlock) {
                        const int s = i / Hp, u = i - s * Hp;
                        if ((uint32_t)s < left) ho[((size_t)gi * NB + (size_t)s) * (size_t)Hp + (size_t)u] = src[u * SS + s];
                    }
                }
            }
            if (tid < NB) {
                const float cf_ = smp_in[tid];
                const uint32_t act_j_ = __float_as_uint(smp_in[NB + tid]);
                const float tg_ = smp_in[2 * NB + tid];
                float lg[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    float v = part[0][tid][k];
#pragma unroll
                    for (int q = 1; q < 8; q++) v += part[q][tid][k];
                    lg[k] = v + bo[k];
                }
                float g[4];
                if (!A->critic) {
                    // logits_to_probs (src/MLP.py:139-156) and the policy-gradient logits delta (:328-354)
                    uint32_t mw = 0x01010101u;
                    if (A->use_mask) {
                        uint64_t bw[4];
#pragma unroll
                        for (int wi = 0; wi < 4; wi++) bw[wi] = bds[wi * NB + tid];
                        mw = sized_mask_word(A->size, bw);
                    }
                    const uint32_t act = valid ? act_j_ : 0u;
                    float l4[4];
#pragma unroll
                    for (int k = 0; k < 4; k++) l4[k] = ((mw >> (8 * k)) & 0xFFu) ? lg[k] : -1e9f;
                    const float mx = fmaxf(fmaxf(l4[0], l4[1]), fmaxf(l4[2], l4[3]));
                    float e[4];
#pragma unroll
                    for (int k = 0; k < 4; k++) e[k] = expf(l4[k] - mx);
                    const float es = ((e[0] + e[1]) + e[2]) + e[3];
#pragma unroll
                    for (int k = 0; k < 4; k++) g[k] = (((uint32_t)k == act ? 1.0f : 0.0f) - e[k] / es) * cf_;
                } else {
                    // the critic's value-loss gradient (update_batch :403-498, _get_grad_logits_critic :884-910)
                    const float diff = lg[0] - tg_;
                    const float gd = (A->huber && fabsf(diff) > A->huber_delta) ? copysignf(A->huber_delta, diff) : diff;
                    g[0] = gd * cf_;
                    g[1] = g[2] = g[3] = 0.0f;
                    if (valid && A->delta_out) A->delta_out[j] = tg_ - lg[0];
                    if (valid && A->v_out) A->v_out[j] = lg[0];
                }
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    gs[tid][k] = g[k];
                    dbo_l[tid * 4 + k] += g[k];
                }
            }
            lds_barrier();
        }
        {
            SIZED_LANE_IDS;
            // ---- output layer backward: dW_out, db_{L-1}, delta_{L-1} in place; thread (unit u, sample range q)
            const int oq = kBlock / HL, oper = (NB + oq - 1) / oq;
            if (tid < oq * HL) {
                const int u = tid % HL, q = tid / HL, n0 = q * oper, n1 = n0 + oper < NB ? n0 + oper : NB;
                float* arow = actl(A, L - 1) + u * SS;
                const float4 wv = wout[u];
                float d0 = dwo[0], d1 = dwo[1], d2 = dwo[2], d3 = dwo[3], db = dbl;
                for (int n2 = n0; n2 < n1; n2++) {
                    const float x = arow[n2];
                    const float4 g4 = *reinterpret_cast<const float4*>(gs[n2]);
                    d0 = fmaf(x, g4.x, d0);
                    d1 = fmaf(x, g4.y, d1);
                    d2 = fmaf(x, g4.z, d2);
                    d3 = fmaf(x, g4.w, d3);
                    float dh = g4.x * wv.x;
                    dh = fmaf(g4.y, wv.y, dh);
                    dh = fmaf(g4.z, wv.z, dh);
                    dh = fmaf(g4.w, wv.w, dh);
                    const float dl = dh * act_deriv<ACT>(x);
                    db += dl;
                    arow[n2] = dl;
                }
                dwo[0] = d0; dwo[1] = d1; dwo[2] = d2; dwo[3] = d3;
                dbl = db;
            }
            lds_barrier();
        }
        // ---- dense layers top down: dW_l (MFMA over the 32 samples), then delta_{l-1} (MFMA chain) in place
        for (int l = L - 1; l >= 1; l--) {
            SIZED_LANE_IDS;
            const float* Al = actl(A, l - 1);
            const float* D = actl(A, l);
            const int ntin = A->net.nt[l - 1], ntout = A->net.nt[l];
            const int f0 = A->tile_begin[l], f1 = f0 + ntin * ntout;
#pragma unroll
            for (int k = 0; k < TPW; k++) {
                const int f = w + NW * k;
                if (f >= f0 && f < f1) {                     // wave-uniform
                    const int ti = (f - f0) / ntout, tj = (f - f0) % ntout;
                    const float* ap = Al + (32 * ti + col) * SS + h;
                    const float* dp = D + (32 * tj + col) * SS + h;
                    floatx16 c = acc[k];
                    // in chunks of 8 k-steps, the next chunk's operands read while this chunk's MFMAs run
                    float av[2][8], dv[2][8];
#pragma unroll
                    for (int i = 0; i < 8; i++) {
                        av[0][i] = ap[2 * i];
                        dv[0][i] = dp[2 * i];
                    }
#pragma unroll
                    for (int hh = 0; hh < 2; hh++) {
                        if (hh + 1 < 2) {
#pragma unroll
                            for (int i = 0; i < 8; i++) {
                                av[1][i] = ap[2 * (8 + i)];
                                dv[1][i] = dp[2 * (8 + i)];
                            }
                        }
#pragma unroll
                        for (int i = 0; i < 8; i++)
                            c = __builtin_amdgcn_mfma_f32_32x32x2f32(av[hh][i], dv[hh][i], c, 0, 0, 0);
                        if (hh + 1 < 2) {
                            __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);   // the next chunk's reads first
                            __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);   // then this chunk's MFMAs
                            __builtin_amdgcn_sched_barrier(0);
                        }
                    }
                    acc[k] = c;
                }
            }
            // delta_{l-1} = (W_l delta_l) act'(a_{l-1}): output tiles = layer l-1's units, k = layer l's units
            const float4* __restrict__ frag = reinterpret_cast<const float4*>(A->bpacked + A->boff[l]) + lane;
            float* Aw = actl(A, l - 1);
            lds_barrier();                               // every read of a_{l-1} by the dW tiles is done
            for (int o = w; o < ntin; o += NW) {
                const floatx16 c = frag_chain<SS>(frag + (int64_t)o * ntout * 256, D, 0, ntout, h, col);
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    float* pa = Aw + (32 * o + tile_row(r, h)) * SS + col;
                    *pa = c[r] * act_deriv<ACT>(*pa);
                }
            }
            lds_barrier();
            // db_{l-1} of unit tid
            if (tid < 32 * ntin) {
                const float* drow = Aw + tid * SS;
                float db = dbs[(l - 1) * 256 + tid];
#pragma unroll
                for (int n0 = 0; n0 < NB; n0 += 8) {
                    float v[8];
#pragma unroll
                    for (int i = 0; i < 8; i++) v[i] = drow[n0 + i];
                    __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
#pragma unroll
                    for (int i = 0; i < 8; i++) db += v[i];
                }
                dbs[(l - 1) * 256 + tid] = db;
            }
        }
        // ---- first layer's weight gradient
        {
            SIZED_LANE_IDS;
            if constexpr (OBS == G2048_OBS_ONEHOT) {
                // delta_0 out for g2048_sized_onehot_dw1: row j, unit tid (coalesced rows), through a buffer resource
                // over the group's rows (the rows past a ragged group's end fall outside num_records)
                const int H0 = 32 * A->net.nt[0];
                if (tid < H0) {
                    const float* drow = actl(A, 0) + tid * SS;
                    const uint32_t left = A->n - gi * (uint32_t)NB < (uint32_t)NB ? A->n - gi * (uint32_t)NB : (uint32_t)NB;
                    const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc(
                        A->d0_out + (size_t)gi * (uint32_t)NB * (uint32_t)H0, 0, (int)(left * (uint32_t)H0 * 4u), 0x00020000);
                    const int rowb = __builtin_amdgcn_readfirstlane(H0 * 4);
                    int so = 0;
#pragma unroll
                    for (int n0 = 0; n0 < NB; n0 += 8) {
                        float v[8];
#pragma unroll
                        for (int i = 0; i < 8; i++) v[i] = drow[n0 + i];
                        __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);   // the 4 ds_read2 first
                        __builtin_amdgcn_sched_group_barrier(0x040, 8, 0);   // then the 8 stores
#pragma unroll
                        for (int i = 0; i < 8; i++) {
                            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[i]), rd, tid * 4, so, 0);
                            so += rowb;
                            asm volatile("" : "+s"(so));   // one running offset, not 32 hoisted constants
                        }
                    }
                }
            } else {
                // dW_0^T of unit tile w (32 units x 32 features per feature tile): A = delta_0 [unit][sample], B = x
                // [sample][feature 32 ft + col] rebuilt from word 2 ft + (col >> 4) of sample 2 s + h (a word past W
                // and a nibble past N*N are 0, and 0 is the obs value of an empty cell: those products are 0)
                const int cells = A->size * A->size;
                if (w < A->net.nt[0]) {
                    const float* dp = actl(A, 0) + (32 * w + col) * SS + h;
                    const int sh = 4 * (col & 15);
                    const int nft = cells > 32 ? 2 : 1;   // kernel-uniform
#pragma unroll
                    for (int ft = 0; ft < 2; ft++) {
                        if (ft < nft) {
                            floatx16 c = acc0[ft];
                            const uint64_t* bp = bds + (2 * ft + (col >> 4)) * NB + h;
#pragma unroll
                            for (int s2 = 0; s2 < 16; s2++) {
                                const float xv = obs_of_exp<OBS>((uint32_t)(bp[2 * s2] >> sh) & 15u, A->obs_scale);
                                c = __builtin_amdgcn_mfma_f32_32x32x2f32(dp[2 * s2], xv, c, 0, 0, 0);
                            }
                            acc0[ft] = c;
                        }
                    }
                }
            }
            lds_barrier();   // the next group rewrites the boards and layer 0: every LDS access done
        }
    }
    // ---- the output layer's (unit, range) partials summed per unit in range order (LDS: the activation area), db_out's
    //      32 sample slots in slot order, then this workgroup's partial slab
    float dbo = 0.0f;
    __syncthreads();   // (a workgroup without a group comes here straight from the LDS initialisation)
    {
        float* red = dyn;                                   // [oq][HL][5]
        const int oq = kBlock / HL;
        if (tid < NB) {
#pragma unroll
            for (int k = 0; k < 4; k++) gs[tid][k] = dbo_l[tid * 4 + k];
        }
        if (tid < oq * HL) {
#pragma unroll
            for (int k = 0; k < 4; k++) red[tid * 5 + k] = dwo[k];
            red[tid * 5 + 4] = dbl;
        }
        __syncthreads();
        if (tid < HL) {
            float sum[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
            for (int q = 0; q < oq; q++)
#pragma unroll
                for (int k = 0; k < 5; k++) sum[k] += red[(q * HL + tid) * 5 + k];
#pragma unroll
            for (int k = 0; k < 4; k++) dwo[k] = sum[k];
            dbs[(L - 1) * 256 + tid] = sum[4];
        }
        if (tid < 4)
            for (int q = 0; q < NB; q++) dbo += gs[q][tid];
        __syncthreads();
    }
    const SizedGradArgsK K = fresh_args(), A = K;
    float* out = K->part + (size_t)blockIdx.x * K->pslab;
#pragma unroll
    for (int k = 0; k < TPW; k++) {
        const int f = w + NW * k;
        if (f < K->ntiles) {
            int l = 1;
            while (l + 1 < L && f >= K->tile_begin[l + 1]) l++;
            const int ntout = K->net.nt[l], f0 = K->tile_begin[l];
            const int ti = (f - f0) / ntout, tj = (f - f0) % ntout;
            const int Ho = 32 * ntout;
#pragma unroll
            for (int r = 0; r < 16; r++)
                out[K->pw[l] + (int64_t)(32 * ti + tile_row(r, h)) * Ho + 32 * tj + col] = acc[k][r];
        }
    }
    if constexpr (OBS != G2048_OBS_ONEHOT) {
        const int H0 = 32 * K->net.nt[0];
        const int nft = K->size * K->size > 32 ? 2 : 1;
        if (w < K->net.nt[0]) {                               // C[unit][feature]: dW_0[feature][unit]
#pragma unroll
            for (int ft = 0; ft < 2; ft++)
                if (ft < nft) {
#pragma unroll
                    for (int r = 0; r < 16; r++)
                        out[K->pw[0] + (int64_t)(32 * ft + col) * H0 + 32 * w + tile_row(r, h)] = acc0[ft][r];
                }
        }
    }
    for (int l = 0; l < L; l++)
        if (tid < 32 * K->net.nt[l]) out[K->pb[l] + tid] = dbs[l * 256 + tid];
    if (tid < HL) {
#pragma unroll
        for (int k = 0; k < 4; k++) out[K->pw[L] + (int64_t)tid * 4 + k] = dwo[k];
    }
    if (tid < 4) out[K->pb[L] + tid] = dbo;
}

// partial-slab layout: deep_grad_layout's (g2048_deep.hip) with layer 0 sized to the board -- dW_0 [rows0][H0p] with
// rows0 = 32 ceil(N*N / 32) (raw / log2; rows >= N*N are zero) or no dW_0 (one-hot) + db_0, dense dW_l [H_{l-1}p][H_lp]
// + db_l, dW_out [H_{L-1}p][4] + db_out [4]; boff / tile_begin as deep_grad_layout (the backward fragments do not
// depend on the size)
struct SizedGradLayout {
    int64_t pw[kMaxHidden + 1], pb[kMaxHidden + 1], pslab;
    int64_t boff[kMaxHidden + 1];
    int ntiles;
    int tile_begin[kMaxHidden];
    int rows0;
};

SizedGradLayout sized_grad_layout(const DeepNet& n, int size) {
    SizedGradLayout g{};
    g.rows0 = n.onehot ? 0 : 32 * ((size * size + 31) / 32);
    int64_t off = 0;
    for (int l = 0; l < n.L; l++) {
        g.pw[l] = off;
        if (l == 0) off += (int64_t)g.rows0 * 32 * n.nt[0];
        else off += (int64_t)32 * n.nt[l - 1] * 32 * n.nt[l];
        g.pb[l] = off;
        off += 32 * n.nt[l];
    }
    g.pw[n.L] = off;
    off += (int64_t)32 * n.nt[n.L - 1] * 4;
    g.pb[n.L] = off;
    off += 4;
    g.pslab = off;
    int64_t bo = 0;
    int tiles = 0;
    for (int l = 1; l < n.L; l++) {
        g.boff[l] = bo;
        bo += (int64_t)n.nt[l - 1] * n.nt[l] * 1024;
        g.tile_begin[l] = tiles;
        tiles += n.nt[l - 1] * n.nt[l];
    }
    g.boff[n.L] = bo;
    if (n.L == 1) g.boff[1] = 0;
    g.ntiles = tiles;
    return g;
}

// floats of the hidden layers' activations, at least the output layer's final reduction ([oq][HL][5], oq HL <= 512)
int64_t sized_grad_act_floats(const DeepNet& n) {
    int64_t units = 0;
    for (int l = 0; l < n.L; l++) units += 32 * n.nt[l];
    const int64_t f = units * kSS, red = 5 * kGradBlock;
    return f > red ? f : red;
}
int64_t sized_grad_lds_bytes(const DeepNet& n) { return (sized_grad_act_floats(n) + kTailFloats) * 4; }

// the net, when one launch covers it: the dense dW tiles within the accumulators, the LDS bill within 160 KiB
bool sized_grad_covered(int size, int obs_mode, int n_hidden, const int32_t* hidden, DeepNet& n) {
    if (!obs_ok(obs_mode) || !sized_layout(size, n_hidden, hidden, obs_mode == G2048_OBS_ONEHOT, n)) return false;
    const int cap = kGradWaves * (n.onehot ? kTilesOneHot : kTilesDense);
    return sized_grad_layout(n, size).ntiles <= cap && sized_grad_lds_bytes(n) <= 160 * 1024;
}

int device_cus() {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) {
        int c = 0;
        if (hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && c > 0) cus = c;
    }
    return cus;
}

int check_hip() {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? G2048_OK : gfail(G2048_EHIP, hipGetErrorString(e));
}

template <int OBS, int ACT>
int launch_sized_grad(const SizedGradArgs& a, int grid, int64_t lds, hipStream_t s) {
    // the dynamic-LDS attribute is per kernel and device: one bit per device id, set on the first launch there
    // (two threads racing both set it, which is harmless)
    static std::atomic<uint64_t> attr_set{0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return gfail(G2048_EHIP, "sized gradient: hipGetDevice failed");
    const uint64_t bit = 1ull << (dev & 63);
    if (!(attr_set.load(std::memory_order_acquire) & bit)) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&sized_grad_kernel<OBS, ACT>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
            return (void)hipGetLastError(),
                   gfail(G2048_EHIP, "sized gradient: hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
        attr_set.fetch_or(bit, std::memory_order_acq_rel);
    }
    hipLaunchKernelGGL((sized_grad_kernel<OBS, ACT>), dim3(grid), dim3(kGradBlock), (unsigned)lds, s, a);
    return check_hip();
}

// ------------------------------------------------------------------------------------- one-hot dW_0 (17 N*N rows)
constexpr int kDw1Step = 16;   // samples per MFMA k-step

struct Dw1Slot {
    float v[8];       // deltas of this lane's unit, samples 8 h .. 8 h + 7 of the step (0 past the range)
    uint32_t bw[8];   // byte w of the same samples' board word: cells 2 w, 2 w + 1 of the word (this wave's pair)
};

// onehot_dw1_mfma_kernel (g2048_deep.hip) for board word blockIdx.y of plane-major boards: wave w owns units
// 32 w .. 32 w + 31 x the word's 8 cell pairs (8 accumulator tiles); a slab has 17 `cells` rows of dW, then db.  A pair
// past the board's last cell accumulates into a tile nobody stores.  Loads go through buffer resources over the
// workgroup's sample range, so a load past its end returns 0.
__global__ void __launch_bounds__(kGradBlock, 1) sized_onehot_dw1_kernel(
    const uint64_t* __restrict__ boards, int64_t bstride, int cells, const float* __restrict__ d1, int h1, int64_t m,
    int64_t ld, int64_t per, float* __restrict__ part) {
    __shared__ uint4 abuf[2][8][64];   // [buffer][cell pair][lane]: the A fragment (8 bf16) of `lane`
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int wi = blockIdx.y;
    const int64_t s0 = (int64_t)blockIdx.x * per, s1 = s0 + per < m ? s0 + per : m;
    const int u = 32 * w + r;
    const bool live = u < h1;
    const uint32_t q = (uint32_t)r >> 4, e = (uint32_t)r & 15u;
    const int nsteps = s1 > s0 ? (int)((s1 - s0 + kDw1Step - 1) / kDw1Step) : 0;
    const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(d1 + s0 * ld), 0, (int)((s1 - s0) * ld * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint64_t*>(boards + (int64_t)wi * bstride + s0), 0, (int)((s1 - s0) * 8), 0x00020000);
    const uint32_t ld4 = (uint32_t)ld * 4u;
    // this lane's first delta; a unit past h1 reads past num_records (0) instead of being masked per load
    const uint32_t dvo = live ? (uint32_t)(8 * h) * ld4 + (uint32_t)u * 4u : 0x80000000u;
    const uint32_t bvo = (uint32_t)(8 * h) * 8u + (uint32_t)w;                      // its first board byte
    floatx16 acc[8];
#pragma unroll
    for (int p = 0; p < 8; p++) acc[p] = floatx16{};
    float db = 0.0f;
    const auto load = [&](int st, Dw1Slot& sl) {
        const uint32_t so = (uint32_t)(st * kDw1Step);   // the step's first sample, relative to s0
#pragma unroll
        for (int k = 0; k < 8; k++) {
            sl.v[k] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rd, (int)dvo, (int)((so + k) * ld4), 0));
            sl.bw[k] = __builtin_amdgcn_raw_buffer_load_b8(rb, (int)bvo, (int)((so + k) * 8u), 0);
        }
    };
    const auto build_a = [&](const Dw1Slot& sl, int buf) {   // this wave's cell pair of the step's one-hot
        uint32_t d[4];
#pragma unroll
        for (int k2 = 0; k2 < 4; k2++) {
            const uint32_t x0 = (sl.bw[2 * k2] >> (4u * q)) & 15u, x1 = (sl.bw[2 * k2 + 1] >> (4u * q)) & 15u;
            d[k2] = (x0 == e ? 0x3F80u : 0u) | (x1 == e ? 0x3F800000u : 0u);   // bf16 1.0 / 0 per sample
        }
        abuf[buf][w][lane] = make_uint4(d[0], d[1], d[2], d[3]);
    };
    const auto step = [&](Dw1Slot& cur, Dw1Slot& nxt, Dw1Slot& ahead, int st, int buf) {
        if (st + 3 < nsteps) load(st + 3, ahead);
#pragma unroll
        for (int k = 0; k < 8; k++) db += cur.v[k];
        bf16x8 pl[3];
        split3_bf16(cur.v, pl[0], pl[1], pl[2]);
        if (st + 1 < nsteps) build_a(nxt, buf ^ 1);
        uint4 av4 = abuf[buf][0][lane];
#pragma unroll
        for (int p = 0; p < 8; p++) {
            const bf16x8 av = __builtin_bit_cast(bf16x8, av4);
            if (p < 7) av4 = abuf[buf][p + 1][lane];
            acc[p] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, pl[0], acc[p], 0, 0, 0);
            acc[p] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, pl[1], acc[p], 0, 0, 0);
            acc[p] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, pl[2], acc[p], 0, 0, 0);
        }
        __syncthreads();   // the next step's A image is complete; this one is free to be rewritten
    };
    Dw1Slot sl0, sl1, sl2, sl3;
    if (nsteps > 0) load(0, sl0);
    if (nsteps > 1) load(1, sl1);
    if (nsteps > 2) load(2, sl2);
    if (nsteps > 0) build_a(sl0, 0);
    __syncthreads();
    for (int st = 0; st < nsteps; st += 4) {   // block-uniform trip count; the four slots rotate
        step(sl0, sl1, sl3, st, 0);
        if (st + 1 >= nsteps) break;
        step(sl1, sl2, sl0, st + 1, 1);
        if (st + 2 >= nsteps) break;
        step(sl2, sl3, sl1, st + 2, 0);
        if (st + 3 >= nsteps) break;
        step(sl3, sl0, sl2, st + 3, 1);
    }
    db += __shfl_xor(db, 32);   // lane half 0 + half 1 (addition commutes: both halves hold the same bits)
    if (!live) return;
    float* slab = part + (int64_t)blockIdx.x * (17 * cells + 1) * h1;
#pragma unroll
    for (int p = 0; p < 8; p++) {
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int row = tile_row(i, h);                       // 16 q' + e' of the pair
            const int cell = 16 * wi + 2 * p + (row >> 4);
            if (cell < cells) slab[(int64_t)(17 * cell + (row & 15)) * h1 + u] = acc[p][i];
        }
    }
    if (h == 0) {
#pragma unroll
        for (int c = 0; c < 16; c++)   // exponent 16: never on a bitboard
            if (16 * wi + c < cells) slab[(int64_t)(17 * (16 * wi + c) + 16) * h1 + u] = 0.0f;
        if (wi == 0) slab[(int64_t)17 * cells * h1 + u] = db;
    }
}

}  // namespace

extern "C" {

int g2048_sized_grad_slab(int size, int obs_mode, int n_hidden, const int32_t* hidden) {
    DeepNet n;
    if (!sized_grad_covered(size, obs_mode, n_hidden, hidden, n)) return -1;
    return (int)sized_grad_layout(n, size).pslab;   // at most ~0.2 M floats
}

int g2048_sized_grad_parts(int size, int obs_mode, int n_hidden, const int32_t* hidden) {
    DeepNet n;
    if (!sized_grad_covered(size, obs_mode, n_hidden, hidden, n)) return -1;
    return device_cus();   // one 8-wave workgroup per CU
}

int g2048_sized_grad_layout(int size, int obs_mode, int n_hidden, const int32_t* hidden, int32_t* w_off,
                            int32_t* b_off, int32_t* dw0_rows, int32_t* dw0_ld) {
    DeepNet n;
    if (!sized_grad_covered(size, obs_mode, n_hidden, hidden, n)) return -1;
    const SizedGradLayout g = sized_grad_layout(n, size);
    for (int l = 0; l <= n.L; l++) {
        if (w_off) w_off[l] = (int32_t)g.pw[l];
        if (b_off) b_off[l] = (int32_t)g.pb[l];
    }
    if (dw0_rows) *dw0_rows = g.rows0;
    if (dw0_ld) *dw0_ld = 32 * n.nt[0];
    return (int)g.pslab;
}

int g2048_sized_grad(int size, const float* packed, const float* grad_packed, int n_hidden, const int32_t* hidden,
                     int activation, int obs_mode, float obs_scale, int use_mask, const uint64_t* boards,
                     int64_t plane_stride, const uint8_t* actions, const float* coef, int critic, int loss,
                     float huber_delta, const float* target, float* delta_out, float* value_out, float* d0_out,
                     float* const* hidden_out, int64_t n, float* partials, int64_t nparts, void* stream) {
    if (size < 2 || size > 8) return gfail(G2048_EINVAL, "size must be in 2..8 (got " + std::to_string(size) + ")");
    if (n < 0) return gfail(G2048_EINVAL, "n < 0");
    if (n > (int64_t(1) << 30)) return gfail(G2048_EINVAL, "n must be <= 2^30 per call");
    if (plane_stride < n)
        return gfail(G2048_EINVAL, "board plane_stride " + std::to_string(plane_stride) + " < " + std::to_string(n) +
                                       " lanes per plane");
    if (activation != G2048_ACT_RELU && activation != G2048_ACT_SIGMOID)
        return gfail(G2048_EINVAL, "Unsupported activation");
    if (!obs_ok(obs_mode)) return gfail(G2048_EINVAL, "sized gradient: obs_mode must be log2, raw or onehot");
    DeepNet net;
    if (!sized_grad_covered(size, obs_mode, n_hidden, hidden, net))
        return gfail(G2048_EINVAL, "sized gradient: net not covered (1..4 hidden layers of 1..256 units whose dense "
                                   "weight-gradient tiles fit one launch)");
    if (critic && loss != 0 && loss != 1) return gfail(G2048_EINVAL, "Unknown critic loss type");
    if (nparts < 1 || nparts > 65535) return gfail(G2048_EINVAL, "sized gradient: nparts out of range");
    if (!packed || !partials || (n > 0 && (!boards || !coef)) || (n > 0 && !critic && !actions) ||
        (n > 0 && critic && !target) || (n > 0 && obs_mode == G2048_OBS_ONEHOT && !d0_out))
        return gfail(G2048_EINVAL, "sized gradient: NULL buffer");
    const SizedGradLayout g = sized_grad_layout(net, size);
    if (g.boff[net.L] > 0 && !grad_packed) return gfail(G2048_EINVAL, "sized gradient: NULL backward fragments");
    if (n == 0) return G2048_OK;   // nothing to add: no launch, the slabs are left as they are
    SizedGradArgs a{};
    a.net = net;
    a.packed = packed;
    a.bpacked = grad_packed;
    int off = 0;
    for (int l = 0; l < net.L; l++) {
        a.boff[l] = g.boff[l];
        a.tile_begin[l] = g.tile_begin[l];
        a.aoff[l] = off;
        off += 32 * net.nt[l] * kSS;
        a.hidden_out[l] = hidden_out ? hidden_out[l] : nullptr;
        if (a.hidden_out[l]) a.want_hidden = 1;
    }
    a.lds_tail = (int)sized_grad_act_floats(net);   // >= off: room for the output layer's reduction
    for (int l = 0; l <= net.L; l++) {
        a.pw[l] = g.pw[l];
        a.pb[l] = g.pb[l];
    }
    a.pslab = g.pslab;
    a.ntiles = g.ntiles;
    a.boards = boards;
    a.bstride = plane_stride;
    a.actions = actions;
    a.coef = coef;
    a.critic = critic ? 1 : 0;
    a.huber = critic && loss == 1;
    a.huber_delta = huber_delta;
    a.target = target;
    a.delta_out = delta_out;
    a.v_out = value_out;
    a.d0_out = d0_out;
    a.part = partials;
    a.obs_scale = obs_scale;
    a.n = (uint32_t)n;
    a.use_mask = use_mask;
    a.size = size;
    const int64_t lds = sized_grad_lds_bytes(net);
    hipStream_t s = (hipStream_t)stream;
    const int grid = (int)nparts;   // every workgroup writes its slab (zeros when it gets no group)
    if (obs_mode == G2048_OBS_ONEHOT)
        return activation == G2048_ACT_RELU ? launch_sized_grad<G2048_OBS_ONEHOT, 0>(a, grid, lds, s)
                                            : launch_sized_grad<G2048_OBS_ONEHOT, 1>(a, grid, lds, s);
    if (obs_mode == G2048_OBS_LOG2)
        return activation == G2048_ACT_RELU ? launch_sized_grad<G2048_OBS_LOG2, 0>(a, grid, lds, s)
                                            : launch_sized_grad<G2048_OBS_LOG2, 1>(a, grid, lds, s);
    return activation == G2048_ACT_RELU ? launch_sized_grad<G2048_OBS_RAW, 0>(a, grid, lds, s)
                                        : launch_sized_grad<G2048_OBS_RAW, 1>(a, grid, lds, s);
}

int g2048_sized_onehot_dw1_slab(int size, int h1) {
    return size < 2 || size > 8 || h1 < 1 || h1 > 256 ? -1 : (17 * size * size + 1) * h1;
}

int g2048_sized_onehot_dw1(int size, const uint64_t* boards, int64_t plane_stride, const float* d1, int h1, int64_t m,
                           int64_t ld, int64_t per, float* partials, int64_t nparts, void* stream) {
    if (size < 2 || size > 8) return gfail(G2048_EINVAL, "size must be in 2..8 (got " + std::to_string(size) + ")");
    if (h1 < 1 || h1 > 256 || m < 0 || ld < h1 || per < 1) return gfail(G2048_EINVAL, "sized one-hot dW1: bad sizes");
    if (m > (int64_t(1) << 30)) return gfail(G2048_EINVAL, "m must be <= 2^30 per call");
    if (plane_stride < m)
        return gfail(G2048_EINVAL, "board plane_stride " + std::to_string(plane_stride) + " < " + std::to_string(m) +
                                       " lanes per plane");
    if (nparts != (m + per - 1) / per || nparts > 65535)
        return gfail(G2048_EINVAL, "sized one-hot dW1: nparts != ceil(m / per)");
    if (per * ld * 4 >= ((int64_t)1 << 31))
        return gfail(G2048_EINVAL, "sized one-hot dW1: per x ld too large (2 GiB per slab range)");
    if (m > 0 && (!boards || !d1 || !partials)) return gfail(G2048_EINVAL, "sized one-hot dW1: NULL buffer");
    if (m == 0) return G2048_OK;
    const int cells = size * size, words = (cells + 15) >> 4;
    hipLaunchKernelGGL(sized_onehot_dw1_kernel, dim3((unsigned)nparts, (unsigned)words), dim3(kGradBlock), 0,
                       (hipStream_t)stream, boards, plane_stride, cells, d1, h1, m, ld, per, partials);
    return check_hip();
}

}  // extern "C"
