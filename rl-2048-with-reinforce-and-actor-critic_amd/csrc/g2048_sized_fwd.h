// g2048_sized_fwd.h -- the forward for N x N boards, 2 <= N <= 8, that g2048_sized_policy.hip (one forward + choice
// per launch) and g2048_sized_rollout.hip (the persistent whole-rollout kernel) share: the packed-net layout, the
// group's LDS, the forward itself and the action mask through the size switch.  Both translation units run exactly
// this code, which is what keeps the persistent rollout bit for bit the per-step path.  Everything is file-local to
// the including translation unit, as it was inside g2048_sized_policy.hip (the way g2048_deep_fwd.h was carved out
// of g2048_deep.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "g2048.h"
#include "g2048_sized_core.h"
#include "g2048_deep_fwd.h"

namespace sz = g2048::sized;

namespace {

// Packed net (floats): DeepNet's segments (g2048_deep_fwd.h) with layer 0 sized to the board --
//   layer 0 weights   raw / log2: A fragments [nt0][ks][64], ks = ceil(N*N / 2) (k-step s, lane l:
//                     W1[2 s + (l >> 5)][32 t + (l & 31)], zero where 2 s + (l >> 5) >= N*N); one-hot: none
//   dense layers, biases, output layer: as DeepNet
//   one-hot W1 planes [nt0][N*N cells][3 planes][64 lanes] dwords x 4 (lane l: bf16 plane p of
//                     W1[17 c + 8 (l >> 5) + j][32 t + (l & 31)], j = 0..7)
bool sized_layout(int size, int L, const int32_t* hidden, int onehot, DeepNet& n) {
    if (size < 2 || size > 8 || L < 1 || L > kMaxHidden || !hidden) return false;
    const int cells = size * size, ks = (cells + 1) / 2;
    n = DeepNet{};
    n.L = L;
    n.onehot = onehot;
    int64_t off = 0;
    for (int l = 0; l < L; l++) {
        if (hidden[l] < 1 || hidden[l] > 256) return false;
        n.nt[l] = tiles_of(hidden[l]);
        n.w[l] = off;
        if (l == 0) off += onehot ? 0 : (int64_t)n.nt[0] * ks * 64;
        else off += (int64_t)n.nt[l] * n.nt[l - 1] * 1024;
        n.b[l] = off;
        off += 32 * n.nt[l];
    }
    n.w[L] = off;
    off += (int64_t)32 * n.nt[L - 1] * 4;
    n.b[L] = off;
    off += 4;
    n.wpl = onehot ? off : -1;
    if (onehot) off += (int64_t)n.nt[0] * cells * 3 * 64 * 4;
    n.total = off;
    return true;
}

bool obs_ok(int obs_mode) {
    return obs_mode == G2048_OBS_LOG2 || obs_mode == G2048_OBS_RAW || obs_mode == G2048_OBS_ONEHOT;
}

// DeepSmem (g2048_deep.hip) with the group's boards as [word][board]: 72,704 B, two workgroups per CU
struct SizedSmem {
    float act[2][256 * kActStride];   // ping-pong activations [unit][board]
    float part[8][32][4];             // output-layer partial sums [unit slice][board][output]
    uint64_t board[4][32];            // the group's boards, word-major (words >= W are never read)
};

// word wi (wave-uniform) of a board held as 4 registers
__device__ __forceinline__ uint64_t word_of(const uint64_t (&bw)[4], int wi) {
    return wi == 0 ? bw[0] : (wi == 1 ? bw[1] : (wi == 2 ? bw[2] : bw[3]));
}

// deep_forward (g2048_deep.hip) for the group's 32 boards of `cells` cells in `words` words (S.board): layer 0 by the
// board size, then the dense layers and the output-layer partials exactly as there (S.part: 8 partial sums per
// board and output, added by deep_logits).  Every thread of the workgroup calls it; it ends with a barrier.
template <int OBS, int ACT>
__device__ void sized_forward(const DeepNet& net, const float* __restrict__ P, SizedSmem& S, int cells, int words,
                              float obs_scale) {
    const int lane = threadIdx.x & 63, h = lane >> 5, col = lane & 31, w = threadIdx.x >> 6;
    // ---- first hidden layer -> S.act[0]
    {
        float* out = S.act[0];
        const int nt0 = net.nt[0];
        uint64_t bw[4];
#pragma unroll
        for (int wi = 0; wi < 4; wi++) bw[wi] = wi < words ? S.board[wi][col] : 0ull;
        if constexpr (OBS == G2048_OBS_ONEHOT) {
            // wave w, unit tiles w, w + 4; per cell one exact one-hot B operand and 3 MFMAs (hi plane into `hi`, the
            // mid and lo planes into `lo`), cell by cell.  The body is unrolled over 3 cells so that the ring of
            // three fragment sets (two cells in flight ahead of the MFMAs) is indexed by constants while the cell
            // count is a runtime value; past the last cell the ring reloads the last cell (harmless, an L1 hit).
            typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
            const u32x4* fr = reinterpret_cast<const u32x4*>(P + net.wpl) + lane;
            for (int t = w; t < nt0; t += 4) {   // wave-uniform
                const u32x4* ft = fr + (int64_t)t * cells * (3 * 64);
                float bv[16];
#pragma unroll
                for (int i = 0; i < 16; i++) bv[i] = P[net.b[0] + 32 * t + tile_row(i, h)];
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
                    out[(32 * t + tile_row(i, h)) * kActStride + col] = activate<ACT>((hi[i] + lo[i]) + bv[i]);
            }
        } else {
            // k-step s = 8 wi + u of word wi: lane half h supplies the cell in nibble 2 u + h of that word; the 8
            // weight fragments of a word are loaded before its MFMAs (a step past the last reloads the last one)
            const int ks = (cells + 1) >> 1;
            const float* w1f = P + net.w[0];
            for (int t = w; t < nt0; t += 4) {
                floatx16 acc = {};
#pragma unroll 1
                for (int wi = 0; wi < words; wi++) {   // kernel-uniform trip count
                    const uint64_t b = word_of(bw, wi);
                    const float* wf = w1f + ((int64_t)t * ks + 8 * wi) * 64 + lane;
                    const int left = ks - 8 * wi;      // k-steps of this word: 8, fewer in the last word
                    float wv[8], x[8];
#pragma unroll
                    for (int u = 0; u < 8; u++) {
                        wv[u] = wf[(u < left ? u : left - 1) * 64];
                        const uint32_t e = (uint32_t)(b >> (4 * (2 * u + h))) & 15u;
                        if constexpr (OBS == G2048_OBS_LOG2) x[u] = (float)e * obs_scale;
                        else x[u] = e ? (float)(1u << e) : 0.0f;
                    }
#pragma unroll
                    for (int u = 0; u < 8; u++)
                        if (u < left) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[u], x[u], acc, 0, 0, 0);
                }
                const float* bb = P + net.b[0] + 32 * t;
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int u = tile_row(r, h);
                    out[(32 * t + u) * kActStride + col] = activate<ACT>(acc[r] + bb[u]);
                }
            }
        }
    }
    __syncthreads();
    // ---- dense hidden layers 1 .. L-1 (ping-pong)
    for (int l = 1; l < net.L; l++) {
        const float* in = S.act[(l - 1) & 1];
        float* out = S.act[l & 1];
        const int ntin = net.nt[l - 1], ntout = net.nt[l];
        const float4* __restrict__ frag = reinterpret_cast<const float4*>(P + net.w[l]) + lane;
        const float* bias = P + net.b[l];
        for (int o = w; o < ntout; o += 4) {
            const floatx16 acc = frag_chain(frag + (int64_t)o * ntin * 256, in, 0, ntin, h, col);
            const float* bb = bias + 32 * o;
            float bv[16];   // the 16 bias loads issued before the first use
#pragma unroll
            for (int r = 0; r < 16; r++) bv[r] = bb[tile_row(r, h)];
#pragma unroll
            for (int r = 0; r < 16; r++) out[(32 * o + tile_row(r, h)) * kActStride + col] = activate<ACT>(acc[r] + bv[r]);
        }
        __syncthreads();
    }
    // ---- output layer partials: thread (p = tid >> 5, board = tid & 31) sums units [p Hp / 8, (p + 1) Hp / 8)
    {
        const float* in = S.act[(net.L - 1) & 1];
        const int Hp = 32 * net.nt[net.L - 1];
        const int p = threadIdx.x >> 5, bb = threadIdx.x & 31, per = Hp >> 3;
        const float4* wo = reinterpret_cast<const float4*>(P + net.w[net.L]);
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        for (int j = p * per; j < (p + 1) * per; j++) {
            const float x = in[j * kActStride + bb];
            const float4 wv = wo[j];
            s0 = fmaf(x, wv.x, s0);
            s1 = fmaf(x, wv.y, s1);
            s2 = fmaf(x, wv.z, s2);
            s3 = fmaf(x, wv.w, s3);
        }
        S.part[p][bb][0] = s0;
        S.part[p][bb][1] = s1;
        S.part[p][bb][2] = s2;
        S.part[p][bb][3] = s3;
    }
    __syncthreads();
}

// A kernel-uniform value as a per-lane one.  A uniform flag that the slot owners test after the forward otherwise
// lives as a 64-bit lane mask in scalar registers from the kernel's start (and the Philox key as its hoisted 10-round
// key schedule, 20 registers), and the forward then spills scalar registers; held per lane from here on, the test
// is one vector compare in the owners' tail.
template <class T>
__device__ __forceinline__ T per_lane(T v) {
    asm volatile("" : "+v"(v));
    return v;
}

template <int N>
__device__ __forceinline__ uint32_t mask_bits_of(const uint64_t (&bw)[4]) {
    sz::Board<N> b;
#pragma unroll
    for (int w = 0; w < sz::Dim<N>::kWords; w++) b.w[w] = bw[w];
    return sz::action_mask<N>(b);
}

// get_action_mask of a board of `size` as int8[4] in one word: byte a = bit a (mask_word_of of g2048_deep.hip)
__device__ __forceinline__ uint32_t sized_mask_word(int size, const uint64_t (&bw)[4]) {
    uint32_t m;
    switch (size) {   // kernel-uniform
        case 2: m = mask_bits_of<2>(bw); break;
        case 3: m = mask_bits_of<3>(bw); break;
        case 4: m = mask_bits_of<4>(bw); break;
        case 5: m = mask_bits_of<5>(bw); break;
        case 6: m = mask_bits_of<6>(bw); break;
        case 7: m = mask_bits_of<7>(bw); break;
        default: m = mask_bits_of<8>(bw); break;
    }
    return (m & 1u) | ((m & 2u) << 7) | ((m & 4u) << 14) | ((m & 8u) << 21);
}

}  // namespace
