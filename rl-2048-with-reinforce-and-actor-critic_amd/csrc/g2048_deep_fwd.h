// g2048_deep_fwd.h -- the pieces of the any-depth forward that g2048_deep.hip (4 x 4 boards) and
// g2048_sized_policy.hip (boards of 2..8) share: the packed-net descriptor, the bf16 plane split of the one-hot
// first layer, the k-ordered MFMA chain of a dense output tile and the sum of the output-layer partials.  Both
// translation units run exactly this code, which is what keeps g2048_sized_policy(size = 4) bit for bit
// g2048_deep_policy.  Everything is file-local to the including translation unit (device code and small host
// helpers), as it was inside g2048_deep.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "g2048.h"

namespace {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// two floats rounded to nearest even into one dword of bf16 (a in the low half): one v_cvt_pk_bf16_f32
__device__ __forceinline__ uint32_t pk_bf16(float a, float b) {
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    const bf16x2 v = {(__bf16)a, (__bf16)b};
    return __builtin_bit_cast(uint32_t, v);
}

// exact split of 8 floats into three bf16 planes (x = p0 + p1 + p2; each residual is exact in fp32), packed two
// values per dword: 11 VALU per pair
__device__ __forceinline__ void split3_bf16(const float (&v)[8], bf16x8& p0, bf16x8& p1, bf16x8& p2) {
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    u32x4 h, m, l;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const float x0 = v[2 * j], x1 = v[2 * j + 1];
        const uint32_t hh = pk_bf16(x0, x1);
        const float r0 = x0 - __uint_as_float(hh << 16), r1 = x1 - __uint_as_float(hh & 0xFFFF0000u);
        const uint32_t mm = pk_bf16(r0, r1);
        const float t0 = r0 - __uint_as_float(mm << 16), t1 = r1 - __uint_as_float(mm & 0xFFFF0000u);
        h[j] = hh;
        m[j] = mm;
        l[j] = pk_bf16(t0, t1);
    }
    p0 = __builtin_bit_cast(bf16x8, h);
    p1 = __builtin_bit_cast(bf16x8, m);
    p2 = __builtin_bit_cast(bf16x8, l);
}


constexpr int kMaxHidden = G2048_DEEP_MAX_HIDDEN;   // hidden layers
constexpr int kDeepBlock = 256;                      // 4 waves; two workgroups per CU
constexpr int kActStride = 33;                       // LDS activation row stride in floats: [unit][32 boards + 1]

// the hidden unit held by accumulator register r of lane half h of a v_mfma_f32_32x32x2_f32 result tile
__host__ __device__ inline int tile_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// Packed net layout (floats; nt[l] = 32-unit tiles of hidden layer l, zero padded -- exact, a padded unit's
// outgoing weights are zero):
//   layer 0 weights   one-hot: table [272][32 nt0] row-major (row 17 c + e = W1[17 c + e, :]);
//                     else:    A fragments [nt0][8][64] (k-step s, lane l: W1[2 s + (l >> 5)][32 t + (l & 31)])
//   layer l >= 1      A fragments [nt_l][nt_{l-1}][4][64][4]: output tile o, k-tile t, lane l, k-step s = 4 q + u at
//                     [o][t][q][l][u] = W_l[32 t + tile_row(s, l >> 5)][32 o + (l & 31)] -- k-step s takes the input
//                     units an MFMA result tile holds in its register s (round 5), so a wave's accumulator tile of
//                     layer l - 1 can be the B operand of layer l register for register (the two-layer
//                     g2048_policy's layout); the LDS-fed chains read the same rows (frag_chain)
//   bias l            [32 nt_l]
//   output layer      [32 nt_{L-1}][4] row-major (a value head is output 0), bias [4]
//   one-hot W1 planes [nt0][16 cells][3 planes][64 lanes] dwords x 4 (round 5): the A fragment of
//                     v_mfma_f32_32x32x16_bf16 for unit tile t, cell c, plane p -- lane l holds bf16 plane p of
//                     W1[17 c + 8 (l >> 5) + j][32 t + (l & 31)], j = 0..7 (split3_bf16: w = p0 + p1 + p2 exactly)
// (g2048_sized_policy.hip packs the same segments for N*N cells: layer 0 differs, see sized_layout there.)
struct DeepNet {
    int L;                            // hidden layers
    int onehot;                       // first layer is the one-hot bf16-plane table
    int nt[kMaxHidden];
    int64_t w[kMaxHidden + 1], b[kMaxHidden + 1];
    int64_t wpl;                      // one-hot: W1's bf16-plane A fragments (see the layout note above)
    int64_t total;
};

int tiles_of(int h) { return (h + 31) / 32; }

template <int ACT>
__device__ __forceinline__ float activate(float z) {
    if constexpr (ACT == 0) return fmaxf(z, 0.0f);
    else return 1.0f / (1.0f + expf(-z));
}

// The k-ordered MFMA chain of one output tile over k-tiles [t0, t1): A = the tile's weight fragments `fo` (4 float4
// per lane per k-tile, streamed from L2), B = the activation rows `in` (LDS).  Two fragment register sets, fa for
// the even and fb for the odd k-tiles, refilled as a sliding window: as soon as fragment q of k-tile t has fed its 4
// MFMAs, its register is reloaded with fragment q of k-tile t + 2 (a scheduling barrier keeps the load there), so
// every fragment load is issued two k-tiles (~2,000 cycles) before its use -- L2 latency under the gradient kernel's
// load exceeded the one k-tile of round 4's double buffer.  Past the end the window reloads the last k-tile
// (harmless, an L1 hit).  (Without a barrier hipcc sank every fragment load next to its MFMA and waited for it there:
// four L2 round trips per k-tile.)  The B operands run one segment (4 k-steps) ahead: the next segment's two
// ds_read2 are issued before this segment's MFMAs, so no segment waits for LDS reads issued next to its own first
// MFMA (round 6: runner-config update 1.215 -> 1.179 s, rollout 0.252 -> 0.240 s, `profiles/round6/r7h/`).  Same
// MFMAs in the same order as a plain loop.  (Also round 6, in the 64-sample gradient kernel: k-tile 0's fragments of
// each wave's first item loaded before the barrier that opens the phase -- 92 spilled SGPRs, update 1.259-1.264 s
// against 1.119-1.123 s; the hidden biases staged in LDS for the epilogues -- 1.119-1.120 s, even; neither kept,
// `profiles/round6/s3/`.)
template <int STRIDE = kActStride>
__device__ __forceinline__ floatx16 frag_chain(const float4* __restrict__ fo, const float* in, int t0, int t1, int h,
                                               int col) {
    floatx16 c = {};
    if (t0 >= t1) return c;
    float4 fa[4], fb[4];
    const int last = t1 - 1;
    // the B operands (4 LDS values per segment) one segment ahead: the next segment's reads are issued before this
    // segment's MFMAs, so a segment waits for reads issued ~4 MFMAs earlier instead of its own
    const float* base = in + 4 * h * STRIDE + col;
    const auto ld4 = [&](float (&v)[4], int t, int q) {
        const float* ib = base + (32 * t + 8 * q) * STRIDE;   // k-step 4 q + u: row 8 q + u + 4 h
        v[0] = ib[0 * STRIDE];
        v[1] = ib[1 * STRIDE];
        v[2] = ib[2 * STRIDE];
        v[3] = ib[3 * STRIDE];
    };
    float bc[4], bn[4];
    ld4(bc, t0, 0);
    const auto seg = [&](float4& f, int t, int q, int tn) {
        ld4(bn, q < 3 ? t : (t + 1 < t1 ? t + 1 : last), (q + 1) & 3);   // past the end: a harmless re-read
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(f.x, bc[0], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(f.y, bc[1], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(f.z, bc[2], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(f.w, bc[3], c, 0, 0, 0);
        f = fo[tn * 256 + q * 64];
        __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);   // the next segment's 2 ds_read2 first,
        __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);   // then this segment's 4 MFMAs,
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);   // then the fragment reload
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < 4; i++) bc[i] = bn[i];
    };
#pragma unroll
    for (int q = 0; q < 4; q++) fa[q] = fo[t0 * 256 + q * 64];
#pragma unroll
    for (int q = 0; q < 4; q++) fb[q] = fo[(t0 + 1 < t1 ? t0 + 1 : last) * 256 + q * 64];
    __builtin_amdgcn_sched_barrier(0);
    int t = t0;
    for (; t + 1 < t1; t += 2) {
        const int ta = t + 2 < t1 ? t + 2 : last, tb = t + 3 < t1 ? t + 3 : last;
#pragma unroll
        for (int q = 0; q < 4; q++) seg(fa[q], t, q, ta);
#pragma unroll
        for (int q = 0; q < 4; q++) seg(fb[q], t + 1, q, tb);
    }
    if (t < t1) {
#pragma unroll
        for (int q = 0; q < 4; q++) seg(fa[q], t, q, last);
    }
    return c;
}

// the 4 outputs of board `bb` from the partials (threads 0..31 after deep_forward)
template <class Smem>
__device__ __forceinline__ void deep_logits(const DeepNet& net, const float* __restrict__ P, const Smem& S, int bb,
                                            float lg[4]) {
    const float* bo = P + net.b[net.L];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        float v = S.part[0][bb][k];
#pragma unroll
        for (int p = 1; p < 8; p++) v += S.part[p][bb][k];
        lg[k] = v + bo[k];
    }
}

}  // namespace
