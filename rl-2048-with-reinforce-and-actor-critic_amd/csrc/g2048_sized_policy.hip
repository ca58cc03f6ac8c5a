// g2048_sized_policy.hip -- g2048_deep_policy for N x N boards, 2 <= N <= 8 (include/g2048_sized.h): the forward of
// 1..4 hidden layers of 1..256 units (ReLU / Sigmoid) on raw / log2 / one-hot obs + masked softmax + select_action's
// choice, straight from the plane-major bitboards -- no observation buffer, no GEMM launch (part of libg2048.so).
//
// The kernel is deep_policy_kernel's shape (g2048_deep.hip): one 256-thread workgroup (4 waves) per group of 32
// boards, two workgroups per CU, activations ping-ponged in LDS as [unit][board] with row stride 33 floats, 32-unit
// output tiles split over the 4 waves.  Three things depend on the board size:
//   * boards: W = ceil(N*N / 16) words per board, the group's words in LDS as [word][board]; cell k is nibble k & 15
//     of word k >> 4.
//   * layer 0, raw / log2: K = N*N features and ceil(K / 2) k-steps of v_mfma_f32_32x32x2_f32; in step s lane half h
//     supplies feature 2 s + h (a feature index >= K is packed with zero weights; its nibble is 0 anyway).
//   * layer 0, one-hot: per cell the exact one-hot B operand against W1's three bf16 planes (split3_bf16): the hi
//     plane into `hi`, the mid and lo planes into `lo`, cell by cell in cell order, then act((hi + lo) + b1) --
//     deep_forward's arithmetic for N*N cells instead of 16; the fragments stream two cells ahead.
//   * action mask: sized::action_mask<N> of the board, as the int8 x 4 word of mask_word_of.
// The dense layers (frag_chain), the output-layer partials over 8 unit slices, deep_logits, the PCG64 / Philox draw
// and softmax_select are the 4 x 4 kernel's code (g2048_deep_fwd.h, g2048_core.h), in the same order: at N = 4 the
// results are g2048_deep_policy's bit for bit.
// Instantiation: {raw, log2, one-hot} x {ReLU, Sigmoid} x {PCG64, Philox} = 12 kernels, g2048_deep_policy's list;
// the board size is NOT a template parameter.  The cell loops run on a runtime cell count (the one-hot fragment ring
// is indexed by the position inside a 3-cell unrolled body, not by the cell), and N is a compile-time constant only
// inside the mask (a kernel-uniform switch over the 7 sizes, a few dozen bit operations each).  The whole
// translation unit compiles in seconds.  (Obs mode and RNG as runtime branches instead gave 4 kernels that spilled
// 4..10 scalar registers each: every kernel-uniform flag is kept as a 64-bit lane mask across the forward.  See
// per_lane in g2048_sized_fwd.h for the flags that remain.)  The forward, its LDS and the mask live in
// g2048_sized_fwd.h, shared with the persistent rollout (g2048_sized_rollout.hip).  128 VGPRs (raw / log2) or 148
// (one-hot), no spills, 72,704 B of LDS.
// Roofline: as g2048_deep_policy -- the dense layers are fp32-MFMA bound, the one-hot layer 0 runs 3 bf16 MFMAs per
// cell and 32-unit tile; the boards read are 8 W bytes per lane-step against the 4 N*N (* 17) bytes of the
// observation row this path no longer writes and reads back.
#include <hip/hip_runtime.h>

#include <string>

#include "g2048.h"
#include "g2048_sized_core.h"
#include "g2048_deep_fwd.h"
#include "g2048_sized_fwd.h"   // sized_layout, SizedSmem, sized_forward, per_lane, sized_mask_word

using namespace g2048;

namespace g2048_internal {   // g2048.hip
int set_error(int code, const char* msg);
}  // namespace g2048_internal

namespace {

int pfail(int code, const std::string& msg) { return g2048_internal::set_error(code, msg.c_str()); }

struct SizedPackArgs {
    DeepNet net;
    const float* W[kMaxHidden + 1];
    const float* B[kMaxHidden + 1];
    int h[kMaxHidden];
    int out;
    int cells;
    float* dst;
};

// one thread per packed float (deep_pack_kernel for N*N cells)
__global__ void __launch_bounds__(256) sized_pack_kernel(SizedPackArgs a) {
    const DeepNet& n = a.net;
    const int ks = (a.cells + 1) >> 1;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n.total; q += (int64_t)gridDim.x * blockDim.x) {
        if (n.onehot && q >= n.wpl) {   // W1 plane fragment dword (split3_bf16: w = p0 + p1 + p2 exactly)
            const int64_t x = q - n.wpl;
            const int d = (int)(x & 3), lane = (int)((x >> 2) & 63);
            const int64_t r = x >> 8;
            const int p = (int)(r % 3), c = (int)((r / 3) % a.cells), t = (int)(r / (3 * a.cells));
            const int hh = lane >> 5, j = 32 * t + (lane & 31);
            float v8[8];
#pragma unroll
            for (int jj = 0; jj < 8; jj++) v8[jj] = j < a.h[0] ? a.W[0][(int64_t)(17 * c + 8 * hh + jj) * a.h[0] + j] : 0.0f;
            bf16x8 p0, p1, p2;
            split3_bf16(v8, p0, p1, p2);
            typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
            const u32x4 pv = __builtin_bit_cast(u32x4, p == 0 ? p0 : (p == 1 ? p1 : p2));
            a.dst[q] = __uint_as_float(pv[d]);
            continue;
        }
        float v = 0.0f;
        int l = n.L;
        while (l > 0 && q < n.w[l]) l--;          // the segment: [w[l], b[l]) weights, [b[l], w[l+1]) bias
        if (l == n.L) {
            if (q < n.b[l]) {
                const int64_t x = q - n.w[l];
                const int j = (int)(x >> 2), o = (int)(x & 3);
                v = (j < a.h[n.L - 1] && o < a.out) ? a.W[n.L][(int64_t)j * a.out + o] : 0.0f;
            } else {
                const int o = (int)(q - n.b[l]);
                v = o < a.out ? a.B[n.L][o] : 0.0f;
            }
        } else if (q >= n.b[l]) {
            const int j = (int)(q - n.b[l]);
            v = j < a.h[l] ? a.B[l][j] : 0.0f;
        } else if (l == 0) {   // raw / log2 only (a one-hot net has no layer-0 segment here)
            const int64_t x = q - n.w[0];
            const int lane = (int)(x & 63), s = (int)((x >> 6) % ks), t = (int)((x >> 6) / ks);
            const int k = 2 * s + (lane >> 5), j = 32 * t + (lane & 31);
            v = (k < a.cells && j < a.h[0]) ? a.W[0][(int64_t)k * a.h[0] + j] : 0.0f;
        } else {
            const int64_t x = q - n.w[l];
            const int u = (int)(x & 3), lane = (int)((x >> 2) & 63), qq = (int)((x >> 8) & 3);
            const int64_t tt = x >> 10;
            const int t = (int)(tt % n.nt[l - 1]), o = (int)(tt / n.nt[l - 1]);
            const int k = 32 * t + tile_row(4 * qq + u, lane >> 5), j = 32 * o + (lane & 31);
            v = (k < a.h[l - 1] && j < a.h[l]) ? a.W[l][(int64_t)k * a.h[l] + j] : 0.0f;
        }
        a.dst[q] = v;
    }
}

struct SizedPolArgs {
    DeepNet net;
    const float* packed;
    const uint64_t* boards;
    int64_t bstride;              // plane stride of boards
    const uint32_t* lane_state;   // env lane state words (G2048_LS_ACTIVE, step count) or NULL
    const int32_t* lane_index;    // entry j -> lane lane_index[j] (NULL: lane j)
    uint64_t *rs, *inc, *buf;
    uint64_t key;
    const uint64_t* lane_seed;
    float* probs_out;
    float* logits_out;
    uint8_t* actions;             // NULL: forward only (logits_out / the value of a critic net)
    float obs_scale;
    uint32_t n;
    int size;
    int use_mask, greedy;
};

template <int OBS, int ACT, int RNG>
__global__ void __launch_bounds__(kDeepBlock, 2) sized_policy_kernel(SizedPolArgs a) {
    __shared__ SizedSmem S;
    const uint32_t groups = (a.n + 31u) >> 5;
    const int tid = threadIdx.x;
    const int cells = a.size * a.size, words = (cells + 15) >> 4;
    for (uint32_t gi = blockIdx.x; gi < groups; gi += gridDim.x) {
        const uint32_t j = gi * 32u + (uint32_t)(tid & 31);
        const uint32_t jc = j < a.n ? j : a.n - 1u;
        const uint32_t i = a.lane_index ? (uint32_t)a.lane_index[jc] : jc;
        uint64_t bw[4] = {0ull, 0ull, 0ull, 0ull};   // threads 0..31: their board, kept for the mask
        if (tid < 32) {
#pragma unroll
            for (int w = 0; w < 4; w++)
                if (w < words) {
                    bw[w] = a.boards[(int64_t)w * a.bstride + i];
                    S.board[w][tid] = bw[w];
                }
        }
        __syncthreads();
        sized_forward<OBS, ACT>(a.net, a.packed, S, cells, words, a.obs_scale);
        if (tid < 32 && j < a.n) {
            const uint32_t ls = a.lane_state ? a.lane_state[i] : G2048_LS_ACTIVE;
            if (ls & G2048_LS_ACTIVE) {
                float lg[4];
                deep_logits(a.net, a.packed, S, tid, lg);
                if (a.logits_out) reinterpret_cast<float4*>(a.logits_out)[i] = make_float4(lg[0], lg[1], lg[2], lg[3]);
                if (a.actions) {
                    const int use_mask = per_lane(a.use_mask), greedy = per_lane(a.greedy);
                    const uint32_t mw = use_mask ? sized_mask_word(a.size, bw) : 0x01010101u;
                    double u = 0.0;
                    if (!greedy) {
                        if constexpr (RNG == G2048_RNG_PCG64) {
                            Pcg64 g;
                            const ulonglong2 sv = reinterpret_cast<const ulonglong2*>(a.rs)[i];
                            const ulonglong2 iv = reinterpret_cast<const ulonglong2*>(a.inc)[i];
                            const uint64_t bf = a.buf[i];
                            g.s_lo = sv.x; g.s_hi = sv.y; g.i_lo = iv.x; g.i_hi = iv.y;
                            g.has_uint32 = (uint32_t)(bf >> 32); g.uinteger = (uint32_t)bf;
                            u = pcg_random(g);
                            reinterpret_cast<ulonglong2*>(a.rs)[i] = make_ulonglong2(g.s_lo, g.s_hi);
                        } else {
                            const uint64_t sd = a.lane_seed ? a.lane_seed[i] : (uint64_t)i;
                            U4 c{(uint32_t)sd, (uint32_t)(sd >> 32), ls & G2048_LS_STEP_MASK, 3u};
                            const U4 r = philox4x32(c, per_lane((uint32_t)a.key), per_lane((uint32_t)(a.key >> 32)));
                            const uint64_t xx = ((uint64_t)r.x << 32) | r.y;
                            u = (double)(xx >> 11) * (1.0 / 9007199254740992.0);
                        }
                    }
                    float p[4];
                    const uint32_t act = softmax_select(lg, mw, use_mask != 0, greedy != 0, u, p);
                    if (a.probs_out) reinterpret_cast<float4*>(a.probs_out)[i] = make_float4(p[0], p[1], p[2], p[3]);
                    a.actions[i] = (uint8_t)act;
                }
            }
        }
        // S.board is rewritten by threads 0..31 only, after they finished with S.part; every other LDS buffer is
        // rewritten only after the next group's first barrier
    }
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
    return e == hipSuccess ? G2048_OK : pfail(G2048_EHIP, hipGetErrorString(e));
}

template <int OBS, int ACT>
void launch_sized_rng(const SizedPolArgs& a, int rng, int grid, hipStream_t s) {
    if (rng == G2048_RNG_PCG64)
        hipLaunchKernelGGL((sized_policy_kernel<OBS, ACT, G2048_RNG_PCG64>), dim3(grid), dim3(kDeepBlock), 0, s, a);
    else
        hipLaunchKernelGGL((sized_policy_kernel<OBS, ACT, G2048_RNG_PHILOX>), dim3(grid), dim3(kDeepBlock), 0, s, a);
}

template <int OBS>
void launch_sized_act(const SizedPolArgs& a, int act, int rng, int grid, hipStream_t s) {
    if (act == G2048_ACT_RELU) launch_sized_rng<OBS, 0>(a, rng, grid, s);
    else launch_sized_rng<OBS, 1>(a, rng, grid, s);
}

}  // namespace

extern "C" {

int g2048_sized_policy_packed_size(int size, int obs_mode, int n_hidden, const int32_t* hidden) {
    DeepNet n;
    if (!obs_ok(obs_mode) || !sized_layout(size, n_hidden, hidden, obs_mode == G2048_OBS_ONEHOT, n)) return -1;
    return (int)n.total;   // at most ~1.1 M floats (8 x 8 one-hot, 256 units: 64 cells x 3 planes x 8 tiles x 256)
}

int g2048_sized_pack(int size, const float* const* W, const float* const* b, int obs_mode, int n_hidden,
                     const int32_t* hidden, int out_dim, float* packed, int64_t packed_len, void* stream) {
    DeepNet n;
    if (size < 2 || size > 8) return pfail(G2048_EINVAL, "size must be in 2..8 (got " + std::to_string(size) + ")");
    if (!obs_ok(obs_mode)) return pfail(G2048_EINVAL, "sized policy: obs_mode must be log2, raw or onehot");
    if (!sized_layout(size, n_hidden, hidden, obs_mode == G2048_OBS_ONEHOT, n))
        return pfail(G2048_EINVAL, "sized policy: 1..4 hidden layers of 1..256 units");
    if (out_dim != 1 && out_dim != 4) return pfail(G2048_EINVAL, "sized policy: output width must be 4 or 1");
    if (!W || !b || !packed) return pfail(G2048_EINVAL, "sized policy: NULL buffer");
    if (packed_len < n.total) return pfail(G2048_EINVAL, "sized policy: packed buffer too small");
    SizedPackArgs a{};
    a.net = n;
    for (int l = 0; l <= n_hidden; l++) {
        if (!W[l] || !b[l]) return pfail(G2048_EINVAL, "sized policy: NULL weight");
        a.W[l] = W[l];
        a.B[l] = b[l];
    }
    for (int l = 0; l < n_hidden; l++) a.h[l] = hidden[l];
    a.out = out_dim;
    a.cells = size * size;
    a.dst = packed;
    const int grid = (int)((n.total + 255) / 256 < 4096 ? (n.total + 255) / 256 : 4096);
    hipLaunchKernelGGL(sized_pack_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
    return check_hip();
}

int g2048_sized_policy(int size, const float* packed, int n_hidden, const int32_t* hidden, int activation,
                       const uint64_t* boards, int64_t plane_stride, const uint32_t* lane_state,
                       const int32_t* lane_index, int obs_mode, float obs_scale, int use_mask, int greedy, int rng_mode,
                       uint64_t* rng_state, const uint64_t* rng_inc, const uint64_t* rng_buf, uint64_t philox_key,
                       const uint64_t* lane_seed, float* probs_out, float* logits_out, uint8_t* actions, int64_t n,
                       void* stream) {
    if (size < 2 || size > 8) return pfail(G2048_EINVAL, "size must be in 2..8 (got " + std::to_string(size) + ")");
    if (n < 0) return pfail(G2048_EINVAL, "n < 0");
    if (n > (int64_t(1) << 30)) return pfail(G2048_EINVAL, "n must be <= 2^30 per call");
    if (plane_stride < n)
        return pfail(G2048_EINVAL, "board plane_stride " + std::to_string(plane_stride) + " < " + std::to_string(n) +
                                       " lanes per plane");
    if (!obs_ok(obs_mode)) return pfail(G2048_EINVAL, "sized policy: obs_mode must be log2, raw or onehot");
    DeepNet net;
    if (!sized_layout(size, n_hidden, hidden, obs_mode == G2048_OBS_ONEHOT, net))
        return pfail(G2048_EINVAL, "sized policy: 1..4 hidden layers of 1..256 units");
    if (activation != G2048_ACT_RELU && activation != G2048_ACT_SIGMOID)
        return pfail(G2048_EINVAL, "Unsupported activation");
    if (rng_mode != G2048_RNG_PCG64 && rng_mode != G2048_RNG_PHILOX) return pfail(G2048_EINVAL, "Unsupported rng_mode");
    if (!packed || !boards || (!actions && !logits_out))
        return pfail(G2048_EINVAL, "sized policy: packed / boards and actions or logits_out are required");
    if (actions && !greedy && rng_mode == G2048_RNG_PCG64 && (!rng_state || !rng_inc || !rng_buf))
        return pfail(G2048_EINVAL, "PCG64 sampling needs rng_state / rng_inc / rng_buf");
    if (n == 0) return G2048_OK;
    SizedPolArgs a;
    a.net = net;
    a.packed = packed;
    a.boards = boards;
    a.bstride = plane_stride;
    a.lane_state = lane_state;
    a.lane_index = lane_index;
    a.rs = rng_state;
    a.inc = const_cast<uint64_t*>(rng_inc);
    a.buf = const_cast<uint64_t*>(rng_buf);
    a.key = philox_key;
    a.lane_seed = lane_seed;
    a.probs_out = probs_out;
    a.logits_out = logits_out;
    a.actions = actions;
    a.obs_scale = obs_scale;
    a.n = (uint32_t)n;
    a.size = size;
    a.use_mask = use_mask;
    a.greedy = greedy;
    const int64_t groups = (n + 31) / 32;
    const int64_t cap = 2 * (int64_t)device_cus();   // persistent: two workgroups per CU
    const int grid = (int)(groups < cap ? groups : cap);
    hipStream_t s = (hipStream_t)stream;
    if (obs_mode == G2048_OBS_ONEHOT) launch_sized_act<G2048_OBS_ONEHOT>(a, activation, rng_mode, grid, s);
    else if (obs_mode == G2048_OBS_LOG2) launch_sized_act<G2048_OBS_LOG2>(a, activation, rng_mode, grid, s);
    else launch_sized_act<G2048_OBS_RAW>(a, activation, rng_mode, grid, s);
    return check_hip();
}

}  // extern "C"
