// g2048_ntuple_kernel.h -- the kernels of the n-tuple value network (include/g2048_ntuple.h), their argument checks and
// their launches, shared by the two translation units that instantiate them: g2048_ntuple.hip (the 4 x 4 game) and
// g2048_sized_ntuple.hip (sizes 2..8).  The per-step and per-row code is g2048_ntuple_core.h, the code the CPU tests
// run.
//
// ntuple_kernel: scripted_kernel's loop (play_episodes of g2048_scripted_kernel.h, with that file's argument checks and
// grid) with the network's player: one episode per lane, persistent, 256 threads = 4 waves that never talk to each
// other, no LDS, no barrier.  Termination: as scripted_kernel -- every live lane advances its episode by one step per
// iteration (the choice is a bounded loop nest) and gives it up by termination, truncation or suspension at `cap`.
// ntuple_choose_kernel / ntuple_values_kernel: one board per thread.
// ntuple_td_values_kernel / ntuple_td_apply_kernel: the TD(0) update in two passes over the [T, n] rows, one row per
// thread in a grid-stride loop.  Pass 1 reads the weights and writes V(m_t) and (g_t << F) + V(m_t) of every row to
// scratch; pass 2 reads scratch, never a weight, and adds step_t to the 8B entries of the row with int32 atomics.  The
// two launches are ordered by the stream, so no V of a call sees a write of that call; integer adds commute, so the
// weights do not depend on the order in which the atomics arrive.
//
// Roofline (an estimate from the loop nests; the measured rates are in DESIGN.md section 3):
//   gathers    a depth-0 step evaluates V on up to 4 afterstates: 4 x 8B four-byte gathers (160 at N = 4) beside 4
//              moves, against two stores per step.  A depth-1 step is 4 + 4 * 2 E * 4 afterstates with E empty cells:
//              up to 8 E times the gathers.  A TD row is 8B gathers in pass 1 and up to 8B atomics in pass 2.
//   tables     1.25 MiB of weights at the default tuples of N = 4 and up to 3.5 MiB at N = 8, against 4 MiB of L2 per
//              XCD: after the first touches the gathers are L2 hits (Infinity Cache at worst), never HBM streams.  The
//              feature list (at most 2 KiB) is read from the kernel's argument segment with scalar loads.
//   bound      latency of dependent gathers, not bandwidth: a gather returns one dword of a 128-byte line.  The loop
//              over features is unrolled by 4 so that four gathers are in flight per lane.
//   hot spot   the update's atomics: many rows add to the few entries of mostly-empty tuples (early boards hold two or
//              three tiles, so most features read index 0 or one small exponent), which is same-address contention in
//              L2.  Done about it: a row whose step is 0 issues no atomics.  Equal addresses are NOT combined within
//              a wave before the atomic; DESIGN.md section 3 measures what the contention costs against a batch of
//              shuffled random fills.
#pragma once
#include <stddef.h>

#include "g2048_ntuple_core.h"
#include "g2048_scripted_kernel.h"

namespace {

static_assert(ntuple::kFracBits == G2048_NTUPLE_FRAC_BITS && ntuple::kMaxDepth == G2048_NTUPLE_MAX_DEPTH &&
                  ntuple::kMinCells == G2048_NTUPLE_MIN_CELLS && ntuple::kMaxCells == G2048_NTUPLE_MAX_CELLS &&
                  ntuple::kMaxFeatures == G2048_NTUPLE_MAX_FEATURES && ntuple::kMaxLrNum == G2048_NTUPLE_MAX_LR_NUM &&
                  ntuple::kMaxLrShift == G2048_NTUPLE_MAX_LR_SHIFT,
              "ntuple limits");

// the network as a kernel argument: the weights and the checked, packed feature list
struct NtNet {
    int32_t* w;
    uint32_t nf, pad;
    ntuple::Feature feat[ntuple::kMaxFeatures];
};

// ScriptArgs first, so that args_per_lane() (the kernarg segment read as a ScriptArgs at offset 0) serves this kernel
struct NtArgs {
    ScriptArgs s;       // s.script is not read
    NtNet net;
};

struct NtBoardArgs {    // choose / values
    NtNet net;
    const uint64_t* boards;
    uint32_t n;
    uint8_t* actions;
    int64_t* q;         // choose: [n, 4] or NULL; values: [n]
};

struct NtTdArgs {
    NtNet net;
    const uint64_t* boards;
    int64_t bstride;    // elements between two board planes
    const uint8_t* actions;
    const uint8_t* flags;
    const int32_t* lengths;
    uint32_t n, T;
    int32_t lr_num, lr_shift;
    int64_t* scratch;   // [2, T n]: V(m_t), then (g_t << F) + V(m_t)
    int64_t* stats;     // rows updated, sum |d_t|
};

// The network of a kernel whose argument struct holds an NtNet at byte OFF: the feature list is read where the
// dispatch put it, through a constant-address-space pointer (uniform index, scalar loads).
template <size_t OFF>
__device__ __forceinline__ ntuple::Net kernarg_net() {
    typedef const __attribute__((address_space(4))) char* Bytes;
    typedef const __attribute__((address_space(4))) NtNet* NetPtr;
    const NetPtr p = (NetPtr)((Bytes)__builtin_amdgcn_kernarg_segment_ptr() + OFF);
    return ntuple::Net{p->w, (ntuple::FeaturePtr)p->feat, p->nf};
}

// The network's player of depth D for play_episodes: the policy stream is neither read nor written.
template <class G, int D>
struct NTuplePlayer {
    const NtArgs& a;
    __device__ __forceinline__ bool policy_stream() const { return false; }
    __device__ __forceinline__ bool step(scripted::Episode<G>& e, scripted::Row<G>& row) const {
        return ntuple::episode_step<G, D>(e, kernarg_net<offsetof(NtArgs, net)>(), a.s.rc, a.s.max_steps, row);
    }
};

template <class G, int D, bool TRAJ>
__global__ void __launch_bounds__(kScriptBlock) ntuple_kernel(NtArgs a) {
    play_episodes<G, TRAJ>(NTuplePlayer<G, D>{a});
}

// One board per thread: boards are [W, n] planes of stride n (W = 1: n bitboards); q may be NULL.
template <class G, int D>
__global__ void __launch_bounds__(kScriptBlock) ntuple_choose_kernel(NtBoardArgs a) {
    const uint32_t i = blockIdx.x * (uint32_t)kScriptBlock + threadIdx.x;
    if (i >= a.n) return;
    uint64_t b[G::kWords];
#pragma unroll
    for (int k = 0; k < G::kWords; k++) b[k] = a.boards[(size_t)k * a.n + i];
    int64_t qv[4];
    a.actions[i] = (uint8_t)ntuple::choose<G, D>(b, kernarg_net<offsetof(NtBoardArgs, net)>(), qv);
    if (a.q) {
#pragma unroll
        for (int k = 0; k < 4; k++) a.q[4 * (size_t)i + k] = qv[k];
    }
}

template <class G>
__global__ void __launch_bounds__(kScriptBlock) ntuple_values_kernel(NtBoardArgs a) {
    const uint32_t i = blockIdx.x * (uint32_t)kScriptBlock + threadIdx.x;
    if (i >= a.n) return;
    uint64_t b[G::kWords];
#pragma unroll
    for (int k = 0; k < G::kWords; k++) b[k] = a.boards[(size_t)k * a.n + i];
    a.q[i] = ntuple::value<G>(b, kernarg_net<offsetof(NtBoardArgs, net)>());
}

// TD pass 1: row r = t n + i of an episode's first lengths[i] rows -> scratch[r] = V(m_t), scratch[T n + r] =
// (g_t << F) + V(m_t).  Rows past an episode's end are not touched (pass 2 does not read them).
template <class G>
__global__ void __launch_bounds__(kScriptBlock) ntuple_td_values_kernel(NtTdArgs a) {
    const ntuple::Net net = kernarg_net<offsetof(NtTdArgs, net)>();
    const size_t rows = (size_t)a.T * a.n, stride = (size_t)gridDim.x * kScriptBlock;
    for (size_t r = (size_t)blockIdx.x * kScriptBlock + threadIdx.x; r < rows; r += stride) {
        const uint32_t t = (uint32_t)(r / a.n), i = (uint32_t)(r % a.n);
        const int32_t len = a.lengths[i];
        if (len < 0 || t >= (uint32_t)len) continue;
        uint64_t b[G::kWords], m[G::kWords];
#pragma unroll
        for (int k = 0; k < G::kWords; k++) b[k] = a.boards[(size_t)k * (size_t)a.bstride + r];
        int64_t v, q;
        ntuple::td_row_values<G>(b, a.actions[r], net, m, v, q);
        a.scratch[r] = v;
        a.scratch[rows + r] = q;
    }
}

struct AtomicAddI32 {
    __device__ __forceinline__ void operator()(int32_t* p, int32_t v) const { atomicAdd(p, v); }
};

// TD pass 2: the row's target from scratch, its step, and the adds; the count and sum |d| are reduced over the wave
// (every lane of a wave runs the same number of iterations) and added to stats once per wave.
template <class G>
__global__ void __launch_bounds__(kScriptBlock) ntuple_td_apply_kernel(NtTdArgs a) {
    const ntuple::Net net = kernarg_net<offsetof(NtTdArgs, net)>();
    const size_t rows = (size_t)a.T * a.n, stride = (size_t)gridDim.x * kScriptBlock;
    unsigned long long cnt = 0, sum = 0;
    for (size_t base = (size_t)blockIdx.x * kScriptBlock; base < rows; base += stride) {
        const size_t r = base + threadIdx.x;
        if (r >= rows) continue;
        const uint32_t t = (uint32_t)(r / a.n), i = (uint32_t)(r % a.n);
        const int32_t len0 = a.lengths[i];
        const uint32_t len = len0 < 0 ? 0u : (uint32_t)len0 > a.T ? a.T : (uint32_t)len0;
        if (t >= len) continue;
        const int64_t q_next = t + 1u < len ? a.scratch[rows + r + a.n] : 0;
        int64_t y;
        if (!ntuple::td_target(t, len, a.flags[r], q_next, y)) continue;
        const int64_t d = y - a.scratch[r];
        cnt += 1ull;
        sum += (unsigned long long)(d < 0 ? -d : d);
        const int32_t step = ntuple::td_step(d, a.lr_num, a.lr_shift);
        if (step == 0) continue;
        uint64_t b[G::kWords], m[G::kWords];
#pragma unroll
        for (int k = 0; k < G::kWords; k++) b[k] = a.boards[(size_t)k * (size_t)a.bstride + r];
        uint32_t score;
        ntuple::Slide<G>::run(b, (uint32_t)a.actions[r] & 3u, m, score);
        ntuple::td_apply<G>(m, net, a.net.w, step, AtomicAddI32{});
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        cnt += __shfl_down(cnt, off, 64);
        sum += __shfl_down(sum, off, 64);
    }
    if ((threadIdx.x & 63) == 0 && cnt != 0ull) {
        atomicAdd((unsigned long long*)a.stats, cnt);
        atomicAdd((unsigned long long*)a.stats + 1, sum);
    }
}

// The descriptor's checks (every one precedes every HIP call) and the packed network.  size: the board's N.
int ntuple_net(const char* who, const g2048_ntuple* nt, int size, NtNet& out) {
    const std::string p = std::string(who) + ": ";
    if (!nt) return sfail(G2048_EINVAL, p + "net is NULL");
    if (nt->depth < 0 || nt->depth > G2048_NTUPLE_MAX_DEPTH)
        return sfail(G2048_EINVAL, p + "depth must be in 0..1 (got " + std::to_string(nt->depth) + ")");
    if (nt->n_features < 1 || nt->n_features > G2048_NTUPLE_MAX_FEATURES)
        return sfail(G2048_EINVAL, p + "n_features must be in 1..128 (got " + std::to_string(nt->n_features) + ")");
    if (!nt->features || !nt->weights) return sfail(G2048_EINVAL, p + "net->features or net->weights is NULL");
    if (nt->n_weights < 1) return sfail(G2048_EINVAL, p + "n_weights < 1");
    const uint32_t cells_n = (uint32_t)(size * size);
    out = NtNet{};
    out.w = nt->weights;
    out.nf = (uint32_t)nt->n_features;
    for (int f = 0; f < nt->n_features; f++) {
        const g2048_ntuple_feature& ft = nt->features[f];
        const std::string pf = p + "feature " + std::to_string(f) + ": ";
        if (ft.k < G2048_NTUPLE_MIN_CELLS || ft.k > G2048_NTUPLE_MAX_CELLS)
            return sfail(G2048_EINVAL, pf + "k must be in 2..6 (got " + std::to_string((int)ft.k) + ")");
        uint64_t seen = 0, cells = 0;
        for (int j = 0; j < ft.k; j++) {
            if (ft.cells[j] >= cells_n) return sfail(G2048_EINVAL, pf + "cell " + std::to_string((int)ft.cells[j]) +
                                                                       " is outside the board");
            if ((seen >> ft.cells[j]) & 1ull) return sfail(G2048_EINVAL, pf + "a cell is repeated");
            seen |= 1ull << ft.cells[j];
            cells |= (uint64_t)ft.cells[j] << (8 * j);
        }
        if ((int64_t)ft.offset + ((int64_t)1 << (4 * ft.k)) > nt->n_weights)
            return sfail(G2048_EINVAL, pf + "offset + 16^k is beyond n_weights");
        out.feat[f] = ntuple::Feature{ft.offset, ft.k, cells};
    }
    return G2048_OK;
}

// The network's checks, then script_args' for everything the scripted entry points check besides the script: they run
// on a UNIFORM script, the kind that asks nothing of the config.
int ntuple_args(const char* who, int size, const g2048_ntuple* nt, const g2048_env_cfg* cfg, uint64_t* env_state,
                const uint64_t* env_inc, uint64_t* env_buf, uint64_t* pol_state, const uint64_t* pol_inc,
                uint64_t* pol_buf, uint32_t* queue, const int32_t* order, int64_t n_order, int resume,
                const g2048_suspend* sus, int64_t n, int64_t cap, bool rows, const g2048_traj* traj, int64_t board_stride,
                const g2048_eval_out* out, int max_workgroups, NtArgs& a) {
    const int rc = ntuple_net(who, nt, size, a.net);
    if (rc) return rc;
    const g2048_script any = {G2048_SCRIPT_UNIFORM, {0, 1, 2, 3}};
    return script_args(who, &any, cfg, env_state, env_inc, env_buf, pol_state, pol_inc, pol_buf, queue, order, n_order,
                       resume, sus, n, cap, rows, traj, board_stride, out, max_workgroups, a.s);
}

int launched() {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? G2048_OK : sfail(G2048_EHIP, hipGetErrorString(e));
}

template <class G, bool TRAJ>
int launch_ntuple(int depth, const NtArgs& a, int max_workgroups, void* stream) {
    const dim3 grid(script_grid(a.s.n_order, max_workgroups)), block(kScriptBlock);
    if (depth == 0) {
        hipLaunchKernelGGL((ntuple_kernel<G, 0, TRAJ>), grid, block, 0, (hipStream_t)stream, a);
    } else {
        hipLaunchKernelGGL((ntuple_kernel<G, 1, TRAJ>), grid, block, 0, (hipStream_t)stream, a);
    }
    return launched();
}

// the checks of the choose / values entry points, before any HIP call (`out`: actions or values)
int board_args(const char* who, int size, const g2048_ntuple* nt, const uint64_t* boards, int64_t n, const void* out,
               NtBoardArgs& a) {
    const int rc = ntuple_net(who, nt, size, a.net);
    if (rc) return rc;
    if (n < 0 || n > (int64_t)0x7FFFFFFF) return sfail(G2048_EINVAL, std::string(who) + ": n out of range");
    if (!boards || !out) return sfail(G2048_EINVAL, std::string(who) + ": a required buffer is NULL");
    a.boards = boards;
    a.n = (uint32_t)n;
    return G2048_OK;
}

template <class G>
int launch_nt_choose(int depth, const NtBoardArgs& a, void* stream) {
    const dim3 grid((unsigned)((a.n + (uint32_t)kScriptBlock - 1u) / (uint32_t)kScriptBlock)), block(kScriptBlock);
    if (depth == 0) {
        hipLaunchKernelGGL((ntuple_choose_kernel<G, 0>), grid, block, 0, (hipStream_t)stream, a);
    } else {
        hipLaunchKernelGGL((ntuple_choose_kernel<G, 1>), grid, block, 0, (hipStream_t)stream, a);
    }
    return launched();
}

template <class G>
int launch_nt_values(const NtBoardArgs& a, void* stream) {
    const dim3 grid((unsigned)((a.n + (uint32_t)kScriptBlock - 1u) / (uint32_t)kScriptBlock)), block(kScriptBlock);
    hipLaunchKernelGGL((ntuple_values_kernel<G>), grid, block, 0, (hipStream_t)stream, a);
    return launched();
}

// the checks of the two update entry points, before any HIP call; rows = T n
int td_args(const char* who, int size, const g2048_ntuple* nt, const uint64_t* boards, int64_t board_stride,
            const uint8_t* actions, const uint8_t* flags, const int32_t* lengths, int64_t n, int64_t T, int32_t lr_num,
            int32_t lr_shift, int64_t* scratch, int64_t* stats, NtTdArgs& a) {
    const std::string p = std::string(who) + ": ";
    const int rc = ntuple_net(who, nt, size, a.net);
    if (rc) return rc;
    if (lr_num < 1 || lr_num > G2048_NTUPLE_MAX_LR_NUM) return sfail(G2048_EINVAL, p + "lr_num must be in 1..65536");
    if (lr_shift < 0 || lr_shift > G2048_NTUPLE_MAX_LR_SHIFT) return sfail(G2048_EINVAL, p + "lr_shift must be in 0..40");
    if (n < 0 || n > (int64_t)0x7FFFFFFF || T < 0 || T > (int64_t)0x7FFFFFFF || n * T > ((int64_t)1 << 40))
        return sfail(G2048_EINVAL, p + "n or T out of range");
    if (board_stride < n * T) return sfail(G2048_EINVAL, p + "board_stride < T * n");
    if (!boards || !actions || !flags || !lengths || !scratch || !stats)
        return sfail(G2048_EINVAL, p + "a required buffer is NULL");
    a.boards = boards;
    a.bstride = board_stride;
    a.actions = actions;
    a.flags = flags;
    a.lengths = lengths;
    a.n = (uint32_t)n;
    a.T = (uint32_t)T;
    a.lr_num = lr_num;
    a.lr_shift = lr_shift;
    a.scratch = scratch;
    a.stats = stats;
    return G2048_OK;
}

template <class G>
int launch_td(const NtTdArgs& a, void* stream) {
    const hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(a.stats, 0, 2 * sizeof(int64_t), s);
    if (e != hipSuccess) return sfail(G2048_EHIP, hipGetErrorString(e));
    const int64_t rows = (int64_t)a.T * a.n;
    int64_t blocks = (rows + kScriptBlock - 1) / kScriptBlock;
    const int64_t most = 32 * (int64_t)device_cus();      // a grid-stride loop takes the rest
    if (blocks > most) blocks = most;
    const dim3 grid((unsigned)blocks), block(kScriptBlock);
    hipLaunchKernelGGL((ntuple_td_values_kernel<G>), grid, block, 0, s, a);
    int rc = launched();
    if (rc) return rc;
    hipLaunchKernelGGL((ntuple_td_apply_kernel<G>), grid, block, 0, s, a);
    return launched();
}

}  // namespace
