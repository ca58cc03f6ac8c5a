// g2048_ntuple_core.h -- the n-tuple value network (include/g2048_ntuple.h, rl2048_amd.NTupleNetwork / NTuplePolicy):
// the feature index, V, the players of depth 0 and 1, the sibling of episode_step that plays them and the per-row
// arithmetic of the TD(0) update, written once against the game interface of g2048_scripted_core.h (Game4 / GameN<N>).
// Shared by the gfx950 kernels (g2048_ntuple_kernel.h) and the CPU test harness (tests/native/ntuple_host.cpp,
// test-only).  Nothing here allocates or launches.
//
// The model, all in integers (so the host build, the kernels and the Python statement of it agree bit for bit):
//   g(b, a)    = the sum of the values of the tiles move(b, a) creates by merging            (MoveSummary::score)
//   F          = kFracBits = 10 fractional bits; a reward in value units is g << F
//   feature f  = (off, k, cells[k]); index_f(m) = sum_j e[cells[j]] 16^j
//   V(m)       = sum_f w[off_f + index_f(m)]                                                  (int64)
//   Q_0(b, a)  = (g(b, a) << F) + V(move(b, a))    for valid a (move(b, a) != b)
//   V'(s)      = max over valid a' of Q_0(s, a'), 0 when none is valid
//   Q_1(b, a)  = (g << F) + floor(sum over empty c of m [9 V'(m + 2 at c) + V'(m + 4 at c)] / (10 #empty(m)))
//   choice     = the valid action of the largest Q_depth(b, a), the lowest index among equals; 0 when none is valid
// Q may be negative: an invalid entry is INT64_MIN, and the chance node's division is a floor, not C's truncation.
//
// The device knows nothing of symmetry: the feature list holds every dihedral image.  It is wave-uniform (a pointer
// into the kernel's argument segment on the device), the loop over it is rolled, and a cell's exponent is fetched by
// shifting the board by a count read from the list -- no per-thread array is indexed by a run-time value.
#pragma once
#include "g2048_search_core.h"

namespace g2048 {
namespace ntuple {

constexpr int kFracBits = 10;             // include/g2048_ntuple.h: G2048_NTUPLE_FRAC_BITS
constexpr int kMaxDepth = 1;
constexpr int kMinCells = 2, kMaxCells = 6;
constexpr int kMaxFeatures = 128;
constexpr int32_t kMaxLrNum = 65536, kMaxLrShift = 40;
constexpr int64_t kStepClamp = (int64_t)1 << 30;
constexpr int64_t kInvalidQ = INT64_MIN;

// one feature as the loops read it: cell j in byte j of `cells` (bytes past k are 0)
struct Feature {
    uint32_t off, k;
    uint64_t cells;
};

#ifdef __HIP_DEVICE_COMPILE__
typedef const __attribute__((address_space(4))) Feature* FeaturePtr;    // the kernarg segment: scalar loads
#else
typedef const Feature* FeaturePtr;
#endif

struct Net {
    const int32_t* w;
    FeaturePtr f;
    uint32_t nf;
};

// move(b, a) with the score gain: the third piece of a step a value player needs (G::move returns only sum_e)
template <class G>
struct Slide;

template <>
struct Slide<scripted::Game4> {
    G2048_HDM bool run(const uint64_t (&bw)[1], uint32_t a, uint64_t (&out)[1], uint32_t& score) {
        MoveSummary s;
        out[0] = board_move_alu<false>(bw[0], a, s);
        score = s.score;
        return out[0] != bw[0];
    }
};

template <int N>
struct Slide<scripted::GameN<N>> {
    G2048_HDM bool run(const uint64_t (&bw)[sized::Dim<N>::kWords], uint32_t a,
                       uint64_t (&out)[sized::Dim<N>::kWords], uint32_t& score) {
        MoveSummary s;
        const sized::Board<N> m = sized::board_move<N, false>(scripted::GameN<N>::load(bw), a, s, nullptr);
        bool changed = false;
#pragma unroll
        for (int w = 0; w < sized::Dim<N>::kWords; w++) {
            out[w] = m.w[w];
            changed = changed || m.w[w] != bw[w];
        }
        score = s.score;
        return changed;
    }
};

// The exponent of `cell` (uniform).  Every word is shifted by the nibble's offset and masked by "this is the cell's
// word" (0 or 15): a chain of selects between the words is what the optimiser turns back into a run-time index into
// a per-thread array, which it then places in LDS (seen at N >= 6, W >= 3).
template <int W>
G2048_HD uint32_t cell_exponent(const uint64_t (&b)[W], uint32_t cell) {
    const uint32_t sh = 4u * (cell & 15u), word = cell >> 4;
    uint32_t e = 0;
#pragma unroll
    for (int w = 0; w < W; w++) e |= (uint32_t)(b[w] >> sh) & (W == 1 || word == (uint32_t)w ? 15u : 0u);
    return e;
}

// index_f(b)
template <int W>
G2048_HD uint32_t feature_index(const uint64_t (&b)[W], uint32_t k, uint64_t cells) {
    uint32_t idx = 0;
#pragma unroll
    for (int j = 0; j < kMaxCells; j++) {
        const uint32_t e = cell_exponent<W>(b, (uint32_t)(cells >> (8 * j)) & 63u);
        idx |= (uint32_t)j < k ? e << (4 * j) : 0u;
    }
    return idx;
}

// V(b)
template <class G>
G2048_HD int64_t value(const uint64_t (&b)[G::kWords], const Net& net) {
    int64_t v = 0;
#pragma unroll 4
    for (uint32_t f = 0; f < net.nf; f++) {
        const uint32_t off = net.f[f].off, k = net.f[f].k;
        const uint64_t cells = net.f[f].cells;
        v += (int64_t)net.w[(size_t)off + feature_index<G::kWords>(b, k, cells)];
    }
    return v;
}

// floor(a / d), d > 0
G2048_HD int64_t floor_div(int64_t a, int64_t d) {
    const int64_t q = a / d;
    return (a % d != 0 && a < 0) ? q - 1 : q;
}

template <class G, int D>
G2048_HD bool q_value(const uint64_t (&b)[G::kWords], uint32_t a, const Net& net, int64_t& q);

// V'(s): the best Q_0 of s, 0 when no action is valid
template <class G>
G2048_HD int64_t best_q0(const uint64_t (&s)[G::kWords], const Net& net) {
    int64_t best = 0;
    bool any = false;
#pragma unroll 1
    for (uint32_t a = 0; a < 4; a++) {
        int64_t q;
        if (q_value<G, 0>(s, a, net, q)) {
            best = (!any || q > best) ? q : best;
            any = true;
        }
    }
    return best;
}

// the chance layer over the afterstate m
template <class G>
G2048_HD int64_t chance(const uint64_t (&m)[G::kWords], const Net& net) {
    constexpr int W = G::kWords;
    constexpr sized::Masks<G::kSize> M = sized::make_masks<G::kSize>();
    uint64_t z[W];
    uint32_t ne = 0;
#pragma unroll
    for (int i = 0; i < W; i++) {
        z[i] = ~nz_bits(m[i]) & M.cell[i];
        ne += (uint32_t)popc64(z[i]);
    }
    int64_t tot = 0;
#pragma unroll 1
    for (uint32_t i = 0; i < ne; i++) {
        const uint32_t cell = search::take_empty<W>(z);
#pragma unroll 1
        for (uint32_t e = 1; e <= 2; e++) {      // a 2 with weight 9, a 4 with weight 1
            uint64_t c[W];
#pragma unroll
            for (int k = 0; k < W; k++) c[k] = m[k];
            G::put(c, cell, e);
            tot += (int64_t)(e == 1u ? 9 : 1) * best_q0<G>(c, net);
        }
    }
    return ne ? floor_div(tot, (int64_t)(10u * ne)) : 0;   // a valid move always leaves an empty cell
}

// Q_D(b, a) into q; false (q untouched) for an invalid a
template <class G, int D>
G2048_HD bool q_value(const uint64_t (&b)[G::kWords], uint32_t a, const Net& net, int64_t& q) {
    static_assert(D >= 0 && D <= kMaxDepth, "depth 0 or 1");
    uint64_t m[G::kWords];
    uint32_t score;
    if (!Slide<G>::run(b, a, m, score)) return false;
    const int64_t r = (int64_t)((uint64_t)score << kFracBits);
    if constexpr (D == 0) {
        q = r + value<G>(m, net);
    } else {
        q = r + chance<G>(m, net);
    }
    return true;
}

// The choice on board b at depth D: q[a] = Q_D(b, a), kInvalidQ for an invalid a; returns the valid action of the
// largest q (the lowest index among equals), 0 when no action is valid.
template <class G, int D>
G2048_HD uint32_t choose(const uint64_t (&b)[G::kWords], const Net& net, int64_t (&q)[4]) {
    uint32_t act = 0;
    int64_t best = 0;
    bool any = false;
#pragma unroll
    for (int k = 0; k < 4; k++) q[k] = kInvalidQ;
#pragma unroll 1
    for (uint32_t a = 0; a < 4; a++) {
        int64_t v;
        if (q_value<G, D>(b, a, net, v)) {
#pragma unroll
            for (int k = 0; k < 4; k++) q[k] = a == (uint32_t)k ? v : q[k];
            const bool better = !any || v > best;
            act = better ? a : act;
            best = better ? v : best;
            any = true;
        }
    }
    return act;
}

// choose for a depth known at run time (0..kMaxDepth; the caller has checked it)
template <class G>
G2048_HD uint32_t choose_at(int depth, const uint64_t (&b)[G::kWords], const Net& net, int64_t (&q)[4]) {
    return depth == 0 ? choose<G, 0>(b, net, q) : choose<G, 1>(b, net, q);
}

// episode_step (g2048_scripted_core.h) for the network's player: the choice is computed from the board alone -- no
// action mask is read, so it plays with use_action_mask on or off, and it is always a valid action -- and the policy
// stream is not touched.
template <class G, int D>
G2048_HD bool episode_step(scripted::Episode<G>& e, const Net& net, const RewardCfg& rc, int64_t max_steps,
                           scripted::Row<G>& row) {
    int64_t q[4];
    const uint32_t act = choose<G, D>(e.bw, net, q);
#pragma unroll
    for (int k = 0; k < G::kWords; k++) row.bw[k] = e.bw[k];
    G::step(e.bw, act, e.sc, e.mt, e.ge, rc, max_steps, row.reward, row.flags);
    row.action = act;
    e.sc += 1u;
    e.t += 1u;
    e.total += row.reward;
    return (row.flags & (kFTerminated | kFTruncated)) != 0u;
}

// ---------------------------------------------------------------------------------------------------------------
// TD(0) on afterstates, per row.  Pass 1 (td_row_values) reads the weights and writes v = V(m_t) and
// q = (g_t << F) + V(m_t); pass 2 (td_target, td_step, td_apply) reads those and only adds to the weights.
// ---------------------------------------------------------------------------------------------------------------

// m = move(b, a) (b itself for an invalid recorded action, whose gain is 0), v and q of the row
template <class G>
G2048_HD void td_row_values(const uint64_t (&b)[G::kWords], uint32_t a, const Net& net, uint64_t (&m)[G::kWords],
                            int64_t& v, int64_t& q) {
    uint32_t score;
    Slide<G>::run(b, a & 3u, m, score);      // unchanged board: no merge, score 0
    v = value<G>(m, net);
    q = (int64_t)((uint64_t)score << kFracBits) + v;
}

// the target of row t of an episode of `len` rows: false when the row is skipped (a truncated last row)
G2048_HD bool td_target(uint32_t t, uint32_t len, uint32_t flags, int64_t q_next, int64_t& y) {
    if (t + 1u < len) {
        y = q_next;
        return true;
    }
    y = 0;
    return (flags & kFTerminated) != 0u;
}

// clamp(floor(delta lr_num / 2^lr_shift), -2^30, 2^30): an arithmetic shift of the int64 product
G2048_HD int32_t td_step(int64_t delta, int32_t lr_num, int32_t lr_shift) {
    const int64_t s = (delta * (int64_t)lr_num) >> lr_shift;
    return (int32_t)(s < -kStepClamp ? -kStepClamp : s > kStepClamp ? kStepClamp : s);
}

// w[off_f + index_f(m)] += step for every feature, through add(int32_t*, int32_t): a wrapping int32 add (atomic on
// the device).  Features that hit the same entry add twice.
template <class G, class Add>
G2048_HD void td_apply(const uint64_t (&m)[G::kWords], const Net& net, int32_t* w, int32_t step, const Add& add) {
#pragma unroll 4
    for (uint32_t f = 0; f < net.nf; f++) {
        const uint32_t off = net.f[f].off, k = net.f[f].k;
        const uint64_t cells = net.f[f].cells;
        add(w + (size_t)off + feature_index<G::kWords>(m, k, cells), step);
    }
}

}  // namespace ntuple
}  // namespace g2048
