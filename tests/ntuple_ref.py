"""Shared by tests/test_ntuple_host.py, tests/test_gpu_ntuple.py, tests/test_ntuple_sizes_cpu.py and
tests/test_gpu_ntuple_sizes.py: the TEST-ONLY host build of csrc/g2048_ntuple_core.h (tests/native/ntuple_host.cpp)
behind numpy wrappers, the fixture tests/golden/ntuple.npz (tests/golden/make_golden_ntuple.py) and networks rebuilt
from its hash seeds; for the two size tests, seeded inputs for every size 2..8 with the answers of
tests/ntuple_pyref.py computed once.  Not a test module."""
import ctypes
import functools
import json
import os
import subprocess

import numpy as np

import sized_ref as SR
from test_scripted_host import ScState
from test_sized_host import EpCfg, ep_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "rl-2048-with-reinforce-and-actor-critic_amd", "csrc")
INVALID = -(1 << 63)
BOARD_SIZES = (2, 3, 4, 5, 8)
FEATURE = np.dtype([("off", "<u4"), ("k", "<u4"), ("cells", "<u8")])     # ntuple::Feature


def _sources():
    return [os.path.join(NATIVE, "ntuple_host.cpp")] + [os.path.join(CSRC, h) for h in (
        "g2048_ntuple_core.h", "g2048_search_core.h", "g2048_scripted_core.h", "g2048_sized_core.h", "g2048_core.h")]


@functools.lru_cache(maxsize=None)
def host():
    """The host build, compiled on first use."""
    so = os.path.join(NATIVE, "libntuple_host.so")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in _sources()):
        tmp = f"{so}.{os.getpid()}.tmp"   # build aside, then rename: parallel workers never load a partial file
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I" + CSRC, "-o", tmp, _sources()[0]],
                       check=True)
        os.replace(tmp, so)
    L = ctypes.CDLL(so)
    vp, i32, i64, u32, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint64
    net = [vp, u32, vp]
    L.nt_values.argtypes = [i32, i32] + net + [vp, i64, vp]
    L.nt_choose.argtypes = [i32, i32, i32] + net + [vp, i64, vp, vp]
    L.nt_play.restype = i64
    L.nt_play.argtypes = [i32, i32, i32] + net + [ctypes.POINTER(EpCfg), i32, u64, u64, ctypes.POINTER(ScState), i64,
                                                   vp, vp, vp, vp]
    L.nt_td.argtypes = [i32, i32] + net + [vp, vp, vp, vp, i64, i64, ctypes.c_int32, ctypes.c_int32, vp]
    L.nt_td_step.restype = ctypes.c_int32
    L.nt_td_step.argtypes = [i64, ctypes.c_int32, ctypes.c_int32]
    L.nt_floor_div.restype = i64
    L.nt_floor_div.argtypes = [i64, i64]
    return L


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "ntuple.npz")) as z:
        return {k: z[k] for k in z.files}


def ep_cases():
    return json.loads(str(golden()["ep_cases"]))


def make_net(size, device="cpu", tuples=None, seed=None):
    """An NTupleNetwork with the fixture's hash weights for this size (seed: another hash seed; False: zeros)."""
    from rl2048_amd import NTupleNetwork

    net = NTupleNetwork(size, tuples, device=device)
    if seed is not False:
        net.fill_hash(int(golden()["hash_seed"][size]) if seed is None else seed)
    return net


def features_array(net) -> np.ndarray:
    """net.features as the host build reads them."""
    f = np.zeros(len(net.features), dtype=FEATURE)
    for i, (_, off, cells) in enumerate(net.features):
        f[i] = (off, len(cells), sum(c << (8 * j) for j, c in enumerate(cells)))
    return f


def _net_args(net, weights=None):
    f = features_array(net)
    w = np.ascontiguousarray(net.host_weights() if weights is None else weights, dtype=np.int32)
    return f, w, (f.ctypes.data, len(f), w.ctypes.data)


def host_values(net, native4, planes, weights=None):
    """V of [W, m] planes (int64 / uint64) through the host build."""
    planes = np.ascontiguousarray(planes).view(np.uint64).reshape(SR.words(net.size), -1)
    m = planes.shape[1]
    out = np.full(m, -7, dtype=np.int64)
    f, w, args = _net_args(net, weights)
    assert host().nt_values(net.size, int(native4), *args, planes.ctypes.data, m, out.ctypes.data) == 0
    return out


def host_choose(net, native4, depth, planes, weights=None):
    """The host build's choice on [W, m] planes: (actions uint8 [m], q int64 [m, 4])."""
    planes = np.ascontiguousarray(planes).view(np.uint64).reshape(SR.words(net.size), -1)
    m = planes.shape[1]
    acts = np.full(m, 255, dtype=np.uint8)
    q = np.full((m, 4), -7, dtype=np.int64)
    f, w, args = _net_args(net, weights)
    assert host().nt_choose(net.size, int(native4), depth, *args, planes.ctypes.data, m, acts.ctypes.data,
                            q.ctypes.data) == 0
    return acts, q


def host_play(net, native4, depth, env_kw, env_seed, pol_seed, chunk=16, most=1 << 16, weights=None):
    """One episode through the host build, `chunk` steps per call (the state carried the way the kernels' suspend
    protocol carries it): planes [W, T] uint64, actions, rewards, flags and the final ScState."""
    W = SR.words(net.size)
    cfg = ep_cfg(env_kw)
    st = ScState()
    f, w, args = _net_args(net, weights)
    boards, acts, rews, flags = [], [], [], []
    fresh = 1
    while True:
        b = np.zeros((chunk, W), dtype=np.uint64)
        a = np.zeros(chunk, dtype=np.uint8)
        r = np.zeros(chunk, dtype=np.float64)
        fl = np.zeros(chunk, dtype=np.uint8)
        k = host().nt_play(net.size, int(native4), depth, *args, ctypes.byref(cfg), fresh, env_seed, pol_seed,
                           ctypes.byref(st), chunk, b.ctypes.data, a.ctypes.data, r.ctypes.data, fl.ctypes.data)
        assert 1 <= k <= chunk
        boards.append(b[:k]); acts.append(a[:k]); rews.append(r[:k]); flags.append(fl[:k])
        fresh = 0
        if st.ended:
            break
        assert k == chunk and st.t < most
    out = (np.concatenate(boards).T.copy(), np.concatenate(acts), np.concatenate(rews), np.concatenate(flags), st)
    assert st.t == st.sc == len(out[1])
    return out


def host_td(net, native4, weights, planes, actions, flags, lengths, lr_num, lr_shift):
    """One update through the host build on [W, T, n] planes: (new weights int32, rows, sum |delta|); `weights` (the
    weights before) is not written."""
    T, n = actions.shape
    planes = np.ascontiguousarray(planes).view(np.uint64).reshape(SR.words(net.size), T, n)
    w = np.array(weights, dtype=np.int32, copy=True)
    f = features_array(net)
    stats = np.zeros(2, dtype=np.int64)
    acts, fl, ln = (np.ascontiguousarray(x, dtype=d) for x, d in ((actions, np.uint8), (flags, np.uint8),
                                                                  (lengths, np.int32)))
    assert host().nt_td(net.size, int(native4), f.ctypes.data, len(f), w.ctypes.data, planes.ctypes.data,
                        acts.ctypes.data, fl.ctypes.data, ln.ctypes.data, n, T, lr_num, lr_shift, stats.ctypes.data) == 0
    return w, int(stats[0]), int(stats[1])


def host_rollout(net, native4, depth, env_kw, env_seeds, pol_seeds, weights=None):
    """The episodes of these seeds through the host build as a time-major batch: planes [W, T, n] uint64, actions,
    flags (INACTIVE past an episode's end), lengths int32 and the fp64 totals."""
    eps = [host_play(net, native4, depth, env_kw, int(e), int(p), chunk=64, weights=weights)
           for e, p in zip(env_seeds, pol_seeds)]
    n, T, W = len(eps), max(len(ep[1]) for ep in eps), SR.words(net.size)
    planes = np.zeros((W, T, n), dtype=np.uint64)
    actions = np.zeros((T, n), dtype=np.uint8)
    flags = np.full((T, n), 0x40, dtype=np.uint8)
    for i, (b, a, _, f, _) in enumerate(eps):
        planes[:, :len(a), i], actions[:len(a), i], flags[:len(a), i] = b, a, f
    lengths = np.array([len(ep[1]) for ep in eps], dtype=np.int32)
    return planes, actions, flags, lengths, np.array([ep[4].total for ep in eps], dtype=np.float64)


def td_case(size):
    """A fixture TD case as a time-major batch: planes [W, T, n] uint64, actions [T, n], flags [T, n] (CHANGED on every
    row, TERMINATED on a terminated episode's last row, TRUNCATED on a truncated one's, INACTIVE past the end), lengths."""
    g = golden()
    P = f"td{size}_"
    lens = g[P + "length"].astype(np.int64)
    n, T = len(lens), int(lens.max())
    ex = np.zeros((T, n, size * size), dtype=np.uint8)
    actions = np.zeros((T, n), dtype=np.uint8)
    flags = np.full((T, n), 0x40, dtype=np.uint8)
    s = 0
    for i, L in enumerate(lens.tolist()):
        ex[:L, i] = g[P + "boards"][s:s + L]
        actions[:L, i] = g[P + "actions"][s:s + L]
        flags[:L, i] = 0x01
        flags[L - 1, i] |= 0x02 if g[P + "terminated"][i] else 0x04
        s += L
    planes = SR.pack_planes(ex.reshape(T * n, -1), size).reshape(SR.words(size), T, n)
    return planes, actions, flags, lens.astype(np.int32)


def td_expected(size, before):
    """The fixture's weights after the update of weights `before`."""
    g = golden()
    P = f"td{size}_"
    want = before.astype(np.int64)
    want[g[P + "pos"]] += g[P + "val"]
    return want.astype(np.int32), int(g[P + "rows"]), int(g[P + "abs_delta"])


# ------------------------------------------------------------------------------------------------------------------
# Inputs of tests/test_ntuple_sizes_cpu.py and tests/test_gpu_ntuple_sizes.py: every size 2..8 (BOARD_SIZES above keys
# the fixture and stays as it is), wide tuples, raw feature lists.  Everything is generated from a seed.
# ------------------------------------------------------------------------------------------------------------------
ALL_SIZES = (2, 3, 4, 5, 6, 7, 8)
# the two networks with 5- and 6-cell tuples: (size, base tuples); 16^6 + 16^5 + 16^2 and 16^6 + 16^5 weights
WIDE_NETS = {"N4-k6": (4, [(0, 1, 2, 3, 4, 5), (0, 1, 2, 4, 5), (5, 6)]),
             "N6-k6": (6, [(0, 1, 2, 6, 7, 8), (14, 15, 16, 20, 21)])}
# 16 base tuples = 128 features, the ABI's maximum: the 14 default tuples of N = 8 and two across word boundaries
FULL_NET = "N8-f128"
FULL_TUPLES = [(15, 16), (31, 32, 47, 48, 63)]
F_CHANGED, F_TERMINATED, F_TRUNCATED, F_INACTIVE = 0x01, 0x02, 0x04, 0x40


def features_of(net) -> list:
    """net.features as tests/ntuple_pyref.py reads them: [(offset, cells)]."""
    return [(off, tuple(cells)) for _, off, cells in net.features]


class RawNet:
    """A feature list written by hand, with no symmetry images, behind the attributes the host wrappers above read
    (size, features as (table, offset, cells), host_weights())."""

    def __init__(self, size, features, weights):
        self.size = size
        self.features = [(i, off, tuple(cells)) for i, (off, cells) in enumerate(features)]
        self.weights = np.ascontiguousarray(weights, dtype=np.int32)
        self.n_weights = len(self.weights)

    def host_weights(self):
        return self.weights


def raw_features(size: int, nf: int):
    """The first nf of 7 hand-written features on a size x size board (size >= 4): k = 3, 3, 2, 4, 6, 5, 2, the first
    two on one offset, cells spread over the board (across the word boundaries where there are any) and in no
    particular order.  Returns ([(offset, cells)], n_weights)."""
    last, mid = size * size - 1, size * size // 2
    cells = [(0, 5, last), (last, 1, size), (15, 2), (3, last - 1, 12, mid + 1), (last, 10, 0, 9, 4, last - 2),
             (6, 13, last - 3, 1, mid), (last - 1, 8)]
    offs, off = [], 0
    for i, c in enumerate(cells):
        assert len(set(c)) == len(c) and max(c) <= last
        if i == 1:
            offs.append(offs[0])                      # two features on one table
            continue
        offs.append(off)
        off += 16 ** len(c)
    feats = list(zip(offs, cells))[:nf]
    return feats, max(o + 16 ** len(c) for o, c in feats)


def random_weights(count: int, seed: int) -> np.ndarray:
    """int32 weights in the range of fill_hash's (-32768..32767)."""
    return np.random.default_rng(seed).integers(-32768, 32768, size=count, dtype=np.int32)


def _checker(size, lo=1, hi=2):
    r, c = np.indices((size, size))
    return np.where((r + c) % 2 == 0, lo, hi).reshape(-1)


def board_set(size: int, tuple_cells, count: int = 293, seed: int = 20480):
    """The board set of the size tests: (exponents uint8 [count, N*N], the indices of the depth-1 subset).  Crafted
    boards first -- a dead board, boards with exactly one valid action, a full board with one merge, a lone tile in a
    corner (its two moves tie by symmetry), tiles only in the cells on either side of each word boundary (15|16,
    31|32, 47|48 where the board has them), exponent 15 in every cell of `tuple_cells` alone and over a random fill --
    then random fills of 30..100 % with top exponents 3..15.  The depth-1 subset is the crafted boards and the first
    random ones."""
    cells = size * size
    rng = np.random.default_rng([seed, size])
    out = []
    out.append(_checker(size))                                         # dead: full, no equal neighbours
    b = np.zeros(cells, dtype=np.int64)
    b[cells - size:] = 1 + np.arange(size) % 2 * 2                     # bottom row full, no merge: only `up` is valid
    out.append(b)
    b = np.zeros(cells, dtype=np.int64)
    b[size - 1::size] = 2 + np.arange(size) % 2                        # right column full: only `left` is valid
    out.append(b)
    b = _checker(size, 3, 4)
    b[cells - 1] = b[cells - 2]                                        # full, one merge in the last row
    out.append(b)
    for cell in (0, cells - 1):
        b = np.zeros(cells, dtype=np.int64)
        b[cell] = 1
        out.append(b)
    for lo in (15, 31, 47):
        if lo + 1 < cells:
            for e in ((3, 5), (7, 7)):                                 # unequal, then equal (they merge across words)
                b = np.zeros(cells, dtype=np.int64)
                b[lo], b[lo + 1] = e
                out.append(b)
    b = np.zeros(cells, dtype=np.int64)
    b[list(tuple_cells)] = 15
    out.append(b)
    b = rng.integers(1, 8, size=cells)
    b[rng.random(cells) < 0.4] = 0
    b[list(tuple_cells)] = 15
    out.append(b)
    crafted = len(out)
    while len(out) < count:
        top, fill = int(rng.integers(3, 16)), rng.uniform(0.3, 1.0)
        b = rng.integers(1, top + 1, size=cells)
        b[rng.random(cells) >= fill] = 0
        out.append(b)
    ex = np.stack(out).astype(np.uint8)
    assert ex.shape == (count, cells) and count % 64 != 0
    return ex, np.arange(crafted + {2: 24, 3: 24, 4: 20, 5: 16, 6: 12, 7: 10, 8: 8}[size])


def td_batch(size: int, T: int = 7, n: int = 40, seed: int = 7):
    """A random time-major batch for the update: exponents 0..14 at about 60 % fill, random actions (so some recorded
    rows are invalid), random lengths 0..T with the entries 0, T, T + 3 (behaves as T) and -1 (as 0) among them, last
    rows terminated or truncated in turn.  Returns (ex uint8 [T, n, N*N], planes uint64 [W, T, n], actions, flags,
    lengths int32)."""
    rng = np.random.default_rng([seed, size, T, n])
    cells = size * size
    ex = rng.integers(1, 15, size=(T, n, cells))
    ex[rng.random((T, n, cells)) >= 0.6] = 0
    ex = ex.astype(np.uint8)
    actions = rng.integers(0, 4, size=(T, n)).astype(np.uint8)
    lengths = rng.integers(0, T + 1, size=n).astype(np.int32)
    lengths[:6] = (0, T, T + 3, -1, T, T + 3)
    flags = np.full((T, n), F_INACTIVE, dtype=np.uint8)
    for i in range(n):
        L = min(max(int(lengths[i]), 0), T)
        flags[:L, i] = F_CHANGED
        if L:
            flags[L - 1, i] |= F_TERMINATED if i % 3 else F_TRUNCATED
    planes = SR.pack_planes(ex.reshape(T * n, cells), size).view(np.uint64).reshape(SR.words(size), T, n)
    return ex, planes, actions, flags, lengths


@functools.lru_cache(maxsize=None)
def named_net(name):
    """The CPU network of a case: a size (the default tuples, the fixture's hash seed) or a key of WIDE_NETS."""
    if name in WIDE_NETS:
        size, tuples = WIDE_NETS[name]
        return make_net(size, tuples=tuples, seed=77 + size)
    if name == FULL_NET:
        from rl2048_amd import NTupleNetwork

        net = make_net(8, tuples=NTupleNetwork.default_tuples(8) + FULL_TUPLES, seed=85)
        assert len(net.features) == 128
        return net
    return make_net(name)


@functools.lru_cache(maxsize=None)
def size_case(name) -> dict:
    """The board set of a network (named_net) with tests/ntuple_pyref.py's answers, computed once and shared: ex, planes
    [W, m] uint64, i1 (the depth-1 subset), v, q0, a0, q1, a1, and the network's features / weights."""
    import ntuple_pyref as PR

    net = named_net(name)
    feats, w = features_of(net), net.host_weights()
    ex, i1 = board_set(net.size, net.tuples[0])
    q0, a0 = PR.q_values(feats, w, net.size, 0, ex)
    q1, a1 = PR.q_values(feats, w, net.size, 1, ex[i1])
    return dict(net=net, feats=feats, w=w, ex=ex, i1=i1, planes=SR.pack_planes(ex, net.size).view(np.uint64),
                v=PR.values(feats, w, ex), q0=q0, a0=a0, q1=q1, a1=a1)


@functools.lru_cache(maxsize=None)
def raw_case(size: int, nf: int) -> dict:
    """raw_features(size, nf) with random weights as a RawNet, its board set and a (7, 40) td_batch, with
    tests/ntuple_pyref.py's answers: v, q0 / a0 on every board, q1 / a1 on i1, td[(lr_num, lr_shift)] = td_update's."""
    import ntuple_pyref as PR

    feats, n_weights = raw_features(size, nf)
    w = random_weights(n_weights, 900 + nf)
    ex, i1 = board_set(size, feats[0][1])
    i1 = i1[::2]
    q0, a0 = PR.q_values(feats, w, size, 0, ex)
    q1, a1 = PR.q_values(feats, w, size, 1, ex[i1])
    bex, bplanes, actions, flags, lengths = td_batch(size)
    td = {lr: PR.td_update(feats, w, size, bex, actions, flags, lengths, *lr) for lr in ((1, 6), (65536, 0))}
    return dict(net=RawNet(size, feats, w), feats=feats, w=w, ex=ex, i1=i1, v=PR.values(feats, w, ex), q0=q0, a0=a0,
                q1=q1, a1=a1, planes=SR.pack_planes(ex, size).view(np.uint64), bplanes=bplanes, actions=actions,
                flags=flags, lengths=lengths, td=td)


@functools.lru_cache(maxsize=None)
def td_reference(name, lr_num, lr_shift, T=7, n=40) -> dict:
    """td_batch of a network (named_net) and tests/ntuple_pyref.py's update of it, computed once and shared: the batch,
    `before`, and `want` = (weights after, rows, sum |d|, info)."""
    import ntuple_pyref as PR

    net = named_net(name)
    ex, planes, actions, flags, lengths = td_batch(net.size, T, n)
    before = net.host_weights()
    want = PR.td_update(features_of(net), before, net.size, ex, actions, flags, lengths, lr_num, lr_shift)
    return dict(net=net, ex=ex, planes=planes, actions=actions, flags=flags, lengths=lengths, before=before, want=want)
