"""CPU: the host driver of the persistent rollout / evaluation launches (rl2048_amd.rollouts) on CPU tensors, around a
fake `launch` that plays a persistent kernel's part from a list of episode lengths: which launches the loops make
(order, count, resume flag, row capacity / step limit), how the trajectory rows grow and what they keep, the two
episode lists, and both refusals with their texts.  The kernels behind the real launches are tested on the GPU
(tests/test_gpu_rollout_replay.py, test_gpu_deep.py, test_gpu_sized_rollout.py, test_gpu_eval.py, test_gpu_scripted.py).
"""
import pytest
import torch

CPU = torch.device("cpu")
ENDLESS = 1 << 40
HINT = "set max_steps"
NO_LIMIT = dict(max_rows=1 << 24, free_bytes=lambda: 1 << 62, hint=HINT)


class FakeKernel:
    """launch(order, n_order, resume, sus, limit) as a persistent kernel answers it: every episode named by `order`
    (0..n_order-1 without one) plays on from where it stopped until its length or `limit` steps in all; a finished one
    gets its length written, the others are suspended (ids into the list the launch was given, their count beside).
    With rows it writes row t of episode i as action t + 1, reward t + i / 8, flags 0, board 1000 i + t (+ plane)."""

    def __init__(self, lengths, outs, rows=None):
        self.full, self.outs, self.rows = list(lengths), outs, rows
        self.done = [0] * len(self.full)
        self.calls, self.orders, self.strides = [], [], []

    def __call__(self, order, n_order, resume, sus, limit):
        assert (order is None) == (resume == 0)
        ids = list(range(n_order)) if order is None else order[:n_order].tolist()
        self.calls.append((n_order, resume, limit))
        self.orders.append(None if order is None else ids)
        rows = self.rows
        if rows is not None:
            assert limit == rows.cap == rows.actions.shape[0]
            self.strides.append(rows.plane_stride)
        if sus is not None:
            fill = sus.list
            assert sus.struct().list == fill.data_ptr() and sus.struct().count == sus.count.data_ptr()
            assert order is None or order.data_ptr() != fill.data_ptr()     # never reads the list it fills
            assert int(sus.count) == 0
        suspended = []
        for i in ids:
            for t in range(self.done[i], min(self.full[i], limit)):
                if rows is not None:
                    rows.actions[t, i], rows.rewards[t, i], rows.flags[t, i] = t + 1, t + i / 8, 0
                    if rows.W is None:
                        rows.boards[t, i] = 1000 * i + t
                    else:
                        rows.boards[:, t, i] = 1000 * i + t + torch.arange(rows.W) * 10 ** 6
            self.done[i] = min(self.full[i], limit)
            if self.done[i] < self.full[i]:
                suspended.append(i)
            else:
                self.outs.lengths[i] = self.done[i]
        if suspended:
            assert sus is not None, "an episode outlived the only launch of a family that suspends none"
            fill[:len(suspended)] = torch.tensor(suspended, dtype=torch.int32)
            sus.count[0] = len(suspended)


def _growing(lengths, first_cap, max_steps=None, W=None, probs=False, suspends=True, **limits):
    from rl2048_amd import rollouts as R

    n = len(lengths)
    outs, rows = R.EpisodeOutputs(n, CPU, W), R.TrajectoryRows(n, CPU, W, probs=probs, cap=first_cap)
    sus = R.SuspendState(n, CPU, W) if suspends else None
    kernel = FakeKernel(lengths, outs, rows)
    queue = torch.ones(1, dtype=torch.int32)
    run = lambda: R.run_growing(kernel, rows, outs, sus, queue, n, max_steps, **dict(NO_LIMIT, **limits))  # noqa: E731
    return run, kernel, rows, outs, queue


def _check_rows(rows_of, lengths, T, W=None):
    """Every written row is there, every row past an episode's end keeps its fill."""
    from rl2048_amd import _lib as L

    assert rows_of["actions"].shape == (T, len(lengths)) and rows_of["actions"].dtype == torch.uint8
    assert rows_of["rewards"].dtype == torch.float64 and rows_of["flags"].dtype == torch.uint8
    assert rows_of["boards"].shape == ((T, len(lengths)) if W is None else (W, T, len(lengths)))
    for i, n_i in enumerate(lengths):
        t = torch.arange(n_i)
        assert torch.equal(rows_of["actions"][:n_i, i], (t + 1).to(torch.uint8))
        assert torch.equal(rows_of["rewards"][:n_i, i], t.double() + i / 8)
        assert not rows_of["flags"][:n_i, i].any()
        planes = rows_of["boards"][None] if W is None else rows_of["boards"]
        for w in range(planes.shape[0]):
            assert torch.equal(planes[w, :n_i, i], 1000 * i + t + w * 10 ** 6)
        assert not rows_of["actions"][n_i:, i].any() and not rows_of["rewards"][n_i:, i].any()
        assert (rows_of["flags"][n_i:, i] == L.F_INACTIVE).all()


def test_growing_doubles_and_resumes_only_the_suspended():
    lengths = [3, 8, 9, 20, 70]
    run, kernel, rows, outs, queue = _growing(lengths, first_cap=8)
    assert run() == 70
    assert kernel.calls == [(5, 0, 8), (3, 1, 16), (2, 1, 32), (1, 1, 64), (1, 1, 128)]
    assert kernel.orders == [None, [2, 3, 4], [3, 4], [4], [4]]
    assert outs.lengths.tolist() == lengths and int(queue) == 0 and rows.cap == 128
    got = rows.sliced(70)
    assert got["probs"] is None and list(got) == ["boards", "actions", "rewards", "flags", "probs"]
    _check_rows(got, lengths, 70)                # rows written before a growth survive it, the fills too
    _check_rows(rows.sliced(128), lengths, 128)


def test_growing_sized_planes_stop_at_max_steps():
    lengths = [3, 40, 40]
    run, kernel, rows, outs, _ = _growing(lengths, first_cap=8, max_steps=40, W=2, probs=True)
    assert run() == 40
    assert [c[2] for c in kernel.calls] == [8, 16, 32, 40]
    assert kernel.strides == [cap * 3 for cap in (8, 16, 32, 40)]
    assert kernel.orders == [None, [1, 2], [1, 2], [1, 2]]
    got = rows.sliced(40)
    _check_rows(got, lengths, 40, W=2)
    assert got["boards"].stride() == (40 * 3, 3, 1)
    assert got["probs"].shape == (40, 3, 4) and got["probs"].dtype == torch.float32 and not got["probs"].any()
    assert outs.final.shape == (2, 3)


def test_row_limit_refuses_before_it_allocates():
    run, kernel, rows, _, _ = _growing([20], first_cap=8, max_rows=12, free_bytes=lambda: 5 << 30)
    with pytest.raises(RuntimeError, match="still running after 8 steps") as e:
        run()
    assert str(e.value) == ("rollout_batch (max_steps=None): 1 episode(s) still running after 8 steps; growing the "
                            "[T, n] trajectory buffer to 16 rows needs 0.0 GiB (free: 5.0 GiB, row limit 12) -- "
                            "set max_steps")
    assert kernel.calls == [(1, 0, 8)] and rows.cap == 8 and rows.actions.shape[0] == 8
    run, kernel, rows, _, _ = _growing([20], first_cap=8, max_rows=1 << 24)
    assert run() == 20 and [c[2] for c in kernel.calls] == [8, 16, 32]


def test_memory_refusal_at_the_byte():
    """n = 4 bitboard episodes: 8 + 1 + 8 + 1 bytes per row and episode, 16 more with probabilities.  Growing 8 rows
    to 16 needs 16 * 72 = 1152 bytes, of which half the present rows' 576 come back from the copy: 864 must be free."""
    from rl2048_amd import rollouts as R

    assert R.TrajectoryRows(4, CPU).row_bytes == 72
    assert R.TrajectoryRows(4, CPU, probs=True).row_bytes == 136
    assert R.TrajectoryRows(4, CPU, W=2).row_bytes == 4 * (16 + 1 + 8 + 1)
    lengths = [12, 1, 1, 1]
    asked = []
    run, kernel, rows, _, _ = _growing(lengths, first_cap=8, free_bytes=lambda: asked.append(1) or 863,
                                       hint=HINT + " or use_action_mask=True")
    with pytest.raises(RuntimeError, match=r"needs 0\.0 GiB .* -- set max_steps or use_action_mask=True$"):
        run()
    assert rows.cap == 8 and len(asked) == 1
    run, kernel, rows, _, _ = _growing(lengths, first_cap=8, free_bytes=lambda: 864)
    assert run() == 12 and rows.cap == 16


def test_a_family_that_suspends_nothing_is_one_launch():
    run, kernel, rows, outs, queue = _growing([3, 8, 5], first_cap=8, max_steps=8, suspends=False,
                                              free_bytes=lambda: pytest.fail("asked for memory"))
    assert run() == 8
    assert kernel.calls == [(3, 0, 8)] and kernel.orders == [None] and int(queue) == 1    # nothing to reset
    _check_rows(rows.sliced(8), [3, 8, 5], 8)
    run, kernel, _, _, _ = _growing([], first_cap=8, suspends=False)
    assert run() == 0 and kernel.calls == [(0, 0, 8)]


def _budgeted(lengths, budget, most, suspends=True):
    from rl2048_amd import rollouts as R

    n = len(lengths)
    outs = R.EpisodeOutputs(n, CPU)
    sus = R.SuspendState(n, CPU) if suspends else None
    kernel = FakeKernel(lengths, outs)
    queue = torch.ones(1, dtype=torch.int32)
    return (lambda: R.run_budgeted(kernel, sus, queue, n, budget, most, HINT)), kernel, outs, queue


def test_budgeted_relaunches_with_more_steps():
    run, kernel, outs, queue = _budgeted([5, 16, 17, 50], budget=16, most=1 << 20)
    run()
    assert kernel.calls == [(4, 0, 16), (2, 1, 32), (1, 1, 48), (1, 1, 64)]
    assert kernel.orders == [None, [2, 3], [3], [3]]
    assert outs.lengths.tolist() == [5, 16, 17, 50] and int(queue) == 0
    run, kernel, _, _ = _budgeted([5, 3], budget=16, most=1 << 20, suspends=False)
    run()
    assert kernel.calls == [(2, 0, 16)]


def test_budgeted_refuses_past_the_most_steps():
    run, kernel, _, _ = _budgeted([ENDLESS, 2], budget=8, most=6)
    with pytest.raises(RuntimeError, match="eval_max_steps = 6") as e:
        run()
    assert str(e.value) == ("evaluate_batch: 1 episode(s) still running after 6 steps; playing on would pass "
                            "eval_max_steps = 6 -- set max_steps")
    assert kernel.calls == [(2, 0, 6)]
    run, kernel, _, _ = _budgeted([ENDLESS], budget=4, most=8)
    with pytest.raises(RuntimeError, match="still running after 8 steps; playing on would pass eval_max_steps = 8"):
        run()
    assert kernel.calls == [(1, 0, 4), (1, 1, 8)]


def test_episode_outputs_and_their_structs():
    from rl2048_amd import _lib as L
    from rl2048_amd import rollouts as R

    outs = R.EpisodeOutputs(3, CPU)
    assert (outs.lengths.dtype, outs.totals.dtype, outs.max_e.dtype, outs.final.dtype) == \
        (torch.int32, torch.float64, torch.uint8, torch.int64)
    outs.max_e.copy_(torch.tensor([1, 11, 15], dtype=torch.uint8))
    assert outs.max_tile.dtype == torch.int64 and outs.max_tile.tolist() == [2, 2048, 32768]
    ev = outs.eval_out()
    assert [getattr(ev, f) for f, _ in L.EvalOut._fields_] == \
        [t.data_ptr() for t in (outs.lengths, outs.totals, outs.max_e, outs.final)]
    rows = R.TrajectoryRows(3, CPU, probs=True)
    rows.grow(4)
    tr = rows.traj(outs)
    assert [getattr(tr, f) for f, _ in L.Traj._fields_] == \
        [t.data_ptr() for t in (rows.boards, rows.actions, rows.rewards, rows.flags, rows.probs, outs.lengths,
                                outs.totals, outs.max_e, outs.final)]
    rows = R.TrajectoryRows(3, CPU)
    rows.grow(1)
    assert rows.pointers()[4] is None and rows.probs is None
    assert R.EpisodeOutputs(0, CPU).longest() == 0 and R.EpisodeOutputs(3, CPU, W=4).final.shape == (4, 3)
    sus = R.SuspendState(3, CPU, W=2)
    assert sus.board.shape == (2, 3) and sus.meta.shape == (9,) and sus.meta.dtype == torch.int32
    assert sus.list.shape == (3,) and sus.list.dtype == torch.int32 and R.SuspendState(0, CPU).list.shape == (1,)
    first = sus.list
    assert sus.flip() is first and sus.list is not first and sus.flip() is not first and sus.list is first
