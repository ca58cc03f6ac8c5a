"""The step kernel's chunk tickets (csrc/g2048.hip, the three-cell path: LDS && RK == 1) against the batched CPU
oracle, every lane and every output by equality after every step (test_gpu_step_matrix.Case).

From its third sweep on a wave claims its chunks from a counter in the workgroup's LDS, so which wave steps which
chunk, and how many a wave steps, varies from launch to launch; a lane's pending auto-reset sits in one slot per lane
and moves to the workgroup's list when the lane flags a second one.  In all three tests the state word's step count
equals the oracle's in every lane after every step (Case.check_state), so each lane was stepped exactly once per
launch.  `cus` is the device's CU count; the grid is one workgroup per CU.

* test_ragged_third_round: n = 2 * 1024 * cus + 5 * 64 + 37.  Only workgroup 0 has a third round, of five full chunks
  and one ragged one; every other workgroup's first ticket is void.  Every lane resets exactly once, in step 2.
* test_sparse_resets: n = 3 * 1024 * cus + 37, the smallest batch in which every wave draws a ticket; mixed start
  boards, so terminations, truncations and invalid moves fall in different sweeps of a lane.
* test_reset_slot_collision: n = 7 * 1024 * cus + 3 * 1024 + 37, more than two trips round the three register buffers
  on claimed chunks.  max_steps = 1 resets every lane in every sweep, so the slot collides in each sweep after a
  wave's first, and every workgroup's list (4,096 entries for >= 7,168 resets) overflows into the per-lane fallback.
"""
import pytest
import torch

from oracle import oracle as O
from test_gpu_step_matrix import K_BLOCK, Case

pytestmark = pytest.mark.gpu

K_RESET3_CAP = 4 * K_BLOCK     # csrc/g2048.hip kReset3Cap


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("obs,rng", [("log2", "pcg64"), ("onehot", "philox")])
def test_ragged_third_round(obs, rng):
    cus = _cus()
    n = 2 * K_BLOCK * cus + 5 * 64 + 37
    c = Case(n, obs, rng, "xo3_rk1", case=3, max_steps=2, boards="reset")
    fl = [c.step() for _ in range(3)]
    both = O.B_RESET | O.B_TRUNCATED
    assert bool(((fl[0] & O.B_RESET) == 0).all()) and bool(((fl[1] & both) == both).all())
    assert bool(((fl[2] & O.B_RESET) == 0).all()) and int(c.resets.min()) == 1 == int(c.resets.max())


@pytest.mark.parametrize("rng", ["pcg64", "philox"])
def test_sparse_resets(rng):
    cus = _cus()
    n = 3 * K_BLOCK * cus + 37
    c = Case(n, "log2", rng, "xo3_rk1", case=6, max_steps=4, boards="mixed")
    for _ in range(6):
        c.step()
    k = c.count
    assert k["term"] > 0 and k["trunc"] > 0 and k["invalid"] > 0, k
    assert int(c.resets.sum()) > 0, "resets occurred"
    assert k["skipped"] == 0, k


def test_reset_slot_collision():
    cus = _cus()
    n = 7 * K_BLOCK * cus + 3 * K_BLOCK + 37
    assert 7 * K_BLOCK > K_RESET3_CAP, "every workgroup's list overflows"
    c = Case(n, "log2", "pcg64", "xo3_rk1", case=9, max_steps=1, boards="reset")
    fl = [c.step() for _ in range(2)]
    for f in fl:   # a fresh game cannot end in one move: every step truncates and resets every lane
        assert bool(((f & (O.B_RESET | O.B_TRUNCATED)) == (O.B_RESET | O.B_TRUNCATED)).all())
    assert int(c.resets.min()) == 2 == int(c.resets.max())
