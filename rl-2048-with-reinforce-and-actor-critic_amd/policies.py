"""Scripted players for ReinforceAgent.rollout_batch / evaluate_batch / run_episode (their ``action_gen`` argument): the
reference's baseline generators (tools/simple_action_gen.py) as objects the device kernels of
include/g2048_scripted.h can play whole episodes for.  No device work happens here."""
from __future__ import annotations

import ctypes
import operator

from . import _lib as L


class PriorityPolicy:
    """The first action of ``order`` (a permutation of (0, 1, 2, 3): 0 up, 1 right, 2 down, 3 left) that the board's
    action mask allows.  PriorityPolicy(PriorityPolicy.URDL) is the reference's action_gen_1 and
    PriorityPolicy(PriorityPolicy.URLD) its action_gen_2.  select_action takes a valid candidate as it is
    (src/reinforce_agent.py:153-176): the policy stream is never drawn from and the net does not influence the episode.

    Callable with the reference's signature ``(state, action_mask) -> int``, so an instance also serves as the
    ``action_gen`` of the host path and of the reference itself."""

    URDL = (0, 1, 2, 3)
    URLD = (0, 1, 3, 2)

    def __init__(self, order):
        try:
            entries = tuple(operator.index(a) for a in order)   # integers only: 1.0 or "1" is no action
        except TypeError:
            raise ValueError(f"order must be a permutation of (0, 1, 2, 3), got {order!r}") from None
        if sorted(entries) != [0, 1, 2, 3]:
            raise ValueError(f"order must be a permutation of (0, 1, 2, 3), got {order!r}")
        self.order = entries

    def __call__(self, state, action_mask) -> int:
        for a in self.order:
            if action_mask[a]:
                return a
        return self.order[0]

    def __repr__(self) -> str:
        return f"PriorityPolicy({self.order!r})"

    def _script(self) -> L.Script:
        return L.Script(L.SCRIPT_PRIORITY, (ctypes.c_uint8 * 4)(*self.order))


class UniformPolicy:
    """The random-valid baseline on the episode's policy stream: select_action for a net whose logits are all equal.
    p[a] = fp32(1) / fp32(k) on the k actions the mask allows (all four when the env has no action mask), 0 elsewhere;
    one Generator.random() draw per step, also when k = 1; the action is Generator.choice(4, p=p).  Not a callable: it
    needs the policy stream, which the reference's action_gen signature does not carry."""

    def __repr__(self) -> str:
        return "UniformPolicy()"

    def _script(self) -> L.Script:
        return L.Script(L.SCRIPT_UNIFORM, (ctypes.c_uint8 * 4)(0, 1, 2, 3))
