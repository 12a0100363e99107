"""CPU reference of the path-to-goal planes and sub-goals (docs/SPEC.md S22): the walk over tests/
goal_directions_reference.py's masks.  At every cell the lowest bit of the mask is the move; the walk ends where the mask
is empty (the target, or nothing to descend), where the move leaves the window, or at the cap.  The masks of the window's
edge cells see the field beyond the window, so the edge is exact.  Test infrastructure only; the package never imports
it."""
from __future__ import annotations

import numpy as np

from expert_reference import MOVES
from goal_directions_reference import goal_directions_reference


def walk(bits, steps=None):
    """bits uint8 [w, w]: one agent's direction masks -> (plane uint8 [w, w], (dx, dy), length)."""
    w = bits.shape[0]
    r = w // 2
    cap = w * w - 1 if steps is None else min(int(steps), w * w - 1)
    plane = np.zeros((w, w), dtype=np.uint8)
    u = v = r
    n = 0
    while n < cap and bits[u, v]:
        m = int(bits[u, v])
        dx, dy = MOVES[(m & -m).bit_length()]
        if not (0 <= u + dx < w and 0 <= v + dy < w):
            break
        u, v, n = u + dx, v + dy, n + 1
        plane[u, v] = 1
    return plane, (u - r, v - r), n


def goal_paths_reference(obstacles, agents_xy, targets_xy, is_active, r, steps=None, envs=None):
    """Batched: obstacles [B, H, W], agents_xy / targets_xy [B, A, 2], is_active [B, A] ->
    (planes uint8 [B, A, 2r+1, 2r+1], subgoal int8 [B, A, 2], length int32 [B, A]).  `envs`: only these environments
    (the other rows stay 0)."""
    bits = goal_directions_reference(obstacles, agents_xy, targets_xy, is_active, r, envs=envs)
    B, A = bits.shape[:2]
    planes = np.zeros(bits.shape, dtype=np.uint8)
    subgoal = np.zeros((B, A, 2), dtype=np.int8)
    length = np.zeros((B, A), dtype=np.int32)
    for b, i in zip(*np.nonzero(bits[:, :, r, r])):
        planes[b, i], subgoal[b, i], length[b, i] = walk(bits[b, i], steps)
    return planes, subgoal, length


def rows(planes):
    """uint8 [..., w, w] planes -> int32 [..., w] row masks, bit v of word u = cell (u, v)."""
    planes = np.asarray(planes)
    return (planes.astype(np.int64) << np.arange(planes.shape[-1])).sum(-1).astype(np.int32)
