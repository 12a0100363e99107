"""Inputs the collision-shielding tests share: tests/test_shield.py proves on the CPU reference alone that they exercise
what they are meant to (failed PIBT calls, overridden and kept choices), tests/test_shield_gpu.py runs them on the device."""
from __future__ import annotations

import numpy as np

CROWD_SCORES = (0.0, 1.0, 0.5, 3.0, 2.0)    # everyone wants left, then right, up, down; staying is the last resort


def crowd_state():
    """30 agents side by side in the far corner of a 200 x 200 map (the cells of test_pibt_gpu's crowded corner, in
    index order and reversed).  Walls on the left and above close the 5 x 6 block into a room with no free cell but a
    two-cell pocket above it: with CROWD_SCORES everyone pushes left, into each other and the wall; agents rotate
    through the pocket and PIBT calls fail in both envs at every step.  Few distinct targets (the CPU reference runs one BFS over the
    map per target); those of env 1 lie outside the room, out of reach.
    -> (obstacles [2, 200, 200], agents_xy [2, 30, 2], targets_xy [2, 30, 2])."""
    obst = np.zeros((2, 200, 200), dtype=np.uint8)
    obst[:, 192:200, 193] = 1
    obst[:, 194, 193:200] = 1
    obst[:, 192, 193:200] = 1
    obst[:, 193, 193:196] = 1
    obst[:, 193, 198:200] = 1
    obst[:, 194, 196] = 0                   # the door to the pocket (193, 196), (193, 197)
    cells = np.array([(199 - i // 6, 199 - i % 6) for i in range(30)], dtype=np.int32)
    agents = np.stack([cells, cells[::-1]])
    targets = np.stack([cells[np.arange(30) % 3 * 7], np.array([(i % 2, 0) for i in range(30)], dtype=np.int32)])
    return obst, agents, targets


def crowd_scores(batch=2, agents=30):
    return np.broadcast_to(np.array(CROWD_SCORES, dtype=np.float32), (batch, agents, 5)).copy()


def random_scores(rng, batch, agents):
    """float32 [batch, agents, 5], standard normal: no ties, every order of the five actions about equally often."""
    return rng.standard_normal((batch, agents, 5)).astype(np.float32)


def special_scores(rng, batch, agents):
    """Random scores drawn from a few values only, NaN, +-inf and +-0.0 among them: many ties and every special value
    in every position."""
    values = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0, 1e-40, -1e-40, 3.5], dtype=np.float32)
    return values[rng.integers(0, len(values), size=(batch, agents, 5))]
