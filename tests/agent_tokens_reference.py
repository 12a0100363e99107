"""Plain numpy statement of docs/SPEC.md S21 (agent tokens), the reference of tests/test_agent_tokens*.py, on the state
`VecPogema.get_state()` and the installed maps describe.  The row of an agent is put together from the references of the
queries S21 names -- cost_to_go_reference, visible_agents_reference, goal_directions_reference -- and restates none of
them; the vocabulary is written out here as numbers, so that a constant that moves in the engine fails the tests.  Test
infrastructure only; the package never imports it."""
from __future__ import annotations

import numpy as np

from cost_to_go_reference import cost_to_go_reference
from goal_directions_reference import goal_directions_reference
from visible_agents_reference import visible_agents_reference

CLIP = 20
BLOCKED = 41
ACTION_NONE = 42
ACTION0 = 43
GREEDY0 = 48
PAD = 64
NUM_TOKENS = 65
HISTORY = 5
SLOT_LEN = 10


def token_length(r, slots):
    return (2 * r + 1) ** 2 + SLOT_LEN * slots


def _clip(v):
    return np.clip(np.asarray(v, dtype=np.int64), -CLIP, CLIP) + CLIP


def tokens_from_queries(ctg, index, offset, mask, agents_xy, targets_xy, is_active, slots, history=None, length=None):
    """The rows from the results of the queries: ctg int [B, A, W, W]; index [B, A, slots - 1] and offset
    [B, A, slots - 1, 2] (None with slots = 1); mask uint8 [B, A] (the bits at the window centres); the state arrays;
    history int [B, A, 5] or None -> uint8 [B, A, length]."""
    ctg = np.asarray(ctg).astype(np.int64)
    agents_xy, targets_xy = np.asarray(agents_xy).astype(np.int64), np.asarray(targets_xy).astype(np.int64)
    is_active = np.asarray(is_active).astype(bool)
    B, A, W, _ = ctg.shape
    r = (W - 1) // 2
    l0 = token_length(r, slots)
    length = l0 if length is None else length
    assert l0 <= length
    hist = np.full((B, A, HISTORY), ACTION_NONE, dtype=np.int64)
    if history is not None:
        h = np.asarray(history).astype(np.int64)
        hist = np.where((h >= 0) & (h <= 4), ACTION0 + h, ACTION_NONE)
    out = np.full((B, A, length), PAD, dtype=np.uint8)
    for b in range(B):
        for i in range(A):
            if not is_active[b, i]:
                continue
            own = ctg[b, i, r, r]
            win = ctg[b, i].reshape(-1)
            out[b, i, :W * W] = np.where((win == -1) | (own == -1), BLOCKED, _clip(win - own))
            for s in range(slots):
                if s == 0:
                    j, dx, dy = i, 0, 0
                else:
                    j = int(index[b, i, s - 1])
                    dx, dy = (int(v) for v in offset[b, i, s - 1])
                if j == -1:
                    continue
                at = W * W + SLOT_LEN * s
                out[b, i, at:at + 2] = (dx + CLIP, dy + CLIP)
                out[b, i, at + 2:at + 4] = _clip(targets_xy[b, j] - agents_xy[b, i])
                out[b, i, at + 4:at + 4 + HISTORY] = hist[b, j]
                out[b, i, at + 9] = GREEDY0 + int(mask[b, j])
    return out


def agent_tokens_reference(obstacles, agents_xy, targets_xy, is_active, r, slots=13, history=None, length=None):
    """Batched: obstacles [B, H, W], agents_xy / targets_xy [B, A, 2], is_active [B, A] -> uint8 [B, A, length]."""
    ctg = cost_to_go_reference(obstacles, agents_xy, targets_xy, is_active, r)
    index = offset = None
    if slots > 1:
        index, offset, _ = visible_agents_reference(np.asarray(agents_xy), np.asarray(is_active), r, slots - 1)
    mask = goal_directions_reference(obstacles, agents_xy, targets_xy, is_active, r)[:, :, r, r]
    return tokens_from_queries(ctg, index, offset, mask, agents_xy, targets_xy, is_active, slots, history, length)
