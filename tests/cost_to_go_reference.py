"""CPU reference of the cost-to-go windows (docs/SPEC.md S11), on the state `VecPogema.get_state()` and the installed
maps describe.  `cost_to_go_env` runs tests/expert_reference.py's queue BFS once per distinct target; `fields_packed` is a
vectorised variant for many searches on maps at most 64 wide (bit-parallel rows, the distance counted in bit planes).
Test infrastructure only; the package never imports it."""
from __future__ import annotations

import numpy as np

from expert_reference import bfs_from


def window(field, x, y, r):
    """The (2r+1, 2r+1) window of `field` (-1: unreachable) around unpadded cell (x, y); -1 outside the map."""
    H, W = field.shape
    w = 2 * r + 1
    out = np.full((w, w), -1, dtype=np.int32)
    x0, y0 = x - r, y - r
    xa, xb = max(x0, 0), min(x0 + w, H)
    ya, yb = max(y0, 0), min(y0 + w, W)
    if xa < xb and ya < yb:
        out[xa - x0:xb - x0, ya - y0:yb - y0] = field[xa:xb, ya:yb]
    return out


def fields_packed(obstacles, targets):
    """Distance fields for many searches at once: obstacles [N, H, W] (W <= 64), targets [N, 2] -> int32 [N, H, W],
    -1 where unreachable (everywhere when the target is an obstacle).  Level-synchronous BFS on uint64 row masks."""
    obstacles = np.asarray(obstacles) != 0
    N, H, W = obstacles.shape
    assert W <= 64
    weights = np.left_shift(np.uint64(1), np.arange(W, dtype=np.uint64))
    free = (np.where(~obstacles, weights, np.uint64(0))).sum(axis=2, dtype=np.uint64)     # [N, H]
    t = np.asarray(targets, dtype=np.int64)
    v = np.zeros((N, H), dtype=np.uint64)
    v[np.arange(N), t[:, 0]] = np.left_shift(np.uint64(1), t[:, 1].astype(np.uint64))
    v &= free
    one = np.uint64(1)
    planes = []                                   # dist = number of levels a cell was still unvisited, in bit planes
    while True:
        nv = v | (v << one) | (v >> one)
        nv[:, 1:] |= v[:, :-1]
        nv[:, :-1] |= v[:, 1:]
        nv &= free
        if np.array_equal(nv, v):
            break
        carry = ~v & free
        for p in planes:
            p ^= carry
            carry &= ~p
            if not carry.any():
                break
        if carry.any():
            planes.append(carry.copy())
        v = nv
    dist = np.zeros((N, H, W), dtype=np.int64)
    bits = np.arange(W, dtype=np.uint64)
    for k, p in enumerate(planes):
        dist += ((p[:, :, None] >> bits) & one).astype(np.int64) << k
    visited = ((v[:, :, None] >> bits) & one).astype(bool)
    return np.where(visited, dist, -1).astype(np.int32)


def cost_to_go_env(obstacles, agents_xy, targets_xy, is_active, r, packed=False):
    """One environment: obstacles [H, W], agents_xy / targets_xy [A, 2], is_active [A] -> int32 [A, 2r+1, 2r+1]."""
    obstacles = np.asarray(obstacles) != 0
    agents_xy, targets_xy = np.asarray(agents_xy), np.asarray(targets_xy)
    is_active = np.asarray(is_active).astype(bool)
    A = agents_xy.shape[0]
    w = 2 * r + 1
    out = np.full((A, w, w), -1, dtype=np.int32)
    want = sorted({(int(targets_xy[i][0]), int(targets_xy[i][1])) for i in range(A) if is_active[i]})
    if packed and want:
        f = fields_packed(np.broadcast_to(obstacles, (len(want),) + obstacles.shape), want)
        fields = {t: f[k] for k, t in enumerate(want)}
    else:
        fields = {t: bfs_from(obstacles, *t) for t in want}
    for i in range(A):
        if is_active[i]:
            t = (int(targets_xy[i][0]), int(targets_xy[i][1]))
            out[i] = window(fields[t], int(agents_xy[i][0]), int(agents_xy[i][1]), r)
    return out


def cost_to_go_reference(obstacles, agents_xy, targets_xy, is_active, r, envs=None):
    """Batched: obstacles [B, H, W], agents_xy / targets_xy [B, A, 2], is_active [B, A] -> int32 [B, A, 2r+1, 2r+1].
    `envs`: only these environments (the other rows stay -1).  Maps at most 64 wide take the vectorised search, all
    environments' distinct targets together."""
    obstacles, agents_xy, targets_xy, is_active = (np.asarray(v) for v in (obstacles, agents_xy, targets_xy, is_active))
    B, A = agents_xy.shape[:2]
    w = 2 * r + 1
    out = np.full((B, A, w, w), -1, dtype=np.int32)
    envs = list(range(B) if envs is None else envs)
    if obstacles.shape[2] > 64:
        for b in envs:
            out[b] = cost_to_go_env(obstacles[b], agents_xy[b], targets_xy[b], is_active[b], r)
        return out
    keys = sorted({(b, int(targets_xy[b, i, 0]), int(targets_xy[b, i, 1])) for b in envs for i in range(A)
                   if is_active[b, i]})
    fields = {}
    for c in range(0, len(keys), 4096):
        chunk = np.array(keys[c:c + 4096], dtype=np.int64)
        f = fields_packed(obstacles[chunk[:, 0]], chunk[:, 1:])
        fields.update({tuple(int(x) for x in k): f[j] for j, k in enumerate(chunk)})
    for b in envs:
        for i in range(A):
            if is_active[b, i]:
                field = fields[(b, int(targets_xy[b, i, 0]), int(targets_xy[b, i, 1]))]
                out[b, i] = window(field, int(agents_xy[b, i, 0]), int(agents_xy[b, i, 1]), r)
    return out
