"""CPU reference of the agent forecasts (docs/SPEC.md S24), a literal statement of the section on tests/
cost_to_go_reference.py's fields: every active agent descends its own distance field for K steps by the lowest move that
leads to a defined, strictly smaller distance inside the map and waits where there is none; an active observer's plane
s - 1 holds the step-s cell of every other active agent it sees now.  Test infrastructure only; the package never imports
it."""
from __future__ import annotations

import numpy as np

from cost_to_go_reference import fields_packed
from expert_reference import MOVES, bfs_from


def forecast(field, x, y, K):
    """field int [H, W] (-1: no distance), the agent's cell -> [(x, y)] * K: q(1) .. q(K)."""
    H, W = field.shape
    out = []
    for _ in range(K):
        if field[x, y] >= 0:
            for dx, dy in MOVES[1:]:
                nx, ny = x + dx, y + dy
                if 0 <= nx < H and 0 <= ny < W and 0 <= field[nx, ny] < field[x, y]:
                    x, y = nx, ny
                    break
        out.append((x, y))
    return out


def _fields(obstacles, targets_xy, is_active, envs):
    """(b, i) -> the distance field of active agent i of env b, one search per distinct (env, target)."""
    B, A = targets_xy.shape[:2]
    keys = sorted({(b, int(targets_xy[b, i, 0]), int(targets_xy[b, i, 1])) for b in envs for i in range(A) if is_active[b, i]})
    by_key = {}
    if obstacles.shape[2] <= 64:
        for c in range(0, len(keys), 4096):
            chunk = np.array(keys[c:c + 4096], dtype=np.int64)
            f = fields_packed(obstacles[chunk[:, 0]], chunk[:, 1:])
            by_key.update({tuple(int(v) for v in k): f[n] for n, k in enumerate(chunk)})
    else:
        for b, tx, ty in keys:
            by_key[(b, tx, ty)] = bfs_from(obstacles[b] != 0, tx, ty)
    return {(b, i): by_key[(b, int(targets_xy[b, i, 0]), int(targets_xy[b, i, 1]))]
            for b in envs for i in range(A) if is_active[b, i]}


def agent_forecasts_reference(obstacles, agents_xy, targets_xy, is_active, r, K, envs=None):
    """Batched: obstacles [B, H, W], agents_xy / targets_xy [B, A, 2], is_active [B, A] ->
    (planes uint8 [B, A, K, 2r+1, 2r+1], cells int16 [B, A, K, 2]).  `envs`: only these environments (the other rows
    stay 0)."""
    obstacles, agents_xy, targets_xy = (np.asarray(v) for v in (obstacles, agents_xy, targets_xy))
    is_active = np.asarray(is_active).astype(bool)
    B, A = agents_xy.shape[:2]
    w = 2 * r + 1
    envs = list(range(B) if envs is None else envs)
    fields = _fields(obstacles, targets_xy, is_active, envs)
    planes = np.zeros((B, A, K, w, w), dtype=np.uint8)
    cells = np.zeros((B, A, K, 2), dtype=np.int16)
    for b in envs:
        for j in range(A):
            if is_active[b, j]:
                cells[b, j] = forecast(fields[(b, j)], int(agents_xy[b, j, 0]), int(agents_xy[b, j, 1]), K)
            else:
                cells[b, j] = -1
        for i in np.nonzero(is_active[b])[0]:
            off = agents_xy[b] - agents_xy[b, i]
            seen = is_active[b] & (np.abs(off) <= r).all(-1)
            seen[i] = False
            uv = cells[b, seen].astype(np.int64) - agents_xy[b, i] + r          # [seen, K, 2]: q_j(s) as a window cell
            inside = ((uv >= 0) & (uv < w)).all(-1)                              # no clamp: a cell outside is not drawn
            _, s = np.nonzero(inside)
            planes[b, i, s, uv[inside][:, 0], uv[inside][:, 1]] = 1
    return planes, cells


def rows(planes):
    """uint8 [..., w, w] planes -> int32 [..., w] row masks, bit v of word u = cell (u, v)."""
    planes = np.asarray(planes)
    return (planes.astype(np.int64) << np.arange(planes.shape[-1])).sum(-1).astype(np.int32)
