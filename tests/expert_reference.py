"""CPU reference of the shortest-path expert (docs/SPEC.md "Shortest-path expert"): a plain queue BFS per agent from
its target, on the state `VecPogema.get_state()` and the installed maps describe.  Test infrastructure only; the
package never imports it."""
from __future__ import annotations

from collections import deque

import numpy as np

# upstream's MOVES: noop, up, down, left, right
MOVES = ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1))


def bfs_from(blocked, tx, ty):
    """Distance of every cell to (tx, ty) over the unblocked cells (-1: unreachable); all -1 if the target is blocked."""
    H, W = blocked.shape
    dist = np.full((H, W), -1, dtype=np.int64)
    if blocked[tx, ty]:
        return dist
    dist[tx, ty] = 0
    q = deque([(tx, ty)])
    while q:
        x, y = q.popleft()
        d = dist[x, y] + 1
        for dx, dy in MOVES[1:]:
            nx, ny = x + dx, y + dy
            if 0 <= nx < H and 0 <= ny < W and not blocked[nx, ny] and dist[nx, ny] < 0:
                dist[nx, ny] = d
                q.append((nx, ny))
    return dist


def expert_env(obstacles, agents_xy, targets_xy, is_active, agents_as_obstacles=False):
    """One environment: obstacles [H, W], agents_xy / targets_xy [A, 2], is_active [A] -> (actions [A], distance [A])."""
    obstacles = np.asarray(obstacles) != 0
    agents_xy, targets_xy = np.asarray(agents_xy), np.asarray(targets_xy)
    is_active = np.asarray(is_active).astype(bool)
    H, W = obstacles.shape
    A = agents_xy.shape[0]
    actions = np.zeros(A, dtype=np.int64)
    distance = np.full(A, -1, dtype=np.int32)
    cache = {}
    for i in range(A):
        if not is_active[i]:
            continue
        ax, ay = (int(v) for v in agents_xy[i])
        tx, ty = (int(v) for v in targets_xy[i])
        if (ax, ay) == (tx, ty):
            distance[i] = 0
            continue
        blocked = obstacles.copy()
        if agents_as_obstacles:
            for j in range(A):
                if j != i and is_active[j]:
                    blocked[agents_xy[j][0], agents_xy[j][1]] = True
            # the agent's own cell and its own target are never blocked by agents (obstacles still count)
            blocked[ax, ay] = obstacles[ax, ay]
            blocked[tx, ty] = obstacles[tx, ty]
            field = bfs_from(blocked, tx, ty)
        else:
            if (tx, ty) not in cache:
                cache[(tx, ty)] = bfs_from(blocked, tx, ty)
            field = cache[(tx, ty)]
        d = int(field[ax, ay])
        distance[i] = d
        if d > 0:
            for a, (dx, dy) in enumerate(MOVES[1:], start=1):
                nx, ny = ax + dx, ay + dy
                if 0 <= nx < H and 0 <= ny < W and field[nx, ny] == d - 1:
                    actions[i] = a
                    break
    return actions, distance


def expert_reference(obstacles, agents_xy, targets_xy, is_active, agents_as_obstacles=False, envs=None):
    """Batched: obstacles [B, H, W], agents_xy / targets_xy [B, A, 2], is_active [B, A] -> (actions int64 [B, A],
    distance int32 [B, A]).  `envs`: only these environments (the other rows stay 0 / -1)."""
    obstacles, agents_xy, targets_xy, is_active = (np.asarray(v) for v in (obstacles, agents_xy, targets_xy, is_active))
    B, A = agents_xy.shape[:2]
    actions = np.zeros((B, A), dtype=np.int64)
    distance = np.full((B, A), -1, dtype=np.int32)
    for b in (range(B) if envs is None else envs):
        actions[b], distance[b] = expert_env(obstacles[b], agents_xy[b], targets_xy[b], is_active[b], agents_as_obstacles)
    return actions, distance
