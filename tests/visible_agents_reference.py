"""Plain numpy / Python statement of docs/SPEC.md S12 (neighbour lists), the reference of tests/test_visible_agents*.py.

Agent j is visible to agent i iff j != i, j is active and |dx| <= r and |dy| <= r for (dx, dy) = xy_j - xy_i; an
inactive agent sees nobody.  The visible agents are sorted as Python tuples (dx*dx + dy*dy, dx + r, dy + r, j); nothing
is packed and no code is shared with the engine."""
import numpy as np


def visible_agents_env(agents_xy, active, r, k):
    """One env: agents_xy [A, 2], active [A] -> (index int32 [A, k], offset int8 [A, k, 2], count int32 [A])."""
    xy = np.asarray(agents_xy, dtype=np.int64).reshape(-1, 2)
    act = np.asarray(active).astype(bool).reshape(-1)
    n = len(xy)
    index = np.full((n, k), -1, dtype=np.int32)
    offset = np.zeros((n, k, 2), dtype=np.int8)
    count = np.zeros((n,), dtype=np.int32)
    for i in range(n):
        if not act[i]:
            continue
        d = xy - xy[i]
        inside = act & (np.abs(d[:, 0]) <= r) & (np.abs(d[:, 1]) <= r)
        inside[i] = False
        seen = []
        for j in np.nonzero(inside)[0]:
            dx, dy = int(d[j, 0]), int(d[j, 1])
            seen.append((dx * dx + dy * dy, dx + r, dy + r, int(j)))
        seen.sort()
        count[i] = len(seen)
        for slot, (_, u, v, j) in enumerate(seen[:k]):
            index[i, slot] = j
            offset[i, slot] = (u - r, v - r)
    return index, offset, count


def visible_agents_reference(agents_xy, active, r, k):
    """Batch: agents_xy [B, A, 2], active [B, A] -> (index [B, A, k], offset [B, A, k, 2], count [B, A])."""
    per_env = [visible_agents_env(agents_xy[b], active[b], r, k) for b in range(len(agents_xy))]
    return tuple(np.stack([e[i] for e in per_env]) for i in range(3))
