"""CPU reference of the global state (docs/SPEC.md S20): the five whole-map planes of one env, and of a batch, in numpy,
written as the definition reads -- a loop over the agents, highest index first, so that the lowest index is written last
and wins a shared cell."""
import numpy as np

CHANNELS = ("obstacles", "agents", "targets", "agent_ids", "target_ids")
ACTIVE, GHOST = 1, 2                         # the bits of the engine's per-agent `active` byte


def global_state_env(obstacles, agents_xy, targets_xy, active_byte):
    """obstacles [H, W] of 0 / 1, agents_xy / targets_xy [A, 2] unpadded (row, column), active_byte [A]: 0 = finished and
    hidden, 1 = active, 3 = active but missing from the occupancy array (a `soft` ghost).  Returns int32 [5, H, W], plane
    k the channel CHANNELS[k]."""
    obstacles = np.asarray(obstacles)
    H, W = obstacles.shape
    out = np.zeros((5, H, W), dtype=np.int32)
    out[0] = obstacles
    agents_xy, targets_xy = np.asarray(agents_xy).reshape(-1, 2), np.asarray(targets_xy).reshape(-1, 2)
    active_byte = np.asarray(active_byte).reshape(-1)
    for i in range(len(active_byte) - 1, -1, -1):
        a = int(active_byte[i])
        if a == ACTIVE:                      # stands there and is in the occupancy array
            x, y = (int(v) for v in agents_xy[i])
            out[1, x, y] = 1
            out[3, x, y] = i + 1
        if a & ACTIVE:                       # a ghost is still on its way to its target
            x, y = (int(v) for v in targets_xy[i])
            out[2, x, y] = 1
            out[4, x, y] = i + 1
    return out


def global_state_reference(obstacles, agents_xy, targets_xy, active_byte):
    """The batched form: obstacles [B, H, W], agents_xy / targets_xy [B, A, 2], active_byte [B, A] -> int32 [B, 5, H, W]."""
    return np.stack([global_state_env(o, a, t, b) for o, a, t, b in zip(obstacles, agents_xy, targets_xy, active_byte)])
