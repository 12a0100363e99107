"""CPU reference of the one plane of the policy input that nothing else in the engine writes (docs/SPEC.md S18;
VecPogema.policy_input / pgx_policy_input): `other_goals`, the targets of the agents an observer sees, from the arrays of
get_state().  Written as the definition reads: a double loop over observers and agents, with the clamp.  The other seven
planes are observe()'s and goal_directions()', which have references of their own."""
import numpy as np

CHANNELS = ("obstacles", "agents", "target", "other_goals", "up", "down", "left", "right")  # index = PGX_CHANNEL_* code


def clamp(v, r):
    return max(-r, min(r, v))


def other_goals_env(agents_xy, targets_xy, is_active, r):
    """One env: agents_xy, targets_xy [A][2] unpadded (row, col), is_active [A] -> uint8 [A, W, W], W = 2r + 1."""
    A, W = len(agents_xy), 2 * r + 1
    out = np.zeros((A, W, W), dtype=np.uint8)
    for i in range(A):
        if not is_active[i]:
            continue                          # an inactive observer sees nobody
        xi, yi = int(agents_xy[i][0]), int(agents_xy[i][1])
        for j in range(A):
            if j == i or not is_active[j]:
                continue
            xj, yj = int(agents_xy[j][0]), int(agents_xy[j][1])
            if abs(xj - xi) > r or abs(yj - yi) > r:
                continue                      # j is not visible to i (S12)
            fx, fy = int(targets_xy[j][0]), int(targets_xy[j][1])
            out[i, r + clamp(fx - xi, r), r + clamp(fy - yi, r)] = 1
    return out


def other_goals_reference(agents_xy, targets_xy, is_active, r):
    """agents_xy, targets_xy [B, A, 2], is_active [B, A] -> uint8 [B, A, W, W]."""
    return np.stack([other_goals_env(agents_xy[b], targets_xy[b], is_active[b], r) for b in range(len(agents_xy))])
