"""CPU reference of the direction-to-goal planes (docs/SPEC.md S14), on the state `VecPogema.get_state()` and the installed
maps describe.  A plane bit compares a cell's distance with its neighbour's in the agent's WHOLE field (tests/
expert_reference.py's queue BFS from the target), so the cells on the window's edge see the field beyond the window.
The batched variant takes tests/cost_to_go_reference.py's vectorised search on maps at most 64 wide.  The result is the
"bits" format, uint8 with bit a-1 = plane a-1; `planes` expands it.  Test infrastructure only; the package never imports
it."""
from __future__ import annotations

import numpy as np

from cost_to_go_reference import fields_packed
from expert_reference import MOVES, bfs_from


def bits_from_tiles(tiles):
    """tiles int [N, w+2, w+2]: the window and one cell around it, -1 where the distance is undefined -> uint8 [N, w, w]."""
    tiles = np.asarray(tiles)
    hs = tiles.shape[-1]
    c = tiles[:, 1:-1, 1:-1]
    bits = np.zeros(c.shape, dtype=np.uint8)
    for a, (dx, dy) in enumerate(MOVES[1:]):
        n = tiles[:, 1 + dx:hs - 1 + dx, 1 + dy:hs - 1 + dy]
        bits |= ((c >= 0) & (n >= 0) & (n < c)).astype(np.uint8) << a
    return bits


def halo_tile(field, x, y, r):
    """The (2r+3, 2r+3) tile of `field` (-1: undefined) around unpadded cell (x, y); -1 outside the map."""
    pad = r + 1
    return np.pad(np.asarray(field), pad, constant_values=-1)[x:x + 2 * pad + 1, y:y + 2 * pad + 1]


def directions_window(field, x, y, r):
    """uint8 [2r+1, 2r+1] masks of the window around (x, y) from a whole-map distance field (-1: undefined)."""
    return bits_from_tiles(halo_tile(field, x, y, r)[None])[0]


def planes(bits):
    """uint8 [..., w, w] masks -> uint8 [..., 4, w, w] planes of 0 / 1."""
    bits = np.asarray(bits)
    return np.stack([(bits >> a) & 1 for a in range(4)], axis=-3).astype(np.uint8)


def goal_directions_env(obstacles, agents_xy, targets_xy, is_active, r):
    """One environment: obstacles [H, W], agents_xy / targets_xy [A, 2], is_active [A] -> uint8 [A, 2r+1, 2r+1]."""
    obstacles = np.asarray(obstacles) != 0
    agents_xy, targets_xy = np.asarray(agents_xy), np.asarray(targets_xy)
    is_active = np.asarray(is_active).astype(bool)
    A = agents_xy.shape[0]
    w = 2 * r + 1
    out = np.zeros((A, w, w), dtype=np.uint8)
    fields = {}
    for i in range(A):
        if is_active[i]:
            t = (int(targets_xy[i][0]), int(targets_xy[i][1]))
            if t not in fields:
                fields[t] = bfs_from(obstacles, *t)
            out[i] = directions_window(fields[t], int(agents_xy[i][0]), int(agents_xy[i][1]), r)
    return out


_WIDE_FIELDS = {}


def _wide_field(blocked, tx, ty):
    """bfs_from, remembered per (map, target): a queue BFS over a map wider than 64 takes a tenth of a second at 65k
    cells, and a test checks the same targets on the same map before and after its steps."""
    key = (blocked.shape, blocked.tobytes(), tx, ty)
    if key not in _WIDE_FIELDS:
        if len(_WIDE_FIELDS) >= 64:
            _WIDE_FIELDS.clear()
        _WIDE_FIELDS[key] = bfs_from(blocked, tx, ty).astype(np.int32)
    return _WIDE_FIELDS[key]


def goal_directions_reference(obstacles, agents_xy, targets_xy, is_active, r, envs=None):
    """Batched: obstacles [B, H, W], agents_xy / targets_xy [B, A, 2], is_active [B, A] -> uint8 [B, A, 2r+1, 2r+1].
    `envs`: only these environments (the other rows stay 0).  One search per distinct (env, target); the tiles of all
    agents are gathered from the padded fields at once."""
    obstacles, agents_xy, targets_xy = (np.asarray(v) for v in (obstacles, agents_xy, targets_xy))
    want = np.asarray(is_active).astype(bool).copy()
    B, A = agents_xy.shape[:2]
    H, W = obstacles.shape[1:]
    w = 2 * r + 1
    out = np.zeros((B, A, w, w), dtype=np.uint8)
    if envs is not None:
        keep = np.zeros(B, dtype=bool)
        keep[list(envs)] = True
        want &= keep[:, None]
    bi, ai = np.nonzero(want)
    if bi.size == 0:
        return out
    t = targets_xy[bi, ai].astype(np.int64)
    keys, inverse = np.unique((bi * H + t[:, 0]) * W + t[:, 1], return_inverse=True)
    kb, kx, ky = keys // (H * W), keys // W % H, keys % W
    pad = r + 1
    fields = np.full((len(keys), H + 2 * pad, W + 2 * pad), -1, dtype=np.int32)
    if W <= 64:
        for c in range(0, len(keys), 4096):
            s = slice(c, c + 4096)
            fields[s, pad:pad + H, pad:pad + W] = fields_packed(obstacles[kb[s]], np.stack([kx[s], ky[s]], 1))
    else:
        for k in range(len(keys)):
            fields[k, pad:pad + H, pad:pad + W] = _wide_field(obstacles[kb[k]] != 0, int(kx[k]), int(ky[k]))
    xy = agents_xy[bi, ai].astype(np.int64)     # the tile's corner in padded coordinates
    d = np.arange(2 * pad + 1)
    for c in range(0, bi.size, 8192):
        s = slice(c, c + 8192)
        tiles = fields[inverse.reshape(-1)[s, None, None], xy[s, 0, None, None] + d[None, :, None],
                       xy[s, 1, None, None] + d[None, None, :]]
        out[bi[s], ai[s]] = bits_from_tiles(tiles)
    return out
