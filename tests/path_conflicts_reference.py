"""CPU reference of the path conflicts (docs/SPEC.md S26): the literal all-pairs statement of the section -- every pair
of agents at every step, a [K, A, A] mask per kind and env.  Test infrastructure only; the package never imports it."""
from __future__ import annotations

import numpy as np

KINDS = {"vertex": 1, "edge": 2, "follow": 4}


def as_steps(paths):
    """Either layout -> int64 [K, B, A, 2]: int32 [K, B, A, 2] (the plan layout) or int16 [B, A, K, 2] (the cells layout)."""
    paths = np.asarray(paths)
    if paths.dtype == np.int16:
        return paths.astype(np.int64).transpose(2, 0, 1, 3)
    assert paths.dtype == np.int32, paths.dtype
    return paths.astype(np.int64)


def takes_part(pos, targets_xy, is_active, H, W, vanish):
    """pos int64 [K + 1, B, A, 2] (pos[0]: the current cells) -> bool [K + 1, B, A]: part_h(i)."""
    inside = (pos[..., 0] >= 0) & (pos[..., 0] < H) & (pos[..., 1] >= 0) & (pos[..., 1] < W)
    part = inside & np.asarray(is_active).astype(bool)[None]
    if vanish:
        on_target = (pos == np.asarray(targets_xy)[None]).all(-1)
        before = np.zeros_like(on_target)
        before[1:] = np.logical_or.accumulate(on_target, 0)[:-1]     # some h' < h stood on the target
        part &= ~before
    return part


def incidences(paths, agents_xy, targets_xy, is_active, H, W, vanish):
    """The three kinds' incidences, each bool [K, B, A, A]: entry [h - 1, b, i, j] = agent i has (h, j)."""
    steps = as_steps(paths)
    pos = np.concatenate([np.asarray(agents_xy).astype(np.int64)[None], steps])          # [K + 1, B, A, 2]
    part = takes_part(pos, targets_xy, is_active, H, W, vanish)
    A = pos.shape[2]
    other = ~np.eye(A, dtype=bool)[None, None]
    now, was = pos[1:], pos[:-1]
    p_now = part[1:, :, :, None] & part[1:, :, None, :]                                    # part_h of both
    p_both = p_now & part[:-1, :, :, None] & part[:-1, :, None, :]                         # ... and part_{h-1} of both

    def same(a, b):      # a[.., i, :] == b[.., j, :]
        return (a[:, :, :, None, :] == b[:, :, None, :, :]).all(-1)

    moved = ~(now == was).all(-1)                                                          # pos_h[i] != pos_{h-1}[i]
    vertex = other & p_now & same(now, now)
    into = other & p_both & same(now, was) & moved[:, :, :, None]                          # i enters the cell j stood on
    edge = into & same(was, now)                                                           # ... and j the one i stood on
    follow = into & moved[:, :, None, :] & ~edge
    return vertex, edge, follow


def path_conflicts_reference(paths, agents_xy, targets_xy, is_active, H, W, kinds=("vertex", "edge"), vanish=False):
    """-> (first_step int32 [B, A], partner int32 [B, A], kind uint8 [B, A], count int32 [B, A])."""
    masks = dict(zip(("vertex", "edge", "follow"), incidences(paths, agents_xy, targets_xy, is_active, H, W, vanish)))
    K, B, A, _ = masks["vertex"].shape
    any_kind = np.zeros((K, B, A, A), dtype=bool)
    bits = np.zeros((K, B, A, A), dtype=np.uint8)
    for name in kinds:
        any_kind |= masks[name]
        bits |= masks[name].astype(np.uint8) * np.uint8(KINDS[name])
    count = any_kind.sum((0, 3)).astype(np.int32)
    per_step = any_kind.any(3)                                                             # [K, B, A]
    has = per_step.any(0)
    h0 = per_step.argmax(0)                                                                # the first step, 0-based
    b_idx, a_idx = np.meshgrid(np.arange(B), np.arange(A), indexing="ij")
    row = any_kind[h0, b_idx, a_idx]                                                       # [B, A, A]
    first_step = np.where(has, h0 + 1, -1).astype(np.int32)
    partner = np.where(has, row.argmax(-1), -1).astype(np.int32)
    kind = np.where(has, np.bitwise_or.reduce(bits[h0, b_idx, a_idx], -1), 0).astype(np.uint8)
    return first_step, partner, kind, count
