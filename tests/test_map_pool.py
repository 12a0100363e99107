"""CPU: the map pool's C-ABI entry points are declared and refuse a null handle; VecPogema refuses malformed pools and
pools combined with an explicit map before any device is needed; the host restatement of the map choice equals the
formula of docs/SPEC.md S10."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from pogema_amd import GridConfig, Semantics, VecPogema, _lib
from pogema_amd.vec_env import parse_map_pool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POOL_SYMBOLS = ("pgx_set_map_pool", "pgx_reset_pool", "pgx_regenerate_pool", "pgx_get_map_index")


def test_pool_entry_points_declared_and_exported(engine_lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pogema_amd.h")).read(), flags=re.S)
    for name in POOL_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", text), f"{name} not declared in include/pogema_amd.h"
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(engine_lib, name)
    assert engine_lib.pgx_abi_version() == 6  # additive: the ABI version stays


def test_pool_entry_points_refuse_null_handle(engine_lib):
    maps = (C.c_uint8 * 16)()
    cap = (C.c_int32 * 1)()
    out = (C.c_int32 * 4)()
    mask = (C.c_uint8 * 4)()
    assert engine_lib.pgx_set_map_pool(None, maps, 1, cap, None) == -1
    assert "pgx_set_map_pool" in engine_lib.pgx_last_error().decode()
    assert engine_lib.pgx_reset_pool(None, 1, None, 10, None) == -1
    assert engine_lib.pgx_regenerate_pool(None, mask, 1, 3, None, None) == -1
    assert engine_lib.pgx_get_map_index(None, out, None) == -1
    assert "pgx_get_map_index" in engine_lib.pgx_last_error().decode()


def test_parse_accepts_tensors_arrays_rows_and_text():
    a = np.zeros((3, 4, 5), np.uint8)
    a[1, 2, 3] = 7
    for given in (a, a.astype(bool), torch.from_numpy(a), torch.from_numpy(a).bool()):
        t = parse_map_pool(given)
        assert t.dtype == torch.uint8 and tuple(t.shape) == (3, 4, 5)
        assert int(t.sum()) == 1 and int(t[1, 2, 3]) == 1
    t = parse_map_pool(["..#\n#..", [[0, 1, 0], [0, 0, 1]]])
    assert t.tolist() == [[[0, 0, 1], [1, 0, 0]], [[0, 1, 0], [0, 0, 1]]]


@pytest.mark.parametrize("pool,needle", [
    (["..\n..", "...\n..."], "one shape"),                             # ragged: maps of two shapes
    ([[[0, 0], [0]]], "rectangular"),                                  # ragged rows inside one map
    (["a.A\n...", "...\n..."], "map 0 has symbols"),                   # agent letters
    (["...\n...", "..@\n..$"], "map 1 has symbols"),                   # possible start / target cells
    (np.zeros((2, 4, 4), np.int32), "uint8 or bool"),
    (np.zeros((4, 4), np.uint8), "[M, H, W]"),
    ([], "non-empty"),
])
def test_malformed_pools_are_refused(pool, needle):
    with pytest.raises(ValueError, match=re.escape(needle)):
        parse_map_pool(pool)
    with pytest.raises(ValueError, match=re.escape(needle)):
        VecPogema(GridConfig(num_agents=1, obs_radius=2), batch=2, map_pool=pool)


@pytest.mark.parametrize("kw", [
    dict(map="....\n...."),
    dict(map=[[0, 0, 0, 0], [0, 0, 0, 0]], agents_xy=[[0, 0]], targets_xy=[[1, 1]]),
    dict(map="@...\n...$"),
])
def test_pool_with_explicit_map_or_agents_is_refused(kw):
    pool = np.zeros((2, 2, 4), np.uint8)
    with pytest.raises(ValueError, match="map_pool cannot be combined"):
        VecPogema(GridConfig(num_agents=1, obs_radius=2, **kw), batch=2, map_pool=pool)


def test_pool_with_numpy_generator_is_not_implemented():
    with pytest.raises(NotImplementedError, match="generator_rng"):
        VecPogema(GridConfig(num_agents=1, obs_radius=2), batch=2, map_pool=np.zeros((1, 4, 4), np.uint8),
                  semantics=Semantics(generator_rng="numpy"))


def test_pool_shape_passes_the_side_limit_first():
    with pytest.raises(ValueError, match="sides up to"):
        VecPogema(GridConfig(num_agents=1, obs_radius=2), batch=1,
                  map_pool=np.zeros((1, 2, _lib.MAX_SIDE + 1), np.uint8))


def test_host_map_choice_equals_the_spec_formula():
    from oracle.generator_oracle import instance_hash
    from oracle.pogema_oracle import splitmix64
    from pogema_amd.generator_host import pool_pick
    rng = np.random.default_rng(4)
    for _ in range(200):
        seed, env, epoch = int(rng.integers(0, 2 ** 63)), int(rng.integers(0, 10 ** 6)), int(rng.integers(0, 50))
        M = int(rng.integers(1, 1000))
        h0 = instance_hash(seed, env, epoch, 0)
        want = ((splitmix64(h0 ^ 0x504F4F4C00000000) >> 32) * M) >> 32
        assert pool_pick(seed, env, epoch, M) == want < M
    # a one-map pool always picks map 0, and the choice spreads over a larger pool
    assert {pool_pick(1, e, 0, 1) for e in range(50)} == {0}
    assert len({pool_pick(1, e, 0, 8) for e in range(400)}) == 8
