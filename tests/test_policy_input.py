"""CPU: the policy input (docs/SPEC.md S18).  The `other_goals` reference (tests/policy_input_reference.py) on cases
worked by hand, the channel parser and its refusals, the tables of the ctypes binding against the header, and the C-ABI
of the feature: pgx_policy_input is declared and exported, and its argument checks need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from pogema_amd import _lib
from pogema_amd.queries import parse_channels
from policy_input_reference import CHANNELS, other_goals_env, other_goals_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCABULARY = ("obstacles", "agents", "target", "other_goals", "up", "down", "left", "right")


def _plane(*cells, W=5):
    p = np.zeros((W, W), dtype=np.uint8)
    for u, v in cells:
        p[u, v] = 1
    return p


# ---- other_goals by hand: r = 2, a 5 x 5 window, the observer (agent 0) at (5, 5) = window cell (2, 2) ----------------
def test_target_inside_the_window():
    # agent 1 at (6, 5) is visible; its target (4, 6) lies at offset (-1, +1) of the observer
    got = other_goals_env([(5, 5), (6, 5)], [(9, 9), (4, 6)], [True, True], 2)
    assert got[0].tolist() == [[0, 0, 0, 0, 0],
                               [0, 0, 0, 1, 0],
                               [0, 0, 0, 0, 0],
                               [0, 0, 0, 0, 0],
                               [0, 0, 0, 0, 0]]
    # seen from agent 1 at (6, 5): agent 0 is visible, its target (9, 9) is clamped on both axes to the corner
    assert got[1].tolist() == [[0, 0, 0, 0, 0],
                               [0, 0, 0, 0, 0],
                               [0, 0, 0, 0, 0],
                               [0, 0, 0, 0, 0],
                               [0, 0, 0, 0, 1]]


def test_target_clamped_on_one_axis_and_on_both():
    # agent 1: target (5, 20), offset (0, +15) -> (0, +2): the right edge of the centre row
    # agent 2: target (0, 0), offset (-5, -5) -> (-2, -2): the top-left corner
    got = other_goals_env([(5, 5), (5, 6), (4, 4)], [(5, 5), (5, 20), (0, 0)], [True, True, True], 2)
    assert got[0].tolist() == [[1, 0, 0, 0, 0],
                               [0, 0, 0, 0, 0],
                               [0, 0, 0, 0, 1],
                               [0, 0, 0, 0, 0],
                               [0, 0, 0, 0, 0]]


def test_agent_just_outside_the_window_contributes_nothing():
    # |dy| = 3 > r for agent 1, |dx| = 3 > r for agent 2; agent 3 at |dx| = |dy| = 2 is the last one inside
    got = other_goals_env([(5, 5), (5, 8), (2, 5), (7, 3)], [(0, 0), (5, 5), (5, 5), (6, 6)], [True] * 4, 2)
    assert got[0].tolist() == [[0, 0, 0, 0, 0],
                               [0, 0, 0, 0, 0],
                               [0, 0, 0, 0, 0],
                               [0, 0, 0, 1, 0],
                               [0, 0, 0, 0, 0]]


def test_inactive_agent_contributes_nothing_and_sees_nothing():
    got = other_goals_env([(5, 5), (5, 6)], [(5, 4), (6, 6)], [True, False], 2)
    assert got[0].tolist() == [[0] * 5] * 5          # the only other agent is inactive
    assert got[1].tolist() == [[0] * 5] * 5          # an inactive observer sees nothing, though agent 0 is in its window
    got = other_goals_env([(5, 5), (5, 6)], [(5, 4), (6, 6)], [True, True], 2)
    assert np.array_equal(got[0], _plane((3, 3))) and np.array_equal(got[1], _plane((2, 0)))


def test_two_visible_agents_projecting_onto_one_cell():
    # agent 1's target (9, 5) clamps to offset (+2, 0); agent 2's target (7, 5) is at offset (+2, 0) exactly
    got = other_goals_env([(5, 5), (4, 5), (5, 4)], [(0, 9), (9, 5), (7, 5)], [True, True, True], 2)
    assert got[0].tolist() == [[0, 0, 0, 0, 0],
                               [0, 0, 0, 0, 0],
                               [0, 0, 0, 0, 0],
                               [0, 0, 0, 0, 0],
                               [0, 0, 1, 0, 0]]
    assert int(got[0].sum()) == 1


def test_visible_agents_target_on_the_observers_own_target_cell():
    # the observer's own target (5, 7) projects to (2, 4) and is NOT part of the plane ...
    alone = other_goals_env([(5, 5), (9, 9)], [(5, 7), (0, 0)], [True, True], 2)
    assert alone[0].tolist() == [[0] * 5] * 5
    # ... unless a visible agent's target falls there too: agent 1's target (5, 12) clamps to the same cell
    got = other_goals_env([(5, 5), (6, 6)], [(5, 7), (5, 12)], [True, True], 2)
    assert got[0].tolist() == [[0, 0, 0, 0, 0],
                               [0, 0, 0, 0, 0],
                               [0, 0, 0, 0, 1],
                               [0, 0, 0, 0, 0],
                               [0, 0, 0, 0, 0]]


def test_batched_reference_stacks_the_envs():
    agents = np.array([[(5, 5), (6, 5)], [(5, 5), (5, 8)]])
    targets = np.array([[(9, 9), (4, 6)], [(0, 0), (5, 5)]])
    active = np.array([[True, True], [True, True]])
    got = other_goals_reference(agents, targets, active, 2)
    assert got.shape == (2, 2, 5, 5) and got.dtype == np.uint8
    assert np.array_equal(got[0, 0], _plane((1, 3))) and not got[1].any()


# ---- the channel parser ------------------------------------------------------------------------------------------------
def test_vocabulary_and_codes():
    assert tuple(_lib.POLICY_CHANNELS) == VOCABULARY == CHANNELS
    for code, name in enumerate(VOCABULARY):
        assert _lib.POLICY_CHANNELS[name] == code
        assert parse_channels((name,)) == (code,) and parse_channels([name]) == (code,)
    assert _lib.NUM_CHANNELS == 8


def test_parser_keeps_the_order():
    assert parse_channels(VOCABULARY) == tuple(range(8))
    assert parse_channels(VOCABULARY[::-1]) == tuple(range(7, -1, -1))
    assert parse_channels(("right", "obstacles", "other_goals")) == (7, 0, 3)
    assert parse_channels(["target", "agents"]) == (2, 1)


def test_default_is_the_seven_plane_input():
    assert _lib.DEFAULT_POLICY_CHANNELS == ("obstacles", "agents", "target", "up", "down", "left", "right")
    assert parse_channels() == (0, 1, 2, 4, 5, 6, 7)
    import inspect
    from pogema_amd import Pogema, VecPogema
    assert inspect.signature(VecPogema.policy_input).parameters["channels"].default == _lib.DEFAULT_POLICY_CHANNELS
    assert inspect.signature(Pogema.policy_input).parameters["channels"].default == _lib.DEFAULT_POLICY_CHANNELS


@pytest.mark.parametrize("bad,needle", [
    ("up", "'up'"),                                    # a bare name is not a sequence of names
    (None, "None"),
    (5, "5"),
    ((), "got 0"),
    (VOCABULARY + ("up",), "got 9"),
    (("obstacles", "goal"), "channels[1] = 'goal'"),   # an unknown name
    (("obstacles", 3), "channels[1] = 3"),             # a code instead of a name
    (("up", "agents", "up"), "channels[2] = 'up' is given twice"),
])
def test_parser_refusals_name_the_entry_and_list_the_vocabulary(bad, needle):
    with pytest.raises(ValueError) as ei:
        parse_channels(bad)
    msg = str(ei.value)
    assert needle in msg
    for name in VOCABULARY:
        assert repr(name) in msg


# ---- the binding against the header ------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pogema_amd.h")).read(), flags=re.S)


def _define(text, name):
    m = re.search(rf"#define\s+{name}\s+(-?\d+)\b", text)
    assert m, f"{name} is not defined in include/pogema_amd.h"
    return int(m.group(1))


def test_tables_equal_the_header():
    import torch
    text = _header()
    for name, code in _lib.POLICY_CHANNELS.items():
        assert _define(text, f"PGX_CHANNEL_{name.upper()}") == code
    assert len(re.findall(r"#define\s+PGX_CHANNEL_", text)) == len(_lib.POLICY_CHANNELS) == _define(text, "PGX_NUM_CHANNELS")
    for dtype, name in ((torch.float32, "F32"), (torch.uint8, "U8"), (torch.bfloat16, "BF16"), (torch.float16, "F16")):
        assert _lib.OBS_DTYPES[dtype] == _define(text, f"PGX_OBS_{name}")
    assert _define(text, "PGX_ABI_VERSION") == _lib.PGX_ABI_VERSION == 6


def test_header_declares_and_library_exports(engine_lib):
    assert re.search(r"int\s+pgx_policy_input\s*\(\s*pgx_env\s*\*\s*env\s*,\s*const\s+int32_t\s*\*\s*channels\s*,"
                     r"\s*int32_t\s+num_channels\s*,\s*int32_t\s+dtype\s*,\s*void\s*\*\s*out\s*,\s*void\s*\*\s*stream\s*\)",
                     _header())
    assert "pgx_policy_input" in _lib.EXPORTED_SYMBOLS
    assert hasattr(engine_lib, "pgx_policy_input")


def test_invalid_arguments_need_no_device(engine_lib):
    """PGX_E_INVALID with a message for a null out or channel list, a count outside 1..8, a code outside 0..7 or given
    twice, an unknown dtype and a misaligned out: checked before the handle, so a NULL handle is never reached (a
    well-formed call on a NULL handle is refused too)."""
    buf = (C.c_uint8 * 64)()
    base = C.addressof(buf)
    base += -base % 16
    call = engine_lib.pgx_policy_input

    def refused(codes, n, dtype, out, needle):
        arr = (C.c_int32 * max(len(codes), 1))(*codes) if codes is not None else None
        assert call(None, arr, n, dtype, out, None) == -1
        assert needle in engine_lib.pgx_last_error().decode(), engine_lib.pgx_last_error().decode()

    refused([0], 1, 0, None, "out is null")
    refused(None, 1, 0, base, "channels is null")
    refused([0], 0, 0, base, "num_channels 0")
    refused(list(range(8)) + [0], 9, 0, base, "num_channels 9")
    refused([0, 8], 2, 0, base, "channels[1] = 8")
    refused([-1], 1, 0, base, "channels[0] = -1")
    refused([4, 1, 4], 3, 0, base, "channels[2] = 4 is given twice")
    refused([0], 1, 4, base, "bad dtype 4")
    refused([0], 1, -1, base, "bad dtype -1")
    refused([0], 1, 0, base + 2, "not 4-byte aligned")
    refused([0], 1, 2, base + 1, "not 2-byte aligned")
    refused([0], 1, 3, base + 1, "not 2-byte aligned")
    refused(list(range(8)), 8, 1, base + 1, "null handle")  # a byte format takes any address: the handle is reached
    refused([0, 1, 2, 4, 5, 6, 7], 7, 0, base, "null handle")
