"""CPU: the global state (docs/SPEC.md S20).  The numpy reference (tests/global_state_reference.py) on cases worked by
hand, the channel parser and its refusals, the id-range rule, the tables of the ctypes binding against the header, and the
C-ABI of the feature: pgx_global_state is declared and exported, and its argument checks need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from global_state_reference import CHANNELS, global_state_env, global_state_reference
from pogema_amd import _lib
from pogema_amd.queries import check_global_ids, parse_global_channels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCABULARY = ("obstacles", "agents", "targets", "agent_ids", "target_ids")
OBST = [[0, 1, 0, 0],
        [0, 0, 0, 1],
        [1, 0, 0, 0]]


# ---- the reference by hand: a 3 x 4 map ---------------------------------------------------------------------------------
def test_two_active_agents_share_a_target_lowest_id_wins():
    got = global_state_env(OBST, [(0, 0), (2, 3), (1, 1)], [(1, 2), (0, 3), (1, 2)], [1, 1, 1])
    assert got.shape == (5, 3, 4) and got.dtype == np.int32
    assert got[0].tolist() == OBST
    assert got[1].tolist() == [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1]]
    assert got[3].tolist() == [[1, 0, 0, 0], [0, 3, 0, 0], [0, 0, 0, 2]]
    assert got[2].tolist() == [[0, 0, 0, 1], [0, 0, 1, 0], [0, 0, 0, 0]]
    assert got[4].tolist() == [[0, 0, 0, 2], [0, 0, 1, 0], [0, 0, 0, 0]]   # agents 0 and 2 want (1, 2): id 1, not 3


def test_hidden_agent_is_absent_from_all_four_planes():
    got = global_state_env(OBST, [(0, 0), (2, 3)], [(1, 2), (2, 3)], [1, 0])   # agent 1 finished on its target
    assert got[1].tolist() == [[1, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]]
    assert got[3].tolist() == [[1, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]]
    assert got[2].tolist() == [[0, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 0]]
    assert got[4].tolist() == [[0, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 0]]


def test_ghost_stands_nowhere_but_keeps_its_target():
    got = global_state_env(OBST, [(0, 0), (1, 1)], [(2, 2), (0, 2)], [3, 1])   # agent 0 is a ghost
    assert got[1].tolist() == [[0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 0]]
    assert got[3].tolist() == [[0, 0, 0, 0], [0, 2, 0, 0], [0, 0, 0, 0]]
    assert got[2].tolist() == [[0, 0, 1, 0], [0, 0, 0, 0], [0, 0, 1, 0]]
    assert got[4].tolist() == [[0, 0, 2, 0], [0, 0, 0, 0], [0, 0, 1, 0]]


def test_agent_standing_on_another_agents_target():
    got = global_state_env(OBST, [(1, 2), (0, 0)], [(2, 1), (1, 2)], [1, 1])   # agent 0 stands on agent 1's target
    assert got[1, 1, 2] == 1 and got[2, 1, 2] == 1
    assert got[3, 1, 2] == 1 and got[4, 1, 2] == 2                            # who stands there, whose target it is
    assert got[3].tolist() == [[2, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 0]]
    assert got[4].tolist() == [[0, 0, 0, 0], [0, 0, 2, 0], [0, 1, 0, 0]]


def test_two_ghostless_agents_on_one_cell_lowest_id_wins():
    # (the engine never puts two agents of the occupancy array on one cell; the definition still says who wins)
    got = global_state_env(OBST, [(1, 1), (1, 1)], [(0, 0), (0, 2)], [1, 1])
    assert got[3, 1, 1] == 1 and int(got[1].sum()) == 1


def test_batched_reference_stacks_the_envs():
    obst = np.array([OBST, np.zeros((3, 4), dtype=int)])
    got = global_state_reference(obst, np.array([[(0, 0)], [(2, 2)]]), np.array([[(1, 1)], [(0, 3)]]), np.array([[1], [0]]))
    assert got.shape == (2, 5, 3, 4)
    assert np.array_equal(got[0], global_state_env(OBST, [(0, 0)], [(1, 1)], [1])) and not got[1].any()


# ---- the channel parser ------------------------------------------------------------------------------------------------
def test_vocabulary_and_codes():
    assert tuple(_lib.GLOBAL_CHANNELS) == VOCABULARY == CHANNELS
    for code, name in enumerate(VOCABULARY):
        assert _lib.GLOBAL_CHANNELS[name] == code
        assert parse_global_channels((name,)) == (code,) and parse_global_channels([name]) == (code,)
    assert _lib.NUM_GLOBAL_CHANNELS == 5
    assert parse_global_channels(VOCABULARY[::-1]) == (4, 3, 2, 1, 0)
    assert parse_global_channels(("agent_ids", "obstacles")) == (3, 0)


def test_default_is_the_three_binary_planes():
    assert _lib.DEFAULT_GLOBAL_CHANNELS == ("obstacles", "agents", "targets")
    assert parse_global_channels() == (0, 1, 2)
    import inspect
    from pogema_amd import Pogema, VecPogema
    assert inspect.signature(VecPogema.global_state).parameters["channels"].default == _lib.DEFAULT_GLOBAL_CHANNELS
    assert inspect.signature(Pogema.global_state).parameters["channels"].default == _lib.DEFAULT_GLOBAL_CHANNELS


@pytest.mark.parametrize("bad,needle", [
    ("agents", "'agents'"),                              # a bare name is not a sequence of names
    (None, "None"),
    ((), "got 0"),
    (VOCABULARY + ("agents",), "got 6"),
    (("obstacles", "target"), "channels[1] = 'target'"),  # policy_input's name, not this vocabulary's
    (("obstacles", 1), "channels[1] = 1"),
    (("targets", "agents", "targets"), "channels[2] = 'targets' is given twice"),
])
def test_parser_refusals_name_the_entry_and_list_the_vocabulary(bad, needle):
    with pytest.raises(ValueError) as ei:
        parse_global_channels(bad)
    msg = str(ei.value)
    assert needle in msg
    for name in VOCABULARY:
        assert repr(name) in msg


def test_id_range_rule_in_python():
    import torch
    ids, binary = parse_global_channels(("obstacles", "target_ids")), parse_global_channels()
    check_global_ids(ids, torch.uint8, 255)
    check_global_ids(ids, torch.bfloat16, 256)
    for dtype in (torch.float16, torch.float32):
        check_global_ids(ids, dtype, _lib.MAX_AGENTS)
    with pytest.raises(ValueError, match="at most 255"):
        check_global_ids(ids, torch.uint8, 256)
    with pytest.raises(ValueError, match="at most 256"):
        check_global_ids(parse_global_channels(("agent_ids",)), torch.bfloat16, 257)
    check_global_ids(binary, torch.uint8, 1024)          # no id channel: any count
    check_global_ids(binary, torch.bfloat16, 1024)
    # the limits are the formats' own: every id up to the limit survives the round trip, the next one does not
    assert torch.arange(257, dtype=torch.float32).to(torch.bfloat16).to(torch.float32).tolist() == list(range(257))
    assert float(torch.tensor(257.0).to(torch.bfloat16)) != 257.0
    assert torch.arange(1025, dtype=torch.float32).to(torch.float16).to(torch.float32).tolist() == list(range(1025))


# ---- the binding against the header ------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pogema_amd.h")).read(), flags=re.S)


def _define(text, name):
    m = re.search(rf"#define\s+{name}\s+(-?\d+)\b", text)
    assert m, f"{name} is not defined in include/pogema_amd.h"
    return int(m.group(1))


def test_tables_equal_the_header():
    text = _header()
    for name, code in _lib.GLOBAL_CHANNELS.items():
        assert _define(text, f"PGX_GLOBAL_{name.upper()}") == code
    assert _define(text, "PGX_NUM_GLOBAL_CHANNELS") == _lib.NUM_GLOBAL_CHANNELS == len(_lib.GLOBAL_CHANNELS)
    assert _define(text, "PGX_GLOBAL_BAND_CELLS") == _lib.GLOBAL_BAND_CELLS >= _define(text, "PGX_MAX_SIDE")
    assert _lib.GLOBAL_ID_MAX == {_define(text, "PGX_OBS_U8"): _define(text, "PGX_GLOBAL_ID_MAX_U8"),
                                  _define(text, "PGX_OBS_BF16"): _define(text, "PGX_GLOBAL_ID_MAX_BF16")}
    assert _define(text, "PGX_ABI_VERSION") == _lib.PGX_ABI_VERSION == 6   # additive: the version does not move


def test_header_declares_and_library_exports(engine_lib):
    assert re.search(r"int\s+pgx_global_state\s*\(\s*pgx_env\s*\*\s*env\s*,\s*const\s+int32_t\s*\*\s*channels\s*,"
                     r"\s*int32_t\s+num_channels\s*,\s*int32_t\s+dtype\s*,\s*void\s*\*\s*out\s*,\s*void\s*\*\s*stream\s*\)",
                     _header())
    for name in ("pgx_global_state", "pgx_global_state_check"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(engine_lib, name)


def _aligned_buffer():
    buf = (C.c_uint8 * 64)()
    base = C.addressof(buf)
    return buf, base + (-base % 16)


def test_invalid_arguments_need_no_device(engine_lib):
    """PGX_E_INVALID with a message for a null out or channel list, a count outside 1..5, a code outside 0..4 or given
    twice, an unknown dtype and a misaligned out: checked before the handle, so a NULL handle is never reached (a
    well-formed call on a NULL handle is refused too)."""
    buf, base = _aligned_buffer()
    call = engine_lib.pgx_global_state

    def refused(codes, n, dtype, out, needle):
        arr = (C.c_int32 * max(len(codes), 1))(*codes) if codes is not None else None
        assert call(None, arr, n, dtype, out, None) == -1
        assert needle in engine_lib.pgx_last_error().decode(), engine_lib.pgx_last_error().decode()

    refused([0], 1, 0, None, "out is null")
    refused(None, 1, 0, base, "channels is null")
    refused([0], 0, 0, base, "num_channels 0")
    refused(list(range(5)) + [0], 6, 0, base, "num_channels 6")
    refused([0, 5], 2, 0, base, "channels[1] = 5")
    refused([-1], 1, 0, base, "channels[0] = -1")
    refused([4, 1, 4], 3, 0, base, "channels[2] = 4 is given twice")
    refused([0], 1, 4, base, "bad dtype 4")
    refused([0], 1, -1, base, "bad dtype -1")
    refused([0], 1, 0, base + 2, "not 4-byte aligned")
    refused([0], 1, 2, base + 1, "not 2-byte aligned")
    refused([0], 1, 3, base + 1, "not 2-byte aligned")
    refused(list(range(5)), 5, 1, base + 1, "null handle")   # a byte format takes any address: the handle is reached
    refused([0, 1, 2], 3, 0, base, "null handle")
    assert buf[0] == 0


def test_id_range_rule_in_c_at_the_edges(engine_lib):
    """The rule needs the agent count, which a NULL handle does not have: pgx_global_state_check is the entry's own
    argument check for a given count, the function pgx_global_state runs on the handle's."""
    _, base = _aligned_buffer()
    check = engine_lib.pgx_global_state_check

    def rc(agents, codes, dtype, out=base):
        return check(agents, (C.c_int32 * len(codes))(*codes), len(codes), dtype, out)

    U8, BF16, F16, F32 = 1, 2, 3, 0
    for ids in ([3], [4], [0, 4, 1], [3, 4]):
        assert rc(255, ids, U8) == 0
        assert rc(256, ids, U8) == -1
        msg = engine_lib.pgx_last_error().decode()
        assert "pgx_global_state" in msg and "uint8" in msg and "255" in msg and "256" in msg, msg
        assert rc(256, ids, BF16) == 0
        assert rc(257, ids, BF16) == -1
        msg = engine_lib.pgx_last_error().decode()
        assert "bfloat16" in msg and "256" in msg and "257" in msg, msg
        assert rc(1024, ids, F16) == 0 and rc(1024, ids, F32) == 0
    assert rc(1024, [0, 1, 2], U8) == 0 and rc(1024, [2], BF16) == 0   # no id channel: any count
    # the other checks come first, with the entry's messages
    assert rc(300, [3], U8, None) == -1 and "out is null" in engine_lib.pgx_last_error().decode()
    assert rc(300, [3, 3], U8) == -1 and "given twice" in engine_lib.pgx_last_error().decode()
    assert rc(300, [3], 7) == -1 and "bad dtype 7" in engine_lib.pgx_last_error().decode()
    assert rc(300, [3], BF16, base + 1) == -1 and "not 2-byte aligned" in engine_lib.pgx_last_error().decode()
