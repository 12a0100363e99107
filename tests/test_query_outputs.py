"""The one place a query's `out` tensor is checked or allocated (pogema_amd.queries.query_output), on CPU tensors: what
it allocates, what it hands back as is, and every reason it refuses an `out` -- always a ValueError naming the argument
and the expected dtype, shape and device."""
import numpy as np
import pytest
import torch

from pogema_amd.queries import QueryMixin, query_output

CPU = torch.device("cpu")
SHAPE = (3, 5, 2)
ACTIONS = (torch.int8, torch.int32, torch.int64)


def test_none_allocates_dtype_shape_and_device():
    t = query_output("out", None, torch.int32, SHAPE, CPU)
    assert t.dtype == torch.int32 and tuple(t.shape) == SHAPE and t.device == CPU and t.is_contiguous()
    first = query_output("out[actions]", None, ACTIONS, SHAPE, "cpu")   # several allowed: the first; a device by name
    assert first.dtype == torch.int8 and tuple(first.shape) == SHAPE


@pytest.mark.parametrize("dtype", ACTIONS)
def test_a_fitting_tensor_is_returned_as_is(dtype):
    t = torch.zeros(SHAPE, dtype=dtype)
    assert query_output("out[actions]", t, ACTIONS, SHAPE, CPU) is t
    assert query_output("out[actions]", t, dtype, list(SHAPE), CPU, align=1) is t
    assert not t.any()                                                    # untouched


def _misaligned_int32(n):
    """n int32 elements one byte past a 4-byte boundary (numpy hands torch the address as it is)."""
    raw = np.zeros(4 * n + 8, dtype=np.uint8)
    start = 1 + (-raw.ctypes.data) % 4
    t = torch.from_numpy(raw[start:start + 4 * n].view(np.int32))
    assert t.data_ptr() % 4 == 1 and t.is_contiguous()
    return t


BAD = {
    "dtype": lambda: torch.zeros(SHAPE, dtype=torch.int64),
    "float dtype": lambda: torch.zeros(SHAPE, dtype=torch.float32),
    "shape": lambda: torch.zeros(SHAPE[:-1] + (3,), dtype=torch.int32),
    "rank": lambda: torch.zeros(SHAPE[:-1], dtype=torch.int32),
    "non-contiguous view": lambda: torch.zeros(SHAPE[:-1] + (4,), dtype=torch.int32)[..., ::2],
    "another device": lambda: torch.zeros(SHAPE, dtype=torch.int32, device="meta"),
    "a list": lambda: [[0] * 5] * 3,
    "a numpy array": lambda: np.zeros(SHAPE, dtype=np.int32),
    "address off its element size": lambda: _misaligned_int32(30).view(SHAPE),
}


@pytest.mark.parametrize("why", sorted(BAD))
def test_refused_out(why):
    with pytest.raises(ValueError) as ei:
        query_output("out[distance]", BAD[why](), torch.int32, SHAPE, CPU)
    msg = str(ei.value)
    assert "out[distance]" in msg and "int32" in msg and str(SHAPE) in msg and "cpu" in msg, msg


def test_explicit_alignment():
    """`align` replaces the element size: int8 pairs at an even address, as pgx_visible_agents wants its offsets."""
    raw = torch.zeros(64, dtype=torch.int8)
    base = raw.data_ptr() % 2
    even, odd = raw[base:base + 30].view(SHAPE), raw[base + 1:base + 31].view(SHAPE)
    assert query_output("out[offset]", even, torch.int8, SHAPE, CPU, align=2) is even
    assert query_output("out[offset]", odd, torch.int8, SHAPE, CPU) is odd       # its element size is 1
    with pytest.raises(ValueError, match=r"out\[offset\].*aligned to 2 bytes"):
        query_output("out[offset]", odd, torch.int8, SHAPE, CPU, align=2)


def test_allowed_dtypes_are_all_named():
    with pytest.raises(ValueError) as ei:
        query_output("out[actions]", torch.zeros(SHAPE, dtype=torch.float32), ACTIONS, SHAPE, CPU)
    assert "int8 / int32 / int64" in str(ei.value)


class _NoEngine(QueryMixin):
    """A QueryMixin without an engine behind it: whatever reaches the library fails on the missing attributes."""
    batch, num_agents, window, device = 3, 5, 7, CPU
    _ACTION_CODE = {torch.int8: 0, torch.int32: 1, torch.int64: 2}


@pytest.mark.parametrize("call,names,out", [
    ("expert_actions", "(actions, distance)", (torch.zeros((3, 5), dtype=torch.int64), None)),
    ("expert_actions", "(actions, distance)", (None, torch.zeros((3, 5), dtype=torch.int32))),
    ("visible_agents", "(index, offset, count)",
     (torch.zeros((3, 5, 13), dtype=torch.int32), None, torch.zeros((3, 5), dtype=torch.int32))),
    ("pibt_actions", "(actions, next_xy)", (torch.zeros((3, 5), dtype=torch.int64), None)),
])
def test_none_inside_an_out_tuple_is_refused(call, names, out):
    """The caller gives every output or none: a None entry is not "allocate this one" (and not the C-ABI's "skip it")."""
    with pytest.raises(ValueError) as ei:
        getattr(_NoEngine(), call)(out=out)
    missing = names.strip("()").split(", ")[[t is None for t in out].index(True)]
    assert f"out[{missing}] is None" in str(ei.value) and names in str(ei.value)


@pytest.mark.parametrize("call,out", [("expert_actions", (1,)), ("visible_agents", (1, 2)), ("pibt_actions", (1, 2, 3))])
def test_an_out_tuple_of_the_wrong_length_is_refused(call, out):
    with pytest.raises(ValueError, match="out must be"):
        getattr(_NoEngine(), call)(out=out)
