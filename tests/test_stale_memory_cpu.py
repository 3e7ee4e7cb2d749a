"""CPU tests of the poison helper (tests/stale_memory.py) that the stale-memory GPU tests stand on: the value every pattern gives in
every dtype, the index sentinel, restoration of what was patched, and that nothing but the empty allocators is touched."""
import math

import numpy as np
import pytest

import stale_memory as SM

torch = pytest.importorskip("torch")

FLOATS = [torch.float32, torch.float64, torch.bfloat16, torch.float16]


def allocators():
    """(name, call) for the three patched allocators, each making a (3, 5) tensor of the dtype."""
    return [("empty", lambda dt: torch.empty(3, 5, dtype=dt)),
            ("empty_like", lambda dt: torch.empty_like(torch.zeros(3, 5, dtype=dt))),
            ("new_empty", lambda dt: torch.zeros(2, dtype=torch.float32).new_empty((3, 5), dtype=dt))]


@pytest.mark.parametrize("dtype", FLOATS)
def test_ff_is_nan_in_every_float_type(dtype):
    with SM.poisoned(0xFF):
        for name, make in allocators():
            t = make(dtype)
            assert t.shape == (3, 5) and t.dtype == dtype, name
            assert bool(torch.isnan(t).all()), name


def test_ff_is_minus_one_in_the_integer_types_and_255_in_bytes():
    with SM.poisoned(0xFF):
        for name, make in allocators():
            for dt in (torch.int64, torch.int32, torch.int16, torch.int8):
                assert bool((make(dt) == -1).all()), (name, dt)
            assert bool((make(torch.uint8) == 0xFF).all()), name
            assert bool(make(torch.bool).view(torch.uint8).eq(0xFF).all()), name


def test_3c_is_finite_and_plausible():
    with SM.poisoned(0x3C):
        f32, bf16, f16 = torch.empty(7, dtype=torch.float32), torch.empty(7, dtype=torch.bfloat16), torch.empty(7, dtype=torch.float16)
        f64, i64, u8 = torch.empty(7, dtype=torch.float64), torch.empty(7, dtype=torch.int64), torch.empty(7, dtype=torch.uint8)
    want32 = np.frombuffer(bytes([0x3C] * 4), dtype=np.float32)[0]
    assert bool((f32 == float(want32)).all()) and math.isclose(float(want32), 0.0115, rel_tol=2e-2)
    assert bool((bf16.float() == float(np.frombuffer(bytes([0, 0, 0x3C, 0x3C]), dtype=np.float32)[0])).all())
    assert math.isclose(float(bf16[0]), 0.0115, rel_tol=2e-2)
    assert bool((f16 == float(np.frombuffer(bytes([0x3C] * 2), dtype=np.float16)[0])).all()) and math.isclose(float(f16[0]), 1.06, rel_tol=1e-2)
    assert bool(torch.isfinite(f64).all()) and bool((f64 == float(np.frombuffer(bytes([0x3C] * 8), dtype=np.float64)[0])).all())
    assert bool((i64 == 0x3C3C3C3C3C3C3C3C).all()) and bool((u8 == 0x3C).all())


def test_zero_pattern_is_the_clean_baseline():
    with SM.poisoned(0x00):
        for dt in FLOATS + [torch.int64, torch.uint8]:
            assert bool((torch.empty(9, dtype=dt) == 0).all()), dt


@pytest.mark.parametrize("byte", [0xFF, 0x3C, 0x00])
def test_index_tensors_take_the_sentinel(byte):
    """int32 / int64 get the caller's in-range value; bytes, int16 planes and floats keep the pattern."""
    with SM.poisoned(byte, sentinel=262144):
        for name, make in allocators():
            assert bool((make(torch.int64) == 262144).all()), name
            assert bool((make(torch.int32) == 262144).all()), name
            assert bool((make(torch.uint8) == byte).all()), name
            assert bool(make(torch.int16).view(torch.uint8).eq(byte).all()), name
            assert bool(make(torch.float32).view(torch.uint8).eq(byte).all()), name


def test_every_byte_is_poisoned_whatever_the_shape():
    with SM.poisoned(0x3C):
        for shape in [(), (1,), (5, 7), (2, 3, 4, 5)]:
            t = torch.empty(shape, dtype=torch.float32)
            assert t.shape == torch.Size(shape)
            assert bool(t.reshape(-1).view(torch.uint8).eq(0x3C).all()), shape
        assert torch.empty(0, 4).numel() == 0 and torch.empty((3, 0), dtype=torch.int64).shape == (3, 0)   # empty tensors are skipped
        cl = torch.empty(2, 3, 4, 5, memory_format=torch.channels_last)
        assert bool((cl == cl.flatten()[0]).all()) and math.isclose(float(cl.flatten()[0]), 0.0115, rel_tol=2e-2)


def test_other_constructors_are_untouched():
    with SM.poisoned(0xFF, sentinel=7):
        assert bool((torch.zeros(4, 4) == 0).all())
        assert bool((torch.zeros(4, dtype=torch.int64) == 0).all())
        assert torch.tensor([1.5, 2.5]).tolist() == [1.5, 2.5]
        assert torch.tensor([3, 4]).tolist() == [3, 4]
        assert torch.from_numpy(np.arange(6, dtype=np.int64)).tolist() == list(range(6))
        assert torch.from_numpy(np.ones(3, dtype=np.float32)).tolist() == [1.0, 1.0, 1.0]
        assert bool((torch.ones(3) == 1).all()) and bool((torch.full((3,), 2.0) == 2).all())
        assert torch.arange(4).tolist() == [0, 1, 2, 3]


def test_nothing_is_patched_outside_the_block():
    before = (torch.empty, torch.empty_like, torch.Tensor.new_empty, "new_empty" in vars(torch.Tensor))
    with SM.poisoned(0xFF):
        assert torch.empty is not before[0] and torch.empty_like is not before[1] and torch.Tensor.new_empty is not before[2]
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty, "new_empty" in vars(torch.Tensor)) == before
    torch.empty(4).fill_(1.0)   # (and the original still works)


def test_restored_after_an_exception():
    before = (torch.empty, torch.empty_like, torch.Tensor.new_empty, "new_empty" in vars(torch.Tensor))
    with pytest.raises(KeyError, match="boom"):
        with SM.poisoned(0x3C):
            assert float(torch.empty(1, dtype=torch.float16)[0]) > 1.0
            raise KeyError("boom")
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty, "new_empty" in vars(torch.Tensor)) == before


def test_nested_blocks_unwind_in_order():
    with SM.poisoned(0xFF):
        with SM.poisoned(0x00):
            pass
        assert bool(torch.isnan(torch.empty(3)).all())   # the outer poison is back, not the original
    assert torch.empty.__module__ != SM.__name__


def test_poison_tensor_fills_an_owned_buffer():
    ws = torch.zeros(64, dtype=torch.uint8)
    assert SM.poison_tensor(ws, 0xFF) is ws and bool((ws == 0xFF).all())
    x = torch.zeros(4, 4)
    SM.poison_tensor(x, 0xFF)
    assert bool(torch.isnan(x).all())
    ids = torch.zeros(5, dtype=torch.int64)
    SM.poison_tensor(ids, 0xFF, sentinel=11)
    assert ids.tolist() == [11] * 5
    SM.poison_tensor(ids, 0xFF)
    assert ids.tolist() == [-1] * 5
    part = x[1:3]                     # a contiguous view: only its own bytes
    SM.poison_tensor(part, 0x00)
    assert bool((x[1:3] == 0).all()) and bool(torch.isnan(x[0]).all()) and bool(torch.isnan(x[3]).all())
    assert SM.poison_tensor(None, 0xFF) is None
    with pytest.raises(AssertionError):
        SM.poison_tensor(x.t(), 0xFF)
