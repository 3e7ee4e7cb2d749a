"""Stale-memory poisoning for the tests (a plain module, like tests/dropout_model.py): make every buffer that the code under test takes
from ``torch.empty`` hold a chosen byte pattern instead of whatever the allocator returns, so that a kernel that reads a slot before
writing it, or leaves a corner of an output unwritten, gives a different answer than on fresh (zero) memory.

    with poisoned(0xFF, sentinel=cfg.image_vocab_size):
        out = model.compute_logits(x)

Byte patterns (every byte of the tensor is the pattern):
    0xFF   NaN in f32, f64, bf16 and f16; -1 in the integer types
    0x3C   finite and plausible: 0.0115 in f32 and bf16, 1.06 in f16 -- for stale data that passes through fmaxf, comparisons or flags,
           where a NaN is swallowed
    0x00   the clean baseline

Index tensors (int32 and int64) get ``sentinel`` in every element instead when one is given: an unwritten id read back as an index must
show up as a wrong answer, not run off the end of a table.  The tests pass the mask token id, ``config.image_vocab_size``: a valid index
wherever ids are read, and a value no finished output may contain.  The narrower integer types keep the byte pattern: uint8 is the type
of the byte workspaces and caches, int16 carries 16-bit float planes.

Nothing is patched outside the ``with`` block; the originals are restored on exit, also when the block raises."""
import contextlib

import torch

PATTERNS = (0xFF, 0x3C)     # the poisons; 0x00 is the clean run
INDEX_DTYPES = (torch.int32, torch.int64)


def poison_tensor(t, byte, sentinel=None):
    """Fill every byte of the contiguous tensor ``t`` with ``byte`` (index tensors: every element with ``sentinel``, when given) -> t.
    For buffers a test owns or an object caches (a model's workspace, an evaluator's cache, a rollout's cache, trunk and branch)."""
    if t is None or t.numel() == 0 or t.device.type == "meta":
        return t
    assert 0 <= int(byte) <= 0xFF, byte
    assert t.is_contiguous(), "poison_tensor: contiguous tensors only"
    if sentinel is not None and t.dtype in INDEX_DTYPES:
        t.fill_(int(sentinel))
    else:
        t.reshape(-1).view(torch.uint8).fill_(int(byte))
    return t


@contextlib.contextmanager
def poisoned(byte, sentinel=None):
    """Inside the block torch.empty, torch.empty_like and Tensor.new_empty return tensors poisoned as by poison_tensor."""
    empty, empty_like = torch.empty, torch.empty_like
    own_new_empty = "new_empty" in vars(torch.Tensor)
    new_empty = torch.Tensor.new_empty

    def wrap(fn):
        def alloc(*args, **kwargs):
            t = fn(*args, **kwargs)
            if t.numel() and t.device.type != "meta" and not t.is_contiguous():   # (channels_last and the like: the tensor owns its storage)
                flat = empty(0, dtype=t.dtype, device=t.device).set_(t.untyped_storage())
                poison_tensor(flat, byte, sentinel)
                return t
            return poison_tensor(t, byte, sentinel)
        alloc.__name__ = getattr(fn, "__name__", "alloc")
        return alloc

    torch.empty, torch.empty_like = wrap(empty), wrap(empty_like)
    torch.Tensor.new_empty = wrap(new_empty)
    try:
        yield
    finally:
        torch.empty, torch.empty_like = empty, empty_like
        if own_new_empty:
            torch.Tensor.new_empty = new_empty
        else:
            del torch.Tensor.new_empty
