"""Poisoned workspaces: fill every uninitialised float allocation with a value.

The package allocates all of its workspaces (slabs, BatchNorm partials, tile
statistics, saved activations, gradient outputs, loss partials) from Python
with ``torch.empty`` / ``torch.empty_like``; no kernel allocates.  So a kernel
that reads an element nobody wrote reads whatever the caching allocator left
there -- usually zeros in a fresh test process.  ``poisoned`` replaces that
accident by a deterministic fill, and ``run_thrice`` runs one op on clean
memory, on NaN and on the project's sentinel: every op here is bitwise
reproducible (fixed-order reductions), so the three results must be equal.

Only non-empty fp32 / fp64 tensors are filled.  Integer, bool and byte
allocations (indices, flags, tickets, raw workspaces) are left alone on
purpose: a poisoned index or ticket could send a kernel out of bounds or into
a wait, and this harness must not be able to fault or hang a device even when
it finds a bug.
"""
import contextlib
import functools

import torch

SENTINEL = -7.0
_FLOATS = (torch.float32, torch.float64)

# (owner, attribute): every spelling of an uninitialised allocation that the
# package may use (tests/test_poison_cpu.py scans the package against this).
PATCHED = (
    (torch, "empty"),
    (torch, "empty_like"),
    (torch, "empty_strided"),
    (torch.Tensor, "new_empty"),
    (torch.Tensor, "new_empty_strided"),
)
PATCHED_NAMES = frozenset(
    ("torch." if owner is torch else ".") + name for owner, name in PATCHED)


def _filling(fn, value, devices):
    @functools.wraps(fn)
    def alloc(*args, **kwargs):
        out = fn(*args, **kwargs)
        if (isinstance(out, torch.Tensor) and out.dtype in _FLOATS and out.numel() > 0
                and out.device.type in devices):
            out.detach().fill_(value)
        return out
    return alloc


@contextlib.contextmanager
def poisoned(value, devices=("cuda",)):
    """While active, every fp32 / fp64 tensor with at least one element that
    Python allocates uninitialised on one of ``devices`` (device types) comes
    back filled with ``value``.  The original callables return, by identity,
    on exit -- an exception inside the block included."""
    devices = tuple(devices)
    saved = [(owner, name, getattr(owner, name)) for owner, name in PATCHED]
    try:
        for owner, name, fn in saved:
            setattr(owner, name, _filling(fn, value, devices))
        yield
    finally:
        for owner, name, fn in saved:
            setattr(owner, name, fn)


def _to_cpu(res):
    out = {}
    for k, v in res.items():
        if v is None:
            out[k] = None
        elif isinstance(v, torch.Tensor):
            out[k] = v.detach().cpu().clone()
        else:
            out[k] = torch.as_tensor(v)
    return out


def run_thrice(build, run):
    """``build()`` -> fresh inputs, modules and seeds (outside the poisoned
    region); ``run(state)`` -> dict of result tensors (inside it).  Three
    build + run rounds: clean, NaN-poisoned, sentinel-poisoned.  Returns the
    three result dicts on the CPU, taken after a synchronize."""
    results = []
    for value in (None, float("nan"), SENTINEL):
        state = build()
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        ctx = contextlib.nullcontext() if value is None else poisoned(value)
        with ctx:
            res = run(state)
            if torch.cuda.is_available():
                torch.cuda.synchronize()
        results.append(_to_cpu(res))
    return results


def assert_same(results):
    """The contract: every result tensor of the poisoned runs is
    ``torch.equal`` to the clean run's, and whatever is finite there is finite
    in them.  A float tensor that holds NaN / inf in the clean run itself
    (a per-task metric without both classes) can never be ``torch.equal`` to
    anything, NaN != NaN: those are compared bit for bit instead, which is
    stricter, not looser."""
    clean = results[0]
    for tag, other in zip(("nan", "sentinel"), results[1:]):
        assert other.keys() == clean.keys(), (tag, sorted(clean), sorted(other))
        for k, a in clean.items():
            b = other[k]
            if a is None:
                assert b is None, (tag, k)
                continue
            assert b is not None, (tag, k)
            assert a.shape == b.shape and a.dtype == b.dtype, (tag, k, a.shape, b.shape)
            if a.is_floating_point():
                fin = torch.isfinite(a)
                assert bool(torch.isfinite(b[fin]).all()), (tag, k, "non-finite")
                if not bool(fin.all()):
                    # bit pattern comparison keeps the check exact where the
                    # clean run itself holds NaN / inf
                    ia = a.contiguous().view(torch.int32 if a.dtype == torch.float32
                                             else torch.int64)
                    ib = b.contiguous().view(ia.dtype)
                    assert torch.equal(ia, ib), (tag, k)
                    continue
            assert torch.equal(a, b), (tag, k, _first_diff(a, b))


def _first_diff(a, b):
    bad = (a != b) | (a != a) | (b != b) if a.is_floating_point() else (a != b)
    idx = bad.nonzero()
    if idx.numel() == 0:
        return None
    i = tuple(idx[0].tolist())
    return {"mismatches": int(bad.sum()), "of": a.numel(), "first": i,
            "clean": a[i].item(), "poisoned": b[i].item()}
