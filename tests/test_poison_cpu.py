"""tests/poison.py itself: what it fills, what it leaves alone, that it restores
the allocators, and that the package allocates through nothing it misses."""
import glob
import math
import os
import re

import pytest
import torch

import poison
from conftest import ROOT

FLOATS = (torch.float32, torch.float64)
OTHERS = (torch.int32, torch.int64, torch.uint8, torch.bool)


def _spellings(dtype, shape=(3, 5)):
    """Every patched spelling, as name -> fresh uninitialised tensor."""
    base = torch.zeros(shape, dtype=dtype)
    other = torch.zeros(2, dtype=torch.int16)
    strides = torch.zeros(shape).stride()
    return {
        "torch.empty": torch.empty(shape, dtype=dtype),
        "torch.empty(*sizes)": torch.empty(*shape, dtype=dtype, device="cpu"),
        "torch.empty_like": torch.empty_like(base),
        "torch.empty_like(dtype=)": torch.empty_like(other.new_zeros(shape), dtype=dtype),
        "torch.empty_strided": torch.empty_strided(shape, strides, dtype=dtype),
        ".new_empty": base.new_empty(shape),
        ".new_empty(dtype=)": other.new_empty(shape, dtype=dtype),
        ".new_empty_strided": base.new_empty_strided(shape, strides),
    }


@pytest.mark.parametrize("dtype", FLOATS)
@pytest.mark.parametrize("value", [float("nan"), poison.SENTINEL])
def test_every_spelling_is_filled(dtype, value):
    with poison.poisoned(value, devices=("cpu",)):
        got = _spellings(dtype)
    assert {n.split("(")[0] for n in got} == set(poison.PATCHED_NAMES)
    for name, t in got.items():
        assert t.dtype == dtype and t.shape == (3, 5), name
        if math.isnan(value):
            assert bool(torch.isnan(t).all()), name
        else:
            assert bool((t == value).all()), name


def test_requires_grad_allocation_is_filled():
    with poison.poisoned(poison.SENTINEL, devices=("cpu",)):
        t = torch.empty(4, requires_grad=True)
    assert t.requires_grad and t.is_leaf and bool((t == poison.SENTINEL).all())


@pytest.mark.parametrize("dtype", OTHERS)
def test_integer_allocations_are_left_alone(dtype, monkeypatch):
    """A fill would call Tensor.fill_ on the fresh tensor; for these dtypes it
    is never called (their contents are whatever the allocator left)."""
    calls = []
    orig = torch.Tensor.fill_
    monkeypatch.setattr(torch.Tensor, "fill_",
                        lambda self, *a, **k: (calls.append(self.dtype), orig(self, *a, **k))[1])
    with poison.poisoned(float("nan"), devices=("cpu",)):
        got = _spellings(dtype)
    assert calls == []
    for name, t in got.items():
        assert t.dtype == dtype, name


@pytest.mark.parametrize("dtype", FLOATS)
def test_zero_element_and_other_device_allocations_are_left_alone(dtype, monkeypatch):
    calls = []
    orig = torch.Tensor.fill_
    monkeypatch.setattr(torch.Tensor, "fill_",
                        lambda self, *a, **k: (calls.append(self.shape), orig(self, *a, **k))[1])
    with poison.poisoned(float("nan"), devices=("cpu",)):
        got = _spellings(dtype, shape=(0, 5))
    assert calls == [] and all(t.numel() == 0 for t in got.values())
    with poison.poisoned(float("nan")):  # devices=("cuda",): CPU tensors untouched
        _spellings(dtype)
    assert calls == []


def test_callables_are_restored():
    before = [getattr(o, n) for o, n in poison.PATCHED]
    with poison.poisoned(1.0, devices=("cpu",)):
        inside = [getattr(o, n) for o, n in poison.PATCHED]
        assert all(a is not b for a, b in zip(before, inside))
    assert all(getattr(o, n) is f for (o, n), f in zip(poison.PATCHED, before))
    with pytest.raises(KeyError):
        with poison.poisoned(1.0, devices=("cpu",)):
            raise KeyError("inside")
    assert all(getattr(o, n) is f for (o, n), f in zip(poison.PATCHED, before))


def test_run_thrice_poisons_only_run():
    seen = []

    def build():
        return torch.empty(8)  # outside the poisoned region: never filled by the harness

    def run(state):
        seen.append(torch.empty(4).clone())
        return {"x": torch.arange(3.0), "none": None}

    orig = poison.poisoned
    try:
        poison.poisoned = lambda v: orig(v, devices=("cpu",))
        res = poison.run_thrice(build, run)
    finally:
        poison.poisoned = orig
    assert len(res) == 3 and len(seen) == 3
    assert bool(torch.isnan(seen[1]).all()) and bool((seen[2] == poison.SENTINEL).all())
    poison.assert_same(res)
    bad = [dict(res[0]), dict(res[1]), dict(res[2])]
    bad[1]["x"] = torch.tensor([0.0, float("nan"), 2.0])
    with pytest.raises(AssertionError):
        poison.assert_same(bad)
    bad[1]["x"] = torch.tensor([0.0, 1.0, 2.5])
    with pytest.raises(AssertionError):
        poison.assert_same(bad)


# -- the package allocates through nothing the harness misses -----------------

_PKG = os.path.join(ROOT, "s-cgib_amd")
# torch.empty*( / x.new_empty*( : allowed when patched
_EMPTY = re.compile(r"(?<![\w.])(torch\.empty\w*)\s*\(|(\.new_empty\w*)\s*\(")
# spellings that allocate uninitialised memory and are never patched
_FORBIDDEN = [
    (re.compile(r"\.new\s*\("), "Tensor.new("),
    (re.compile(r"\btorch\.(?:cuda\.)?(?:Float|Double|Half|BFloat16)Tensor\s*\((?!\s*\[)"),
     "legacy typed constructor with sizes"),
    (re.compile(r"\btorch\.Tensor\s*\((?!\s*\[)"), "torch.Tensor(sizes)"),
    (re.compile(r"\.resize_(?:as_)?\s*\("), "Tensor.resize_("),
    (re.compile(r"\.set_\s*\("), "Tensor.set_("),
    (re.compile(r"\b(?:Untyped|Typed|Float|Double)Storage\s*\("), "raw storage"),
    (re.compile(r"\bfrom\s+torch\s+import\b.*(?:\w*empty\w*|\*|\b\w+Tensor\b|\w*Storage\b)"),
     "from torch import of an allocator (an unpatched alias)"),
    (re.compile(r"\bimport\s+torch\s+as\b"), "import torch as"),
    # an allocator taken as a value (alias, default argument, getattr)
    (re.compile(r"(?<![\w.])torch\.empty\w*\b(?!\s*\()"), "torch.empty* not called in place"),
    (re.compile(r"getattr\s*\(\s*torch\b"), "getattr(torch, ...)"),
    (re.compile(r"\btorch\._C\._VariableFunctions\b|\btorch\.ops\.aten\.empty"), "aten empty"),
]


def _code_lines(path):
    """(lineno, text) of a source file without comments and docstring-ish
    string-only lines (so prose may mention a spelling)."""
    import io
    import tokenize
    with open(path, "rb") as fh:
        src = fh.read()
    keep = {}
    for tok in tokenize.tokenize(io.BytesIO(src).readline):
        if tok.type in (tokenize.COMMENT, tokenize.STRING, tokenize.ENCODING,
                        tokenize.NL, tokenize.NEWLINE, tokenize.INDENT, tokenize.DEDENT,
                        tokenize.ENDMARKER):
            continue
        if hasattr(tokenize, "FSTRING_MIDDLE") and tok.type == tokenize.FSTRING_MIDDLE:
            continue
        row = tok.start[0]
        have = keep.get(row, "")
        # (a space only between two words: "from torch import", not "torch . empty")
        sep = " " if have[-1:].isidentifier() and tok.string[:1].isidentifier() else ""
        keep[row] = have + sep + tok.string
    return sorted(keep.items())


def _scan(pkg=_PKG):
    used, forbidden = {}, []
    files = sorted(glob.glob(os.path.join(pkg, "*.py")))
    assert len(files) >= 10
    for path in files:
        rel = os.path.basename(path)
        for row, text in _code_lines(path):
            for m in _EMPTY.finditer(text):
                used.setdefault(m.group(1) or m.group(2), []).append(f"{rel}:{row}")
            for rx, what in _FORBIDDEN:
                if rx.search(text):
                    forbidden.append(f"{rel}:{row}: {what}")
    return used, forbidden


def test_package_allocates_only_through_patched_spellings():
    used, forbidden = _scan()
    print("uninitialised-allocation spellings in use:",
          {k: len(v) for k, v in sorted(used.items())})
    assert "torch.empty" in used and len(used["torch.empty"]) > 100  # the scan sees the sites
    outside = {k: v for k, v in used.items() if k not in poison.PATCHED_NAMES}
    assert not outside, outside
    assert not forbidden, forbidden


def test_scan_catches_a_foreign_spelling(tmp_path):
    """The scan itself has teeth: each unpatched spelling, dropped into a
    package-like directory, is reported."""
    cases = ["y = x.new(3, 4)", "y = torch.FloatTensor(3, 4)", "x.resize_(8)",
             "from torch import empty", "alloc = torch.empty", "y = torch.empty_permuted((2, 3), (0, 1))",
             "y = torch.cuda.FloatTensor(7)", "y = x.new_empty_foo(3)"]
    for i in range(10):
        (tmp_path / f"pad{i}.py").write_text("import torch\n" + "y = torch.empty(3)\n" * 11)
    used, forbidden = _scan(str(tmp_path))
    assert not forbidden and set(used) == {"torch.empty"}
    for i, line in enumerate(cases):
        (tmp_path / "case.py").write_text("import torch\n# x.new( in a comment is fine\n" + line + "\n")
        used, forbidden = _scan(str(tmp_path))
        outside = set(used) - poison.PATCHED_NAMES
        assert forbidden or outside, line
    (tmp_path / "case.py").write_text('import torch\nbuf = torch.FloatTensor([1.0])  # data, not sizes\n')
    used, forbidden = _scan(str(tmp_path))
    assert not forbidden
