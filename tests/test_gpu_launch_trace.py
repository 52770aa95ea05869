"""The host's launch sequence is pinned (tests/launch_trace.py): every
``_lib.call`` of the recorded steps — entry, scalar arguments, which pointers
are NULL, every slab job's (width, n_slabs, stride), the ``meta`` of the
priced launches, the stamp labels — equals tests/golden/launch_trace.json,
recorded before the GIN chain's host code was restructured.  A refactor of
ops.py / optim.py that changes what is launched, in what order or with what
slab-job ownership shows here as the first differing call."""
import pytest
import torch

import launch_trace

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def golden():
    return launch_trace.load()


def test_fixture_holds_every_case(golden):
    assert sorted(golden) == sorted(launch_trace.CASES)


@pytest.mark.parametrize("name", list(launch_trace.CASES))
def test_launch_sequence_unchanged(pkg, dev, golden, name):
    got, want = launch_trace.record(pkg, dev, name), golden[name]
    assert not pkg.ops._FINAL_PENDING and pkg.ops.OBSERVER is None
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, f"{name}: call {i} differs:\n  now      {a}\n  recorded {b}"
    assert len(got) == len(want), (name, len(got), len(want))
    assert len(got) > 0
