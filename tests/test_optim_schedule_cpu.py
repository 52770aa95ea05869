"""optim.Schedule and the host side of optim.Adam's device-hyper mode (no GPU).

Schedule.factor(c) is the host restatement of the factor the Adam kernels
evaluate for themselves; here it is held against torch's own scheduler:
LambdaLR on a CPU SGD with the documented expression written out
independently, stepped after every optimizer step.  Both sides evaluate the
same expression in Python doubles, so the bar is equality.
"""
import copy
import itertools
import math

import pytest
import torch


def _documented(kind, warmup, total, warmup_start, min_ratio):
    """DESIGN.md §24's factor, written from the text (not from optim.py)."""
    def f(c):
        if c < warmup:
            return warmup_start + (1 - warmup_start) * c / warmup
        u = min(max((c - warmup) / max(total - warmup, 1), 0.0), 1.0)
        if kind == "constant":
            return 1.0
        if kind == "linear":
            return 1 - (1 - min_ratio) * u
        return min_ratio + (1 - min_ratio) * 0.5 * (1 + math.cos(math.pi * u))
    return f


@pytest.mark.parametrize("kind,warmup,total,min_ratio", list(itertools.product(
    ("constant", "linear", "cosine"), (0, 1, 5), (0, 5, 6, 30), (0.0, 0.1))))
def test_factor_matches_lambdalr(pkg, kind, warmup, total, min_ratio):
    lr, ws = 3e-3, 0.05
    sched = pkg.optim.Schedule(kind, warmup=warmup, total=total, warmup_start=ws,
                               min_ratio=min_ratio)
    p = torch.zeros(2, requires_grad=True)
    sgd = torch.optim.SGD([p], lr=lr)
    ref = torch.optim.lr_scheduler.LambdaLR(sgd, _documented(kind, warmup, total, ws, min_ratio))
    for c in range(40):  # past total, and total <= warmup among the cases
        assert ref.get_last_lr()[0] == lr * sched.factor(c), (c, kind, warmup, total)
        p.grad = torch.ones_like(p)
        sgd.step()
        ref.step()
    f = [sched.factor(c) for c in range(40)]
    if warmup:
        assert f[0] == ws and f[warmup] == 1.0 and f[:warmup + 1] == sorted(f[:warmup + 1])
    if kind != "constant" and total > warmup:
        assert abs(f[total] - min_ratio) < 1e-15 and f[39] == f[total]
    if kind == "constant":
        assert all(v == 1.0 for v in f[warmup:])


def test_argument_validation(pkg):
    O = pkg.optim
    p = [torch.zeros(3, requires_grad=True)]
    with pytest.raises(ValueError):
        O.Adam(p, lr=1e-3, max_grad_norm=-1.0)
    with pytest.raises(ValueError):
        O.Adam(p, lr=1e-3, max_grad_norm=float("nan"))
    with pytest.raises(ValueError):
        O.Schedule("cosine", warmup=-1)
    with pytest.raises(ValueError):
        O.Schedule("cosine", total=-3)
    with pytest.raises(ValueError):
        O.Schedule("exponential")
    with pytest.raises(ValueError):
        O.Schedule("linear", min_ratio=-0.5)
    with pytest.raises(TypeError):
        O.Adam(p, lr=1e-3, schedule=lambda c: 1.0)
    with pytest.raises(ValueError):  # a schedule cannot run from by-value arguments
        O.Adam(p, lr=1e-3, schedule=O.Schedule("linear", total=5), device_hyper=False)
    with pytest.raises(NotImplementedError):
        O.Adam(p, lr=1e-3, amsgrad=True)


def test_device_hyper_defaulting(pkg):
    O = pkg.optim
    p = [torch.zeros(3, requires_grad=True)]
    assert O.Adam(p, lr=1e-3).device_hyper is False
    assert O.Adam(p, lr=1e-3, decoupled=True).device_hyper is False
    assert O.Adam(p, lr=1e-3, max_grad_norm=1.0).device_hyper is True
    assert O.Adam(p, lr=1e-3, max_grad_norm=0.0).device_hyper is True
    assert O.Adam(p, lr=1e-3, skip_nonfinite=True).device_hyper is True
    assert O.Adam(p, lr=1e-3, schedule=O.Schedule()).device_hyper is True
    assert O.Adam(p, lr=1e-3, device_hyper=True).device_hyper is True
    assert O.Adam(p, lr=1e-3, device_hyper=False).device_hyper is False
    # the param groups keep torch's keys: state dicts stay interchangeable
    assert set(O.Adam(p, lr=1e-3, max_grad_norm=1.0).param_groups[0]) == \
        set(O.Adam(p, lr=1e-3).param_groups[0])
    # without a device block there is nothing to sync or read out
    with pytest.raises(pkg._lib.ScgibError):
        O.Adam(p, lr=1e-3).sync_hyper()
    with pytest.raises(pkg._lib.ScgibError):
        O.Adam(p, lr=1e-3).grad_norm


def test_state_dict_scgib_key(pkg):
    O = pkg.optim
    p = [torch.zeros(3, requires_grad=True)]
    plain = O.Adam(p, lr=1e-3)
    assert "scgib" not in plain.state_dict()  # as before
    opt = O.Adam(p, lr=1e-3, schedule=O.Schedule("linear", total=10))
    sd = opt.state_dict()
    assert sd["scgib"] == {"calls": 0, "skipped": 0}
    sd = copy.deepcopy(sd)
    sd["scgib"] = {"calls": 12, "skipped": 3}
    opt2 = O.Adam(p, lr=1e-3, schedule=O.Schedule("linear", total=10))
    opt2.load_state_dict(sd)
    assert opt2.state_dict()["scgib"] == {"calls": 12, "skipped": 3}
    assert sd["scgib"] == {"calls": 12, "skipped": 3}  # the caller's dict is left as it was
    # a dict without the key (torch's) loads as zeros, also over earlier counts
    theirs = torch.optim.Adam(p, lr=1e-3).state_dict()
    assert "scgib" not in theirs
    opt2.load_state_dict(theirs)
    assert opt2.state_dict()["scgib"] == {"calls": 0, "skipped": 0}
    # ours loads into torch's and into a by-value optimizer of ours
    torch.optim.Adam(p, lr=1e-3).load_state_dict(copy.deepcopy(sd))
    plain.load_state_dict(copy.deepcopy(sd))
    assert "scgib" not in plain.state_dict()
