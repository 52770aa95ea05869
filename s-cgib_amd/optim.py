"""Adam on the device in one launch per 80 tensors (scgib_adam_step).

Drop-in for the optimizer every reference script builds,
``torch.optim.Adam(model.parameters(), lr=args.lr, weight_decay=5e-5)``
(exp_pretraining.py, exp_molhiv.py:53/:89/:160 ...): same hyper-parameters,
same per-parameter state (``step`` / ``exp_avg`` / ``exp_avg_sq``, so
state_dicts are interchangeable with torch's), the arithmetic of torch's
fused Adam, and HIP-graph capturable (the tensor table is passed by value in
the kernel arguments; ``step`` stays on the device).  amsgrad, maximize and
sparse gradients are not supported (the reference does not use them).
HIP only — no CPU fallback.

Built as the reference builds it, the hyper-parameters travel by value too
and a captured step keeps them for good.  ``decoupled=True`` makes it AdamW
(torch's fused arithmetic).  ``schedule``, ``max_grad_norm``,
``skip_nonfinite`` or ``device_hyper=True`` move the hyper-parameters into a
device block that the kernels read: a learning-rate schedule,
global-norm gradient clipping and the skipping of a non-finite step then run
inside a replayed step, and ``sync_hyper()`` carries host edits of
``param_groups`` to the device between replays.
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib
from . import ops


class Schedule:
    """The factor a step's learning rate is multiplied by: ``lr_t = lr *
    factor(c)``, ``c`` the number of ``step()`` calls before this one (so the
    schedule of ``scheduler.step()`` after every ``optimizer.step()``).

    ``c < warmup``: ``warmup_start + (1 - warmup_start) c / warmup``; after
    it, with ``u = clamp((c - warmup) / max(total - warmup, 1), 0, 1)``:
    ``constant`` 1, ``linear`` ``1 - (1 - min_ratio) u``, ``cosine``
    ``min_ratio + (1 - min_ratio) 0.5 (1 + cos(pi u))``.  ``factor`` is the
    host restatement of what the Adam kernels evaluate, in double, for
    themselves."""

    def __init__(self, kind="constant", warmup=0, total=0, warmup_start=0.0, min_ratio=0.0):
        if kind not in _lib.SCHED_KINDS:
            raise ValueError(f"Schedule: unknown kind {kind!r} (one of {sorted(_lib.SCHED_KINDS)})")
        if int(warmup) != warmup or int(total) != total or warmup < 0 or total < 0:
            raise ValueError(f"Schedule: warmup={warmup} and total={total} must be integers >= 0")
        for name, v in (("warmup_start", warmup_start), ("min_ratio", min_ratio)):
            if not (math.isfinite(v) and v >= 0.0):
                raise ValueError(f"Schedule: {name}={v} must be finite and >= 0")
        self.kind, self.warmup, self.total = kind, int(warmup), int(total)
        self.warmup_start, self.min_ratio = float(warmup_start), float(min_ratio)

    def factor(self, c):
        c = int(c)
        if c < self.warmup:
            return self.warmup_start + (1 - self.warmup_start) * c / self.warmup
        u = (c - self.warmup) / max(self.total - self.warmup, 1)
        u = 0.0 if u < 0.0 else (1.0 if u > 1.0 else u)
        if self.kind == "linear":
            return 1 - (1 - self.min_ratio) * u
        if self.kind == "cosine":
            return self.min_ratio + (1 - self.min_ratio) * 0.5 * (1 + math.cos(math.pi * u))
        return 1.0

    def __repr__(self):
        return (f"Schedule({self.kind!r}, warmup={self.warmup}, total={self.total}, "
                f"warmup_start={self.warmup_start}, min_ratio={self.min_ratio})")


_HYPER_WORDS = ctypes.sizeof(_lib.OptimHyper) // 8


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 amsgrad=False, maximize=False, decoupled=False, max_grad_norm=None,
                 skip_nonfinite=False, schedule=None, device_hyper=None):
        if amsgrad or maximize:
            raise NotImplementedError("scgib Adam: amsgrad / maximize are not implemented")
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= weight_decay:
            raise ValueError(f"invalid Adam hyper-parameters lr={lr} eps={eps} wd={weight_decay}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"invalid betas {betas}")
        if max_grad_norm is not None and not (math.isfinite(max_grad_norm) and max_grad_norm >= 0.0):
            raise ValueError(f"invalid max_grad_norm {max_grad_norm}")
        if schedule is not None and not isinstance(schedule, Schedule):
            raise TypeError("scgib Adam: schedule must be an optim.Schedule")
        wants = max_grad_norm is not None or bool(skip_nonfinite) or schedule is not None
        if device_hyper is None:
            device_hyper = wants
        elif not device_hyper and wants:
            raise ValueError("scgib Adam: schedule / max_grad_norm / skip_nonfinite read the "
                             "hyper-parameters from the device (device_hyper=False contradicts them)")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self._max = int(_lib.query("scgib_adam_max_tensors"))
        self.decoupled = bool(decoupled)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.schedule = schedule
        self.device_hyper = bool(device_hyper)
        self._state_blk = self._hyper_blk = self._last_lr = self._norm_ws = None
        self._synced = None          # the host values the device block holds
        self._counts = (0, 0)        # calls, skipped to put into a block not yet allocated

    # -- device-hyper mode: the blocks, their read-outs and the host -> device copy --
    def _device(self):
        for group in self.param_groups:
            for p in group["params"]:
                return p.device
        raise _lib.ScgibError("scgib Adam: no parameters")

    def _blocks(self):
        """The zeroed device blocks (scgib_optim_state | one scgib_optim_hyper
        per group | last_lr), allocated at their first use, outside capture."""
        if not self.device_hyper:
            raise _lib.ScgibError("scgib Adam: built without device_hyper (no schedule, "
                                  "max_grad_norm or skip_nonfinite): there is no device block")
        n = len(self.param_groups)
        if self._state_blk is not None and self._last_lr.numel() == n:
            return
        dev = self._device()
        if dev.type != "cuda":
            raise _lib.ScgibError("scgib Adam: parameters must be HIP tensors (no CPU fallback)")
        if torch.cuda.is_current_stream_capturing():
            raise _lib.ScgibError("scgib Adam: the device hyper-parameter block must be allocated "
                                  "outside capture (call sync_hyper() or step() once before it)")
        if self._state_blk is None:
            self._state_blk = torch.zeros(_lib.OPTIM_STATE_WORDS, dtype=torch.int64, device=dev)
            self._state_blk[3:5] = torch.tensor(self._counts, dtype=torch.int64)
        self._hyper_blk = torch.zeros(n * _HYPER_WORDS, dtype=torch.int64, device=dev)
        self._last_lr = torch.zeros(n, dtype=torch.float64, device=dev)
        self._synced = None

    def _host_hyper(self):
        out = []
        mgn = -1.0 if self.max_grad_norm is None else self.max_grad_norm
        for group in self.param_groups:
            s = group.get("schedule") or self.schedule or _CONSTANT
            b1, b2 = group["betas"]
            out.append((float(group["lr"]), float(b1), float(b2), float(group["eps"]),
                        float(group["weight_decay"]), s.warmup_start, s.min_ratio, mgn,
                        s.warmup, s.total, _lib.SCHED_KINDS[s.kind], 0))
        return tuple(out)

    def sync_hyper(self):
        """Copy the param groups' current lr / betas / eps / weight_decay,
        schedule and max_grad_norm to the device block the kernels read: one
        small host -> device copy on the current stream, ordered after the
        replays already enqueued there.  Not under capture.  An eager step()
        calls it when a value changed; between replays the caller does."""
        self._blocks()
        if torch.cuda.is_current_stream_capturing():
            raise _lib.ScgibError("scgib Adam: sync_hyper() is a host copy, not capturable")
        vals = self._host_hyper()
        arr = (_lib.OptimHyper * len(vals))(*[_lib.OptimHyper(*v) for v in vals])
        host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.int64)
        self._hyper_blk.copy_(host)
        self._synced = vals

    @property
    def grad_norm(self):
        """fp32 device scalar: the last step's global gradient norm, before clipping."""
        self._blocks()
        return self._state_blk[1:2].view(torch.float32)[0]

    @property
    def clip_coef(self):
        """fp32 device scalar: what the last step multiplied the gradients by."""
        self._blocks()
        return self._state_blk[1:2].view(torch.float32)[1]

    @property
    def last_lr(self):
        """fp64 device tensor, one entry per group: the last step's lr_t."""
        self._blocks()
        return self._last_lr

    @property
    def calls(self):
        """int64 device scalar: step() calls so far, skipped ones included."""
        self._blocks()
        return self._state_blk[3]

    @property
    def skipped(self):
        """int64 device scalar: steps skipped for a non-finite gradient norm."""
        self._blocks()
        return self._state_blk[4]

    def state_dict(self):
        sd = super().state_dict()
        if self.device_hyper:  # one host read at save time
            calls, skipped = (self._counts if self._state_blk is None
                              else self._state_blk[3:5].tolist())
            sd["scgib"] = {"calls": int(calls), "skipped": int(skipped)}
        return sd

    def load_state_dict(self, state_dict):
        extra = state_dict.get("scgib") or {}
        super().load_state_dict({k: v for k, v in state_dict.items() if k != "scgib"})
        # (a dict without the key, torch's for one, loads as zeros)
        self._counts = (int(extra.get("calls", 0)), int(extra.get("skipped", 0)))
        if self._state_blk is not None:
            self._state_blk[3:5] = torch.tensor(self._counts, dtype=torch.int64)
        self._synced = None

    def _entries(self, group):
        out = []
        for p in group["params"]:
            if p.grad is None:
                continue
            if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                raise _lib.ScgibError("scgib Adam: parameters must be contiguous fp32 HIP tensors")
            if p.grad.is_sparse:
                raise _lib.ScgibError("scgib Adam: sparse gradients are not supported")
            if p.grad.dtype != torch.float32 or not p.grad.is_contiguous():
                p.grad = p.grad.float().contiguous()
            st = self.state[p]
            if not st:
                st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            elif st["step"].device != p.device or st["step"].dtype != torch.float32:
                st["step"] = st["step"].to(device=p.device, dtype=torch.float32)
            out.append(_lib.AdamTensor(p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(),
                                       st["exp_avg_sq"].data_ptr(), st["step"].data_ptr(),
                                       p.numel()))
        return out

    def _unaliased(self, jobs, ents):
        """The final reduces this step launches write the weight-gradient
        buffers whose views the backward handed autograd; the step is right
        only if those views ARE the gradients it steps on (autograd took them
        over as .grad without a copy, and nobody re-bound .grad since).  Host
        pointer arithmetic: every job's output range must lie inside the
        (merged) gradient ranges of ``ents``.  Returns '' or a description of
        the first range that does not, with the parameters it may belong to."""
        spans = sorted((t.grad, t.grad + 4 * t.numel) for ent in ents for t in ent)
        merged = []
        for lo, hi in spans:
            if merged and lo <= merged[-1][1]:
                merged[-1][1] = max(merged[-1][1], hi)
            else:
                merged.append([lo, hi])
        outs = [(j.out, j.out + 4 * j.width) for j in jobs]
        for ji, (lo, hi) in enumerate(outs):
            if any(a <= lo and hi <= b for a, b in merged):
                continue
            # the floats of this output no gradient covers, and the parameters
            # of that size whose gradient lies outside every job's output
            gap = (hi - lo - sum(max(0, min(hi, b) - max(lo, a)) for a, b in merged)) // 4
            plist = [(gi, pi, p) for gi, group in enumerate(self.param_groups)
                     for pi, p in enumerate(group["params"]) if p.grad is not None]
            cand = [f"group {gi} parameter {pi} {tuple(p.shape)}" for gi, pi, p in plist
                    if p.numel() == gap and not any(
                        a <= p.grad.data_ptr() < b for a, b in outs)]
            return (f"{gap} of the {(hi - lo) // 4} floats reduce job {ji} writes are no "
                    f"parameter's .grad (un-aliased gradient: {', '.join(cand) or 'unknown'})")
        return ""

    def _norm(self, ents, dev, st):
        """The global gradient norm of the step: one scgib_grad_norm launch
        per table over every group's gradients in table order."""
        flat = [t for ent in ents for t in ent]
        tables = [flat[i0:i0 + self._max] for i0 in range(0, len(flat), self._max)] or [[]]
        arrs = [(_lib.AdamTensor * len(t))(*t) if t else None for t in tables]
        need = max(int(_lib.query("scgib_grad_norm_ws_doubles", int(_lib.query(
            "scgib_grad_norm_chunks", ctypes.cast(a, ctypes.c_void_p), len(t))) if t else 0))
            for a, t in zip(arrs, tables))
        if self._norm_ws is None or self._norm_ws.numel() < need:
            self._norm_ws = torch.empty(need, dtype=torch.float64, device=dev)
        cnt = ops.counters(dev, "grad_norm", 1)
        for i, (a, t) in enumerate(zip(arrs, tables)):
            _lib.call("scgib_grad_norm", ctypes.cast(a, ctypes.c_void_p) if t else None, len(t),
                      ops._p(self._norm_ws), ops._p(cnt), ops._p(self._hyper_blk),
                      ops._p(self._state_blk), int(i == 0), int(i == len(tables) - 1), st)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        ops.check_handoff()  # an earlier step's hand-off wait gave up: raise before updating
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        # every group's table first: an exception here (a sparse gradient, a CPU
        # parameter) leaves the pending final reduces where the next step or the
        # end of ops.fuse_final_into_step finds them
        ents = [self._entries(group) for group in self.param_groups]
        dyn = self.device_hyper
        normed = dyn and (self.max_grad_norm is not None or self.skip_nonfinite)
        if dyn:
            self._blocks()
            if self._host_hyper() != self._synced:
                if torch.cuda.is_current_stream_capturing():
                    raise _lib.ScgibError(
                        "scgib Adam: a param group's hyper-parameters changed since the last "
                        "sync_hyper(); a captured step reads them from the device and would "
                        "not see the change: call sync_hyper() before the capture")
                self.sync_hyper()
        # the final weight-gradient reduces left to this step (ops.fuse_final_into_step):
        # one list of ops.SlabWork per backward; they keep the slabs referenced
        pending = []
        for group in self.param_groups:
            pending += ops.take_final(group["params"][0].device) if group["params"] else []
        jobs = [w.job for work in pending for w in work]
        if jobs:
            stale = self._unaliased(jobs, ents)
            if stale:  # the reduces all the same (nothing is lost), no update
                ops.reduce_pending(pending)
                raise _lib.ScgibError(
                    "scgib Adam: a final weight-gradient reduce left to this step "
                    "(ops.fuse_final_into_step) does not write the gradients it steps on: " + stale +
                    ".  A .grad was copied or re-bound between the backward and the step; the "
                    "reduces were launched, the parameters are unchanged")
        fused = False
        if normed:  # the norm needs every reduced gradient: the reduces first, then the norm
            ops.reduce_pending(pending)
            fused = True
            self._norm(ents, self._device(), ops._stream())
        flags = (_lib.OPTIM_NORM if normed else 0) | (_lib.OPTIM_SKIP if normed and
                                                      self.skip_nonfinite else 0)
        dec = self.decoupled
        # the last launch of a device-hyper step advances the call counter
        last = max((gi for gi, ent in enumerate(ents) if ent), default=None)

        def hyper_args(gi, advance):
            return (ctypes.c_void_p(self._hyper_blk.data_ptr() + 8 * _HYPER_WORDS * gi),
                    ops._p(self._state_blk), ctypes.c_void_p(self._last_lr.data_ptr() + 8 * gi),
                    flags | (_lib.OPTIM_ADVANCE if advance else 0), int(dec))

        for gi, group in enumerate(self.param_groups):
            ent = ents[gi]
            if not ent:
                continue
            dev = group["params"][0].device
            b1, b2 = group["betas"]
            byval = (float(group["lr"]), float(b1), float(b2), float(group["eps"]),
                     float(group["weight_decay"]))
            st = ops._stream()
            if (jobs and not fused and len(self.param_groups) == 1 and len(ent) <= self._max
                    and len(jobs) <= int(_lib.query("scgib_adam_reduce_max_jobs"))
                    and max(j.n_slabs for j in jobs) >= ops.FUSE_FINAL_MIN_SLABS):
                # the reduce and this step in one launch (same bits)
                table = (_lib.AdamTensor * len(ent))(*ent)
                jt = (_lib.SlabJob * len(jobs))(*jobs)
                head = (ctypes.cast(table, ctypes.c_void_p), len(ent),
                        ctypes.cast(jt, ctypes.c_void_p), len(jobs))
                cnt = ops._p(ops.counters(dev, "adam", 1))
                if dyn:
                    _lib.call("scgib_adam_step_reduce_dyn", *head, *hyper_args(gi, True), cnt, st)
                else:
                    _lib.call("scgib_adamw_step_reduce" if dec else "scgib_adam_step_reduce",
                              *head, *byval, cnt, st)
                fused = True
                continue
            if pending and not fused:  # not fusable here: the reduces first, as unfused
                ops.reduce_pending(pending)
                fused = True
            starts = range(0, len(ent), self._max)
            for i0 in starts:
                chunk = ent[i0:i0 + self._max]
                table = (_lib.AdamTensor * len(chunk))(*chunk)
                # one word per stream (launches on a stream are ordered, and each
                # leaves it zero): not per optimizer, so new optimizers reuse it
                cnt = ops.counters(dev, "adam", 1)
                head = (ctypes.cast(table, ctypes.c_void_p), len(chunk))
                if dyn:
                    _lib.call("scgib_adam_step_dyn", *head,
                              *hyper_args(gi, gi == last and i0 == starts[-1]), ops._p(cnt), st)
                else:
                    _lib.call("scgib_adamw_step" if dec else "scgib_adam_step", *head, *byval,
                              ops._p(cnt), st)
        if pending and not fused:  # (no gradients here at all)
            ops.reduce_pending(pending)
        if dyn and last is None:  # nothing to step: the call still counts
            _lib.call("scgib_adam_step_dyn", None, 0, *hyper_args(0, True),
                      ops._p(ops.counters(self._device(), "adam", 1)), ops._stream())
        pending = None  # the slabs stay referenced until the launches are enqueued
        ops.stamp("adam_end")
        return loss


_CONSTANT = Schedule()
