"""The tail of the reference's training iteration on the device (train.py:157-167): the custom weight decay,
``clip_grad_norm_`` and ``torch.optim.Adam.step`` through csrc/optim.hip (``tts_optim_*``).

``Adam`` is a ``torch.optim.Optimizer``: ``param_groups``, ``zero_grad``, torch's LR schedulers and
``state_dict()`` / ``load_state_dict()`` (torch's state keys ``step``, ``exp_avg``, ``exp_avg_sq``, so a state
dict moves to and from ``torch.optim.Adam``) work as they do there.  ``step()`` is the Adam launch alone;
``step_fused(wd, grad_clip)`` is ``weight_decay(); check_update(); optimizer.step()`` in one pass over the
parameter set, bitwise the same as the three calls.  The forward and the backward stay the caller's torch.

``decay_`` and ``clip_`` are the stand-alone halves behind ``generic_utils.weight_decay`` / ``check_update``:
they take any list of CUDA float32 parameters (of this ``Adam`` or of any other optimizer).

Constructing an ``Adam`` needs no GPU (a scheduler can be driven on it); the first step does, and raises the
package's "no GPU" RuntimeError without one.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import _native

CHUNK = _native.TTS_OPTIM_CHUNK  # elements per chunk of work and per fp64 norm partial


def _device_tensor(t, what):
    if t.layout != torch.strided or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{what} must be a dense contiguous CUDA float32 tensor, got {t.dtype}, {t.layout} on "
                         f"{t.device}, strides {t.stride() if t.layout == torch.strided else None}")
    return t.data_ptr()


class _Engine:
    """One ``tts_optim`` handle: the chunk map of one tensor set and the calls on it."""

    def __init__(self):
        self._h = None
        self._sizes = None
        self._table = None

    def __del__(self):
        try:
            if self._h is not None:
                self._h[0].tts_optim_destroy(self._h[1])
        except Exception:
            pass

    def _prepare(self, rows):
        """rows: (p, g or None, m or None, v or None, step) per tensor -> (lib, handle, table, n, device)."""
        lib = _native.lib()  # raises without a GPU / library: no CPU fallback
        if not rows:
            raise ValueError("no parameters")
        ptrs = []
        for p, g, m, v, step in rows:
            pp = _device_tensor(p, "a parameter")
            n = p.numel()
            for t, what in ((g, "a gradient"), (m, "exp_avg"), (v, "exp_avg_sq")):
                if t is not None and t.numel() != n:
                    raise ValueError(f"{what} has {t.numel()} elements, its parameter {n}")
            ptrs.append((pp, _device_tensor(g, "a gradient") if g is not None else None,
                         _device_tensor(m, "exp_avg") if m is not None else None,
                         _device_tensor(v, "exp_avg_sq") if v is not None else None, n, int(step)))
        if self._h is None:
            h = ctypes.c_void_p()
            _native.check(lib.tts_optim_create(ctypes.byref(h)), "tts_optim_create")
            self._h = (lib, h)
        h = self._h[1]
        sizes = tuple(r[4] for r in ptrs)
        if sizes != self._sizes:
            self._sizes = None
            arr = (ctypes.c_int64 * len(sizes))(*sizes)
            _native.check(lib.tts_optim_set_tensors(h, arr, len(sizes), _native.stream_handle()),
                          "tts_optim_set_tensors")
            self._table = (_native.OptimTensor * len(sizes))()
            self._sizes = sizes
        table = self._table
        for i, (pp, gp, mp, vp, n, step) in enumerate(ptrs):
            e = table[i]
            e.p, e.g, e.m, e.v, e.numel, e.step = pp, gp, mp, vp, n, step
        return lib, h, table, len(ptrs), rows[0][0].device

    @staticmethod
    def _norm_outputs(device):
        return (torch.empty(2, dtype=torch.float64, device=device), torch.empty(2, dtype=torch.float32, device=device))

    def grad_norm(self, rows, max_norm, clip):
        """The norm (and the in-place clip), waited for: (norm64 [2] = sum of squares, norm; norm32 [2] = norm,
        coefficient; the fp64 norm as a Python float)."""
        lib, h, table, n, device = self._prepare(rows)
        n64, n32 = self._norm_outputs(device)
        host = ctypes.c_double()
        fn = lib.tts_optim_clip if clip else lib.tts_optim_grad_norm
        _native.check(fn(h, table, n, float(max_norm), ctypes.c_void_p(n64.data_ptr()), ctypes.c_void_p(n32.data_ptr()),
                         None, ctypes.byref(host), _native.stream_handle()),
                      "tts_optim_clip" if clip else "tts_optim_grad_norm")
        return n64, n32, host.value

    @staticmethod
    def _written(rows):
        """The library wrote the parameters through their pointers: their version counters say so, as after any
        in-place torch op (layers.LSTM keys its repacked weights on them)."""
        torch.autograd.graph.increment_version([r[0] for r in rows])

    def decay(self, rows, lr, wd):
        lib, h, table, n, _ = self._prepare(rows)
        _native.check(lib.tts_optim_decay(h, table, n, float(lr), float(wd), _native.stream_handle()),
                      "tts_optim_decay")
        self._written(rows)

    def adam(self, rows, lr, betas, eps):
        lib, h, table, n, _ = self._prepare(rows)
        _native.check(lib.tts_optim_adam(h, table, n, float(lr), float(betas[0]), float(betas[1]), float(eps),
                                         _native.stream_handle()), "tts_optim_adam")
        self._written(rows)

    def step(self, rows, lr, betas, eps, wd, max_norm):
        lib, h, table, n, device = self._prepare(rows)
        n64, n32 = self._norm_outputs(device)
        _native.check(lib.tts_optim_step(h, table, n, float(lr), float(betas[0]), float(betas[1]), float(eps),
                                         float(wd), float(max_norm), ctypes.c_void_p(n64.data_ptr()),
                                         ctypes.c_void_p(n32.data_ptr()), _native.stream_handle()), "tts_optim_step")
        self._written(rows)
        return n64, n32


_engines = {}  # the stand-alone calls: one engine per tensor set, by its sizes


def _shared_engine(params):
    key = tuple((p.numel(), p.device.index) for p in params)
    if key not in _engines:
        _engines[key] = _Engine()
    return _engines[key]


def decay_(params, lr, wd):
    """``p <- p + float32(-wd * lr) * p`` in place on every parameter (generic_utils.py:178-181)."""
    params = list(params)
    _shared_engine(params).decay([(p, None, None, None, 0) for p in params], lr, wd)


def clip_(params, max_norm):
    """``clip_grad_norm_(params, max_norm)`` in place: (the norm as a 0-dim CUDA float32 tensor, the fp64 norm as
    a Python float: the call waits for it).  Parameters without a gradient are skipped, as torch skips them."""
    params = list(params)
    rows = [(p, p.grad, None, None, 0) for p in params]
    _, n32, value = _shared_engine(params).grad_norm(rows, max_norm, clip=True)
    return n32[0], value


class Adam(torch.optim.Optimizer):
    """``torch.optim.Adam(params, lr, betas, eps, weight_decay=0)`` (train.py:454-457) on the device.

    One param group of contiguous CUDA float32 parameters.  After ``step_fused``, ``last_norm64`` is the fp64
    gradient norm as a 0-dim CUDA float64 tensor (the returned float32 one is its rounding); after a call that
    waited (``skip_nonfinite=True``) ``last_norm`` is the same as a Python float."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False):
        if amsgrad:
            raise NotImplementedError("amsgrad is not implemented (the reference never sets it)")
        if weight_decay != 0:
            raise ValueError("weight_decay inside Adam is not implemented: the reference passes 0 and decays with "
                             "generic_utils.weight_decay")
        if not lr > 0.0:
            raise ValueError(f"lr must be positive, got {lr}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"betas must lie in [0, 1), got {betas}")
        if not eps >= 0.0:
            raise ValueError(f"eps must not be negative, got {eps}")
        # torch.optim.Adam's own group keys, so that a state dict loads there (and its loads here)
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=0, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False)
        super().__init__(params, defaults)
        self._engine = _Engine()
        self.last_norm = self.last_norm64 = None

    def add_param_group(self, param_group):
        if self.param_groups:
            raise ValueError("one param group only")
        super().add_param_group(param_group)
        for p in self.param_groups[0]["params"]:  # (the device is checked by the first step: none is needed here)
            if p.dtype != torch.float32 or p.layout != torch.strided or not p.is_contiguous():
                raise ValueError("parameters must be dense contiguous float32 tensors")

    def _group(self):
        g = self.param_groups[0]
        if g.get("weight_decay", 0) != 0 or g.get("amsgrad") or g.get("maximize"):
            raise ValueError("weight_decay, amsgrad and maximize are not implemented")
        return g

    def _rows(self, group, make_state=True):
        """(p, g, m, v, the number of the coming step) per parameter; with ``make_state``, state is made where a
        gradient first shows (as torch makes it)."""
        rows = []
        for p in group["params"]:
            g = p.grad
            st = self.state.get(p, {}) if not make_state else self.state[p]
            if make_state and g is not None and not st:
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            rows.append((p, g, st.get("exp_avg"), st.get("exp_avg_sq"),
                         int(st["step"]) + 1 if g is not None and st else 0))
        return rows

    def _advance(self, group):
        for p in group["params"]:
            if p.grad is not None:
                self.state[p]["step"] += 1

    @torch.no_grad()
    def step(self, closure=None):
        """``optimizer.step()``: the Adam launch alone (``tts_optim_adam``)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        group = self._group()
        rows = self._rows(group)
        if any(r[1] is not None for r in rows):
            self._engine.adam(rows, group["lr"], group["betas"], group["eps"])
            self._advance(group)
        return loss

    @torch.no_grad()
    def step_fused(self, wd, grad_clip, skip_nonfinite=False):
        """``weight_decay(optimizer, wd); check_update(model, grad_clip); optimizer.step()`` (train.py:158-160) as
        one norm reduction and one pass (``tts_optim_step``).  Returns ``(grad_norm, current_lr)``, ``grad_norm`` a
        0-dim CUDA float32 tensor; nothing waits for the device.

        With ``skip_nonfinite`` the host reads the norm first (one wait, where the reference's
        ``np.isinf(grad_norm)`` waits too) and on a non-finite norm launches nothing more: parameters, gradients,
        state and step counters stay as they are.  Returns ``(grad_norm, current_lr, skip_flag)`` then."""
        group = self._group()
        lr = group["lr"]
        if skip_nonfinite:
            n64, n32, value = self._engine.grad_norm(self._rows(group, make_state=False), grad_clip, clip=False)
            self.last_norm, self.last_norm64 = value, n64[1]
            if not math.isfinite(value):
                return n32[0], lr, True
        n64, n32 = self._engine.step(self._rows(group), lr, group["betas"], group["eps"], wd, grad_clip)
        self.last_norm64 = n64[1]
        self._advance(group)
        return (n32[0], lr, False) if skip_nonfinite else (n32[0], lr)
