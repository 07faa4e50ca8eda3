"""The reference's criteria on the device (train.py:462-465, layers/losses.py), for evaluation and training.

``L1LossMasked`` / ``MSELossMasked`` keep the reference's ``(input, target, length)`` call, ``L1Loss`` /
``MSELoss`` / ``BCEWithLogitsLoss`` torch.nn's ``(input, target)``; each returns a 0-dim CUDA float32 tensor.
They run ``tts_loss_masked`` / ``tts_loss_bce_logits`` (csrc/losses.hip): one read of every valid element of
both operands, fp64 arithmetic, a fixed summation order.  After a call

  ``last_value``         the loss as a Python float: the fp64 quotient the returned tensor is the rounding of
  ``last_count``         the number of terms (``mask.sum()`` as an int)
  ``last_sum``           the fp64 sum over all terms
  ``last_per_sentence``  CUDA float64 [B]: each sentence's sum (BCEWithLogitsLoss: [1], the whole sum)

Rows at and beyond a sentence's length are not read, so a NaN there does not reach the result (the
reference's ``NaN * 0`` does).

With grad mode on and an ``input`` that requires grad, the call joins autograd: the forward is the same (the
same kernels, bitwise the same values), and ``loss.backward()`` (train.py:157) runs ``tts_loss_backward``, one
elementwise launch on the current stream that waits for nothing: every valid element's gradient formed in
fp64 and rounded once, ``+0.0`` on the padding rows, NaN everywhere when no sentence has a valid row (the
reference's ``inf * 0``).  Such an input must be a CUDA float32 tensor (a silent ``.to()`` would cut the
graph); the target and the lengths get no gradient (the reference sets ``target.requires_grad = False``), and
there is no double backward.  Without a GPU the classes raise the package's "no GPU" RuntimeError; there is
no CPU fallback.
"""
from __future__ import annotations

import ctypes

import torch
from torch.autograd.function import once_differentiable

from . import _native


def _operand(t):
    t = torch.as_tensor(t)
    return t.detach().to("cuda", torch.float32)


def _differentiable(input):
    """True when the call has to join autograd; such an input is used as it is, so it must be CUDA float32."""
    if not (torch.is_grad_enabled() and isinstance(input, torch.Tensor) and input.requires_grad):
        return False
    if not input.is_cuda or input.dtype != torch.float32:
        raise ValueError(f"an input that requires grad must be a CUDA float32 tensor, got {input.dtype} on "
                         f"{input.device}: a conversion here would cut the graph")
    return True


class _Criterion(torch.autograd.Function):
    """``crit._forward`` as it is, with ``tts_loss_backward`` behind it.  ``_forward`` returns the loss and what
    the gradient needs: the fp32 CUDA operands it ran on, their pitches, the device table of valid elements per
    sentence (None: all), B, T * D and the number of terms."""

    @staticmethod
    def forward(ctx, input, crit, target, length):
        loss, (x, xp, y, yp, n_valid, B, per, count) = crit._forward(input, target, length, grad=True)
        ctx.save_for_backward(x, y, *(() if n_valid is None else (n_valid,)))
        ctx.call = (crit.KIND, xp, yp, B, per, count, input.shape)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        x, y, *n_valid = ctx.saved_tensors
        kind, xp, yp, B, per, count, shape = ctx.call
        gout = grad_output.to(x.device, torch.float32).contiguous()  # (the 0-dim tensor autograd hands over, as it is)
        grad = torch.empty(B, per, dtype=torch.float32, device=x.device)
        _native.check(_native.lib().tts_loss_backward(
            kind, ctypes.c_void_p(x.data_ptr()), xp, ctypes.c_void_p(y.data_ptr()), yp,
            ctypes.c_void_p(n_valid[0].data_ptr()) if n_valid else None, B, per, count,
            ctypes.c_void_p(gout.data_ptr()), ctypes.c_void_p(grad.data_ptr()), per, _native.stream_handle()),
            "tts_loss_backward")
        return grad.view(shape), None, None, None


class _Loss:
    def __init__(self):
        self._h = None
        self.last_value = self.last_count = self.last_sum = self.last_per_sentence = None

    def _handle(self):
        lib = _native.lib()  # raises without a GPU / library: no CPU fallback
        if self._h is None:
            h = ctypes.c_void_p()
            _native.check(lib.tts_loss_create(ctypes.byref(h)), "tts_loss_create")
            self._h = (lib, h)
        return self._h

    def __del__(self):
        try:
            if self._h is not None:
                self._h[0].tts_loss_destroy(self._h[1])
        except Exception:
            pass

    def cuda(self):  # the reference moves its criteria to the device (train.py:494-495)
        return self

    def forward(self, *args):
        return self(*args)

    def _run(self, input, target, length=None):
        if _differentiable(input):
            return _Criterion.apply(input, self, target, length)
        return self._forward(input, target, length)[0]


def _rows(t):
    """t as [B][T][D] with contiguous rows: (tensor kept alive, B, T, D, batch pitch in elements)."""
    if t.dim() != 3:
        t = t.reshape(1, 1, -1)
    B, T, D = t.shape
    if t.stride(2) != 1 or t.stride(1) != D or (B > 1 and t.stride(0) < T * D):
        t = t.contiguous()
    return t, B, T, D, (t.stride(0) if B > 1 else T * D)


class _Elementwise(_Loss):
    KIND = None

    def _forward(self, input, target, length, grad=False):
        lib, h = self._handle()
        x, B, T, D, xp = _rows(_operand(input))
        y, By, Ty, Dy, yp = _rows(_operand(target))
        if (B, T, D) != (By, Ty, Dy):
            raise ValueError(f"input {tuple(x.shape)} and target {tuple(y.shape)} differ in shape")
        lens = n_valid = None
        if length is not None:
            lens = [int(v) for v in torch.as_tensor(length).reshape(-1)]
            if len(lens) != B:
                raise ValueError(f"{len(lens)} lengths for a batch of {B}")
            if grad:  # the gradient reads the table on the device, after this call has returned
                n_valid = torch.tensor([min(max(v, 0), T) * D for v in lens], dtype=torch.int64).to(x.device)
            lens = _native.i32_array(lens)
        per = torch.empty(B, dtype=torch.float64, device=x.device)
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        total, count, value = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
        _native.check(lib.tts_loss_masked(h, self.KIND, ctypes.c_void_p(x.data_ptr()), xp,
                                          ctypes.c_void_p(y.data_ptr()), yp, lens, B, T, D,
                                          ctypes.c_void_p(per.data_ptr()), ctypes.c_void_p(loss.data_ptr()),
                                          ctypes.byref(total), ctypes.byref(count), ctypes.byref(value),
                                          _native.stream_handle()), "tts_loss_masked")
        self.last_value, self.last_count, self.last_sum = value.value, count.value, total.value
        self.last_per_sentence = per
        return loss, (x, xp, y, yp, n_valid, B, T * D, count.value)


class _Masked(_Elementwise):
    def __call__(self, input, target, length):
        """input, target: [B, T, D]; length: LongTensor or list [B]."""
        return self._run(input, target, length)


class _Unmasked(_Elementwise):
    def __call__(self, input, target):
        return self._run(input, target, None)


class L1LossMasked(_Masked):  # layers/losses.py:7-33
    KIND = _native.TTS_LOSS_L1


class MSELossMasked(_Masked):  # layers/losses.py:36-62
    KIND = _native.TTS_LOSS_MSE


class L1Loss(_Unmasked):  # nn.L1Loss(), train.py:464
    KIND = _native.TTS_LOSS_L1


class MSELoss(_Unmasked):  # nn.MSELoss(), train.py:464
    KIND = _native.TTS_LOSS_MSE


class BCEWithLogitsLoss(_Loss):  # nn.BCEWithLogitsLoss(), train.py:465
    KIND = _native.TTS_LOSS_BCE

    def __call__(self, input, target):
        return self._run(input, target)

    def _forward(self, input, target, length=None, grad=False):
        lib, h = self._handle()
        x, y = _operand(input).contiguous(), _operand(target).contiguous()
        if x.shape != y.shape:
            raise ValueError(f"input {tuple(x.shape)} and target {tuple(y.shape)} differ in shape")
        per = torch.empty(1, dtype=torch.float64, device=x.device)
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        total, value = ctypes.c_double(), ctypes.c_double()
        _native.check(lib.tts_loss_bce_logits(h, ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr()),
                                              x.numel(), ctypes.c_void_p(per.data_ptr()),
                                              ctypes.c_void_p(loss.data_ptr()), ctypes.byref(total),
                                              ctypes.byref(value), _native.stream_handle()), "tts_loss_bce_logits")
        self.last_value, self.last_count, self.last_sum = value.value, x.numel(), total.value
        self.last_per_sentence = per
        # the gradient's grid is per leading row ([B, steps] stop logits: a workgroup per sentence, not n / 8192 in all)
        rows = x.shape[0] if x.dim() > 1 else 1
        return loss, (x, x.numel() // rows, y, x.numel() // rows, None, rows, x.numel() // rows, x.numel())
