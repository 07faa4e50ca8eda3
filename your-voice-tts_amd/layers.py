"""Trainable layers on the device.  ``LSTM`` is a drop-in for the encoder's ``nn.LSTM(512, 256, num_layers=1,
batch_first=True, bidirectional=True)`` (layers/tacotron2.py:56-61) in the three forms the reference calls it:

* ``Encoder.forward`` (:64-76): a ``PackedSequence`` in, ``(PackedSequence, (h_n, c_n))`` out; the pack / unpack
  glue stays torch, the recurrence, its backward through time and the weight gradients are ``tts_lstm_forward`` /
  ``tts_lstm_backward`` (csrc/lstm_train.hip);
* ``Encoder.inference`` (:78-83): a padded ``[B, T, I]`` tensor, every sentence at full length;
* ``Encoder.inference_truncated`` (:85-93): the same with the ``(h_0, c_0)`` of the previous call.

Parameter names, shapes and initialisation are ``nn.LSTM``'s, so state dicts load both ways.  All arithmetic is
fp32 on fixed summation orders: the same operands give the same bits, forward and backward.  Rows at and beyond
a sentence's length are neither read (``x``, the upstream gradient) nor left undefined (``out``, ``grad_x``: +0.0).
``h_n`` and ``c_n`` are not differentiable and ``hx`` is a constant: an ``hx`` that requires grad raises.

With grad mode off, in ``eval()`` mode (where the output does not join autograd; torch's device LSTM refuses a
backward there too), or when neither the input nor a parameter requires grad, the forward keeps nothing for a
backward (``last_reserve_floats`` is 0) and ``out`` has the same bits.  The weights are repacked for the kernels
when the parameters' version counters or addresses have changed since the last call (``repacks`` counts), which
covers ``optimizer.step()``, ``load_state_dict`` and ``.to()``.

Without a GPU a call raises the package's "no GPU" RuntimeError; there is no CPU fallback.

``ConvBNBlock`` is the reference's conv-BN block (layers/tacotron2.py:9-27) with the same ``net`` Sequential, hence
the same state dict, and ``tts_convbn_forward`` / ``tts_convbn_backward`` (csrc/convbn_train.hip) as its forward and
backward; ``use_device_convs(model)`` swaps it into ``encoder.convolutions`` and ``postnet.convolutions``.

``GRU`` is the single-layer ``nn.GRU`` of the Tacotron / TacotronGST family (the CBHG's bidirectional one,
layers/tacotron.py:165-170, and the GST reference encoder's, layers/gst_layers.py:53-56) with ``tts_gru_forward`` /
``tts_gru_backward`` (csrc/gru_train.hip) as its forward and backward, ``out`` and ``h_n`` both differentiable;
``use_device_gru(model)`` swaps it in wherever the model has one it implements.
"""
from __future__ import annotations

import ctypes
import math

import torch
from torch import nn
from torch.autograd.function import once_differentiable
from torch.nn.utils.rnn import PackedSequence, pack_padded_sequence, pad_packed_sequence

from . import _native

_NAMES = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _ptr_pair(ts):
    """[2] of device pointers (None -> NULL), or NULL when every entry is None."""
    if all(t is None for t in ts):
        return None
    arr = (ctypes.c_void_p * 2)()
    for i, t in enumerate(ts):
        arr[i] = t.data_ptr() if t is not None else None
    return arr


def _aligned(t):
    """t contiguous and 16-byte aligned (a copy where it is not)."""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


class _LSTMFunction(torch.autograd.Function):
    """forward(x [B, T, I], module, lens (host ints), h0, c0, *parameters) -> (out, h_n, c_n).  The parameters ride
    along so that autograd asks for their gradients; the kernels read the module's repacked copies."""

    @staticmethod
    def forward(ctx, x, module, lens, h0, c0, *params):
        out, h_n, c_n, reserve = module._run_forward(x, lens, h0, c0, True)
        ctx.save_for_backward(x, out, reserve, *([] if h0 is None else [h0]))
        ctx.module, ctx.lens, ctx.has_h0 = module, lens, h0 is not None
        ctx.versions = module._key()
        ctx.mark_non_differentiable(h_n, c_n)
        return out, h_n, c_n

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out, _grad_h, _grad_c):
        x, out, reserve, *h0 = ctx.saved_tensors
        m = ctx.module
        if m._key() != ctx.versions:
            raise RuntimeError("layers.LSTM: the parameters were modified between this forward and its backward")
        need = ctx.needs_input_grad
        grads = m._run_backward(x, ctx.lens, reserve, out, h0[0] if ctx.has_h0 else None, grad_out, need[0], need[5:])
        return (grads[0], None, None, None, None) + tuple(grads[1:])


class LSTM(nn.Module):
    """``nn.LSTM(input_size, hidden_size, num_layers=1, bias=True, batch_first=True, bidirectional=...)`` on the
    device.  ``last_reserve_floats``: the size of the reserve the last forward kept (0: none); ``repacks``: how
    often the weights were repacked."""

    def __init__(self, input_size, hidden_size, num_layers=1, bias=True, batch_first=False, dropout=0.0,
                 bidirectional=False, proj_size=0, device=None, dtype=None):
        super().__init__()
        for ok, what in ((num_layers == 1, "num_layers != 1"), (bias, "bias=False"),
                         (batch_first, "batch_first=False"), (dropout == 0, "dropout"), (proj_size == 0, "proj_size"),
                         (dtype in (None, torch.float32), "a dtype other than float32"),
                         (input_size > 0 and input_size % 16 == 0, "an input_size that is no multiple of 16"),
                         (hidden_size > 0 and hidden_size % 16 == 0, "a hidden_size that is no multiple of 16")):
            if not ok:
                raise NotImplementedError(f"layers.LSTM does not implement {what}")
        self.input_size, self.hidden_size, self.bidirectional = input_size, hidden_size, bool(bidirectional)
        self.num_layers, self.bias, self.batch_first, self.dropout, self.proj_size = 1, True, True, 0.0, 0
        G = 4 * hidden_size
        for suffix in ("", "_reverse")[:self.num_directions]:
            for name, shape in zip(_NAMES, ((G, input_size), (G, hidden_size), (G,), (G,))):
                self.register_parameter(name + suffix, nn.Parameter(torch.empty(shape, device=device)))
        self.reset_parameters()
        self._h = None
        self._packed_key = None
        self.repacks = 0
        self.last_reserve_floats = 0

    @property
    def num_directions(self):
        return 2 if self.bidirectional else 1

    def reset_parameters(self):  # nn.LSTM's: U(-1 / sqrt(H), 1 / sqrt(H)) on every parameter
        k = 1.0 / math.sqrt(self.hidden_size)
        for p in self.parameters():
            nn.init.uniform_(p, -k, k)

    def flatten_parameters(self):  # (layers/tacotron2.py:70: nothing to flatten here)
        pass

    def extra_repr(self):
        return f"{self.input_size}, {self.hidden_size}, batch_first=True, bidirectional={self.bidirectional}"

    def __del__(self):
        try:
            if self._h is not None:
                self._h[0].tts_lstm_destroy(self._h[1])
        except Exception:
            pass

    # ------------------------------------------------------------------ the handle and its weights
    def _params(self):
        return [getattr(self, n + s) for s in ("", "_reverse")[:self.num_directions] for n in _NAMES]

    def _key(self):
        return tuple((p.data_ptr(), p._version) for p in self._params())

    def _handle(self):
        lib = _native.lib()  # raises without a GPU / library: no CPU fallback
        if self._h is None:
            h = ctypes.c_void_p()
            _native.check(lib.tts_lstm_create(self.input_size, self.hidden_size, int(self.bidirectional),
                                              ctypes.byref(h)), "tts_lstm_create")
            self._h = (lib, h)
        return self._h

    def _sync_weights(self):
        lib, h = self._handle()
        key = self._key()
        if key == self._packed_key:
            return
        ps = self._params()
        for p in ps:
            if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous() or p.data_ptr() % 16:
                raise ValueError("layers.LSTM: parameters must be contiguous 16-byte aligned CUDA float32 tensors")
        per = [_ptr_pair([ps[d * 4 + k] for d in range(self.num_directions)] + [None] * (2 - self.num_directions))
               for k in range(4)]
        _native.check(lib.tts_lstm_set_weights(h, *per, _native.stream_handle()), "tts_lstm_set_weights")
        self._packed_key = key
        self.repacks += 1

    # ------------------------------------------------------------------ the two calls
    def _run_forward(self, x, lens, h0, c0, want_reserve):
        lib, h = self._handle()
        self._sync_weights()
        B, T, _ = x.shape
        D, H = self.num_directions, self.hidden_size
        x = _aligned(x.detach())
        out = torch.empty(B, T, D * H, dtype=torch.float32, device=x.device)
        h_n = torch.empty(D, B, H, dtype=torch.float32, device=x.device)
        c_n = torch.empty_like(h_n)
        reserve = None
        if want_reserve:
            reserve = torch.empty(lib.tts_lstm_reserve_floats(h, B, T), dtype=torch.float32, device=x.device)
        self.last_reserve_floats = 0 if reserve is None else reserve.numel()
        _native.check(lib.tts_lstm_forward(h, _ptr(x), _native.i32_array(lens), B, T, _ptr(h0), _ptr(c0), _ptr(out),
                                           _ptr(h_n), _ptr(c_n), _ptr(reserve), _native.stream_handle()),
                      "tts_lstm_forward")
        return out, h_n, c_n, reserve

    def _run_backward(self, x, lens, reserve, out, h0, grad_out, need_x, need_params):
        lib, h = self._handle()
        B, T, _ = x.shape
        D = self.num_directions
        x = _aligned(x.detach())
        grad_out = _aligned(grad_out)
        grad_x = torch.empty_like(x) if need_x else None
        ps = self._params()
        gp = [torch.empty_like(p) if need else None for p, need in zip(ps, need_params)]
        per = [_ptr_pair([gp[d * 4 + k] for d in range(D)] + [None] * (2 - D)) for k in range(4)]
        _native.check(lib.tts_lstm_backward(h, _ptr(x), _native.i32_array(lens), B, T, _ptr(reserve), _ptr(out),
                                            _ptr(h0), _ptr(grad_out), _ptr(grad_x), *per, _native.stream_handle()),
                      "tts_lstm_backward")
        return [grad_x] + gp

    def _call(self, x, lens, hx):
        if x.dim() != 3 or x.shape[2] != self.input_size:
            raise ValueError(f"expected input [B, T, {self.input_size}], got {tuple(x.shape)}")
        if not x.is_cuda:
            _native.lib()  # the "no GPU" error where there is none
            raise RuntimeError("layers.LSTM: the input must be a CUDA tensor (there is no CPU path)")
        if x.dtype != torch.float32:
            raise ValueError(f"layers.LSTM: the input must be float32, got {x.dtype}")
        B, T, _ = x.shape
        lens = [int(v) for v in lens]
        if len(lens) != B or min(lens) < 1 or max(lens) > T:
            raise ValueError(f"lengths {lens} do not fit a batch of {B} with {T} positions")
        h0 = c0 = None
        if hx is not None:
            h0, c0 = hx
            if h0.requires_grad or c0.requires_grad:
                raise NotImplementedError("layers.LSTM: hx is a constant; gradients with respect to it are not "
                                          "implemented")
            shape = (self.num_directions, B, self.hidden_size)
            if tuple(h0.shape) != shape or tuple(c0.shape) != shape:
                raise ValueError(f"expected hx of two {shape} tensors, got {tuple(h0.shape)}, {tuple(c0.shape)}")
            h0, c0 = (_aligned(t.detach().to(x.device, torch.float32)) for t in (h0, c0))
        params = self._params()
        if not (self.training and torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params))):
            return self._run_forward(x, lens, h0, c0, False)[:3]
        return _LSTMFunction.apply(x, self, lens, h0, c0, *params)

    def forward(self, input, hx=None):
        if isinstance(input, PackedSequence):
            # padded in the caller's order, which is also the order of hx and of the states nn.LSTM returns
            x, lengths = pad_packed_sequence(input, batch_first=True)
            out, h_n, c_n = self._call(x, lengths.tolist(), hx)
            packed = pack_padded_sequence(out, lengths, batch_first=True, enforce_sorted=input.sorted_indices is None)
            return packed, (h_n, c_n)
        out, h_n, c_n = self._call(input, [input.shape[1]] * input.shape[0], hx)
        return out, (h_n, c_n)


    def lstm(self, x, lengths, hx=None):
        """The functional form on padded input: ``x [B, T, I]`` with ``lengths`` in any order -> ``(out [B, T, D * H]``
        with +0.0 past each length, ``(h_n, c_n))``; no packing on either side."""
        out, h_n, c_n = self._call(x, torch.as_tensor(lengths).reshape(-1).tolist(), hx)
        return out, (h_n, c_n)


def lstm(x, lengths, module, hx=None):
    """``module.lstm(x, lengths, hx)`` for a ``layers.LSTM`` module."""
    return module.lstm(x, lengths, hx)


def use_device_lstm(model):
    """Swap ``model.encoder.lstm`` (the reference's ``nn.LSTM``, layers/tacotron2.py:56-61) for a ``layers.LSTM``
    that carries the same weights on the same device; returns the model.  Build the optimizer afterwards: the
    parameters are new tensors."""
    old = model.encoder.lstm
    if isinstance(old, LSTM):
        return model
    new = LSTM(old.input_size, old.hidden_size, num_layers=old.num_layers, bias=old.bias,
               batch_first=old.batch_first, dropout=old.dropout, bidirectional=old.bidirectional,
               proj_size=getattr(old, "proj_size", 0))
    new.load_state_dict(old.state_dict())
    p = next(old.parameters())
    new.to(p.device)
    new.train(old.training)
    model.encoder.lstm = new
    return model


# ---------------------------------------------------------------------- the conv-BN block
_ACTS = {None: 0, "relu": 1, "tanh": 2}


class _ConvBNFunction(torch.autograd.Function):
    """forward(x [B, Cin, T], module, mask, *parameters) -> out.  The parameters ride along so that autograd asks for
    their gradients; the kernels read the module's repacked copies."""

    @staticmethod
    def forward(ctx, x, module, mask, *params):
        out, reserve = module._run_forward(x, mask, True)
        ctx.save_for_backward(x, reserve, mask)
        ctx.module = module
        ctx.versions = module._key()
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        x, reserve, mask = ctx.saved_tensors
        m = ctx.module
        if m._key() != ctx.versions:
            raise RuntimeError("layers.ConvBNBlock: the parameters were modified between this forward and its backward")
        need = ctx.needs_input_grad
        grads = m._run_backward(x, reserve, mask, grad_out, need[0], need[3:])
        return (grads[0], None, None) + tuple(grads[1:])


class ConvBNBlock(nn.Module):
    """The reference's ``ConvBNBlock`` (layers/tacotron2.py:9-27) on the device: ``self.net`` is built exactly as
    there (``nn.Sequential(Conv1d(k=5, padding=2), BatchNorm1d, [ReLU | Tanh], Dropout(0.5))``), so parameter and
    buffer names, shapes and initialisation are the reference's and state dicts load both ways; only ``forward``
    is replaced, by ``tts_convbn_forward`` / ``tts_convbn_backward`` (csrc/convbn_train.hip).

    ``forward(x, mask=None)``: ``x`` is ``[B, Cin, T]`` float32 on the device, any strided view (copied once where
    it is not contiguous; same bits).  ``mask`` (uint8 or bool ``[B, Cout, T]``, 1 = keep) fixes the dropout mask;
    without it the mask is drawn on the device from torch's generator (``torch.manual_seed`` governs it).
    ``last_mask`` is the mask that was used (None in ``eval()``), the scale is ``1 / (1 - net[-1].p)``.  In training
    mode the batch statistics normalise and the kernel updates ``running_mean`` / ``running_var`` in place
    (``num_batches_tracked += 1``); in ``eval()`` the running statistics normalise, there is no dropout and ``mask``
    is ignored.  With grad mode off, or when nothing requires grad, no reserve is kept (``last_reserve_floats``
    is 0) and the output has the same bits.  The weights are repacked when the parameters' version counters or
    addresses have changed (``repacks`` counts).  Without a GPU a call raises the package's "no GPU" RuntimeError;
    there is no CPU path."""

    def __init__(self, in_channels, out_channels, kernel_size, nonlinear=None):
        super().__init__()
        for ok, what in ((kernel_size == 5, "a kernel_size other than 5"),
                         (nonlinear in _ACTS, f"nonlinear={nonlinear!r}"),
                         (in_channels > 0 and in_channels % 16 == 0, "in_channels that are no multiple of 16"),
                         (out_channels > 0 and out_channels % 16 == 0, "out_channels that are no multiple of 16")):
            if not ok:
                raise NotImplementedError(f"layers.ConvBNBlock does not implement {what}")
        padding = (kernel_size - 1) // 2
        conv1d = nn.Conv1d(in_channels, out_channels, kernel_size, padding=padding)
        norm = nn.BatchNorm1d(out_channels)
        dropout = nn.Dropout(p=0.5)
        if nonlinear == "relu":
            self.net = nn.Sequential(conv1d, norm, nn.ReLU(), dropout)
        elif nonlinear == "tanh":
            self.net = nn.Sequential(conv1d, norm, nn.Tanh(), dropout)
        else:
            self.net = nn.Sequential(conv1d, norm, dropout)
        self.in_channels, self.out_channels, self.kernel_size, self.nonlinear = in_channels, out_channels, 5, nonlinear
        self._h = None
        self._packed_key = None
        self.repacks = 0
        self.last_reserve_floats = 0
        self.last_mask = None

    def __del__(self):
        try:
            if self._h is not None:
                self._h[0].tts_convbn_destroy(self._h[1])
        except Exception:
            pass

    # ------------------------------------------------------------------ the handle and its weights
    def _params(self):
        conv, norm = self.net[0], self.net[1]
        return [conv.weight, conv.bias, norm.weight, norm.bias]

    def _key(self):
        return tuple((p.data_ptr(), p._version) for p in self._params())

    def _handle(self):
        lib = _native.lib()  # raises without a GPU / library: no CPU fallback
        if self._h is None:
            h = ctypes.c_void_p()
            _native.check(lib.tts_convbn_create(self.in_channels, self.out_channels, self.kernel_size,
                                                _ACTS[self.nonlinear], ctypes.byref(h)), "tts_convbn_create")
            self._h = (lib, h)
        return self._h

    def _sync_weights(self):
        lib, h = self._handle()
        key = self._key()
        if key == self._packed_key:
            return
        ps = self._params()
        for p in ps:
            if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                raise ValueError("layers.ConvBNBlock: parameters must be contiguous CUDA float32 tensors")
        _native.check(lib.tts_convbn_set_weights(h, *[_ptr(p) for p in ps], _native.stream_handle()),
                      "tts_convbn_set_weights")
        self._packed_key = key
        self.repacks += 1

    # ------------------------------------------------------------------ the two calls
    def _run_forward(self, x, mask, want_reserve):
        lib, h = self._handle()
        self._sync_weights()
        norm, drop = self.net[1], self.net[-1]
        for buf in (norm.running_mean, norm.running_var):
            if not buf.is_cuda or buf.dtype != torch.float32 or not buf.is_contiguous():
                raise ValueError("layers.ConvBNBlock: the running buffers must be contiguous CUDA float32 tensors")
        B, _, T = x.shape
        x = x.detach().contiguous()
        out = torch.empty(B, self.out_channels, T, dtype=torch.float32, device=x.device)
        reserve = None
        if want_reserve and self.training:
            reserve = torch.empty(lib.tts_convbn_reserve_floats(h, B, T), dtype=torch.float32, device=x.device)
        self.last_reserve_floats = 0 if reserve is None else reserve.numel()
        _native.check(lib.tts_convbn_forward(h, _ptr(x), B, T, _ptr(mask), 1.0 / (1.0 - drop.p),
                                             _ptr(norm.running_mean), _ptr(norm.running_var), float(norm.momentum),
                                             float(norm.eps), int(self.training), _ptr(out), _ptr(reserve),
                                             _native.stream_handle()), "tts_convbn_forward")
        if self.training:
            norm.num_batches_tracked += 1
        return out, reserve

    def _run_backward(self, x, reserve, mask, grad_out, need_x, need_params):
        lib, h = self._handle()
        B, _, T = x.shape
        x = x.detach().contiguous()
        grad_out = grad_out.contiguous()
        grad_x = torch.empty_like(x) if need_x else None
        gp = [torch.empty_like(p) if need else None for p, need in zip(self._params(), need_params)]
        _native.check(lib.tts_convbn_backward(h, _ptr(x), B, T, _ptr(reserve), _ptr(mask), _ptr(grad_out), _ptr(grad_x),
                                              *[_ptr(g) for g in gp], _native.stream_handle()), "tts_convbn_backward")
        return [grad_x] + gp

    def forward(self, x, mask=None):
        norm, drop = self.net[1], self.net[-1]
        if norm.momentum is None or not norm.track_running_stats:
            raise NotImplementedError("layers.ConvBNBlock implements neither momentum=None nor "
                                      "track_running_stats=False")
        if x.dim() != 3 or x.shape[1] != self.in_channels:
            raise ValueError(f"expected input [B, {self.in_channels}, T], got {tuple(x.shape)}")
        if not x.is_cuda:
            _native.lib()  # the "no GPU" error where there is none
            raise RuntimeError("layers.ConvBNBlock: the input must be a CUDA tensor (there is no CPU path)")
        if x.dtype != torch.float32:
            raise ValueError(f"layers.ConvBNBlock: the input must be float32, got {x.dtype}")
        B, _, T = x.shape
        if B < 1 or T < 1:
            raise ValueError(f"layers.ConvBNBlock: an empty input {tuple(x.shape)}")
        shape = (B, self.out_channels, T)
        if not self.training:
            self.last_mask = None
            return self._run_forward(x, None, False)[0]
        if B * T == 1:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x.shape)}")
        if not 0.0 <= drop.p < 1.0:
            raise NotImplementedError("layers.ConvBNBlock needs a dropout probability in [0, 1)")
        if mask is None:
            mask = (torch.rand(shape, device=x.device) >= drop.p).to(torch.uint8)
        else:
            if tuple(mask.shape) != shape or mask.dtype not in (torch.uint8, torch.bool):
                raise ValueError(f"expected a uint8 or bool mask of shape {shape}, got {mask.dtype} {tuple(mask.shape)}")
            mask = mask.to(x.device, torch.uint8).contiguous()
        self.last_mask = mask
        params = self._params()
        if not (torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params))):
            return self._run_forward(x, mask, False)[0]
        return _ConvBNFunction.apply(x, self, mask, *params)


def _conv_block_shape(block):
    """(conv, norm, nonlinear, dropout) when ``block.net`` is the reference's Sequential of Conv1d, BatchNorm1d,
    [ReLU | Tanh], Dropout; else None."""
    net = getattr(block, "net", None)
    if not isinstance(net, nn.Sequential) or len(net) not in (3, 4):
        return None
    if not (isinstance(net[0], nn.Conv1d) and isinstance(net[1], nn.BatchNorm1d) and isinstance(net[-1], nn.Dropout)):
        return None
    nonlinear = None
    if len(net) == 4:
        nonlinear = "relu" if isinstance(net[2], nn.ReLU) else "tanh" if isinstance(net[2], nn.Tanh) else False
        if nonlinear is False:
            return None
    return net[0], net[1], nonlinear, net[-1]


def use_device_convs(model):
    """Swap every conv-BN block of ``model.encoder.convolutions`` and ``model.postnet.convolutions`` (whichever
    exist; layers/tacotron2.py:52-55, :30-45) for a ``layers.ConvBNBlock`` that carries the same parameters and
    buffers on the same device in the same training mode; returns the model.  A block is recognised by its
    structure (a ``.net`` Sequential of Conv1d, BatchNorm1d, [ReLU | Tanh], Dropout).  Calling it again changes
    nothing.  Build the optimizer afterwards: the parameters are new tensors.  Measured against torch's own
    blocks on an MI355X: profiles/convbn_train.json ("timing")."""
    for part in ("encoder", "postnet"):
        convs = getattr(getattr(model, part, None), "convolutions", None)
        if convs is None:
            continue
        for i, old in enumerate(convs):
            found = None if isinstance(old, ConvBNBlock) else _conv_block_shape(old)
            if found is None:
                continue
            conv, norm, nonlinear, drop = found
            new = ConvBNBlock(conv.in_channels, conv.out_channels, conv.kernel_size[0], nonlinear)
            new.load_state_dict(old.state_dict())
            new.net[1].eps, new.net[1].momentum = norm.eps, norm.momentum
            new.net[-1].p = drop.p
            new.to(conv.weight.device)
            new.train(old.training)
            convs[i] = new
    return model


# ---------------------------------------------------------------------- the decoder
_P_PRENET, _NORMS = 0.5, {"sigmoid": 0, "softmax": 1}
_MASK_GROUPS = ("prenet", "att", "dec", "stop")


class _Linear(nn.Module):
    """The reference's ``Linear`` (layers/common_layers.py:8-25): ``linear_layer`` with Xavier-uniform weights."""

    def __init__(self, in_features, out_features, bias=True, init_gain="linear"):
        super().__init__()
        self.linear_layer = nn.Linear(in_features, out_features, bias=bias)
        nn.init.xavier_uniform_(self.linear_layer.weight, gain=nn.init.calculate_gain(init_gain))

    def forward(self, x):
        return self.linear_layer(x)


def _decoder_unsupported(prenet_type, trans_agent, location_attn):
    for bad, what in ((location_attn, "location_attn"), (trans_agent, "trans_agent"),
                      (prenet_type != "original", f"prenet_type={prenet_type!r}")):
        if bad:
            raise NotImplementedError(f"layers.Decoder does not implement {what}")


class _DecoderFunction(torch.autograd.Function):
    """forward(inputs, memories, module, mask, masks, *parameters) -> (out [B, T, MR], stop, alignments, reserve).
    ``alignments`` is not differentiable.  With a separate stopnet ``stop`` is not differentiable here either: the
    stop tokens join autograd through ``_StopFunction``, a node of its own, so a second backward through them works
    after this one; otherwise their gradient arrives here together with that of ``out``."""

    @staticmethod
    def forward(ctx, inputs, memories, module, mask, masks, *params):
        out, stop, align, reserve = module._run_forward(inputs, memories, mask, masks, True)
        ctx.save_for_backward(reserve, mask, *[masks[k] for k in _MASK_GROUPS])
        ctx.module, ctx.shape = module, (inputs.shape[0], inputs.shape[1], stop.shape[1])
        ctx.versions = module._key()
        if module.separate_stopnet:
            ctx.mark_non_differentiable(stop, align, reserve)
        else:
            ctx.mark_non_differentiable(align, reserve)
        return out, stop, align, reserve

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out, grad_stop, _ga, _gr):
        reserve, mask, *mk = ctx.saved_tensors
        m = ctx.module
        if m._key() != ctx.versions:
            raise RuntimeError("layers.Decoder: the parameters were modified between this forward and its backward")
        need, need_params = ctx.needs_input_grad, list(ctx.needs_input_grad[5:])
        if m.separate_stopnet:  # the stopnet's weight and bias (positions 16, 17) belong to _StopFunction
            grad_stop = None
            need_params[16] = need_params[17] = False
        grads = m._run_backward(ctx.shape, mask, dict(zip(_MASK_GROUPS, mk)), reserve, grad_out, grad_stop, need[0],
                                need[1], need_params)
        return (grads[0], grads[1], None, None, None) + tuple(grads[2:])


class _StopFunction(torch.autograd.Function):
    """forward(stop_raw, module, mask, masks, reserve, shape, *parameters) -> the stop tokens of a separate stopnet:
    only its own weight and bias receive gradients (its input is detached), without a walk back through time."""

    @staticmethod
    def forward(ctx, stop_raw, module, mask, masks, reserve, shape, *params):
        ctx.save_for_backward(reserve, mask, *[masks[k] for k in _MASK_GROUPS])
        ctx.module, ctx.shape = module, shape
        return stop_raw.clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_stop):
        reserve, mask, *mk = ctx.saved_tensors
        m = ctx.module
        # (no stale-parameter check: these two gradients read the reserve alone, so train_batch may step the main
        #  optimizer between the two backwards, as the reference does)
        need = [n and i in (16, 17) for i, n in enumerate(ctx.needs_input_grad[6:])]
        grads = m._run_backward(ctx.shape, mask, dict(zip(_MASK_GROUPS, mk)), reserve, None, grad_stop, False, False, need)
        return (None,) * 6 + tuple(grads[2:])


class Decoder(nn.Module):
    """The reference's ``Decoder`` (layers/tacotron2.py:97-247) with its teacher-forced ``forward`` and the whole
    backward through time on the device (``tts_dectrain_forward`` / ``tts_dectrain_backward``,
    csrc/decoder_train.hip).  The submodules are built under the reference's names, so ``state_dict()`` keys,
    shapes and initialisation are the reference's and state dicts load both ways.

    ``forward(inputs [B, L, in_features], memories [B, T * r, mel], mask [B, L] or None, masks=None)`` returns the
    reference's ``(outputs [B, mel, T * r], stop_tokens [B, T], alignments [B, T, L])``; ``alignments`` is for logging
    and not differentiable.  ``masks`` fixes the dropout masks: a dict of the four groups, uint8 with 1 = keep,
    ``prenet [2, T, B, prenet]`` (p = 0.5; absent or ignored without ``prenet_dropout``), ``att [2, T, B, rnn]`` (h, c
    of the attention LSTM, p = 0.1), ``dec [2, T, B, rnn]``, ``stop [T, B, rnn + mel * r]`` (p = ``stopnet[0].p``); without
    it they are drawn on the device from torch's generator.  ``last_masks`` holds what was used (None in ``eval()``).
    A masked row of ``inputs`` never reaches a product; ``grad_inputs`` is +0.0 there.

    ``location_attn``, ``trans_agent`` and ``prenet_type="bn"`` raise ``NotImplementedError``.  ``attn_win`` and
    ``forward_attn_mask`` act only in ``eval()``: accepted and ignored in ``train()``; an ``eval()`` forward with either
    set raises.  ``inference*`` are not part of this module: use the package's ``Tacotron2.inference``.

    With grad mode off, or when nothing requires grad, no reserve is kept (``last_reserve_floats`` is 0) and the
    outputs have the same bits.  In ``eval()`` the forward runs without dropout and its outputs do NOT join autograd,
    even with grad mode on (unlike the reference's ``Decoder``, whose ``eval()`` forward is differentiable): the backward
    exists for training forwards only, as for ``layers.LSTM``.  The weights are repacked when the parameters' version counters or addresses have
    changed (``repacks`` counts).  Without a GPU a call raises the package's "no GPU" RuntimeError; there is no CPU
    path."""

    def __init__(self, in_features, inputs_dim, r, attn_win, attn_norm, prenet_type, prenet_dropout, forward_attn,
                 trans_agent, forward_attn_mask, location_attn, separate_stopnet, prenet_dim=256, rnn_dim=1024,
                 attention_dim=128):
        super().__init__()
        _decoder_unsupported(prenet_type, trans_agent, location_attn)
        if attn_norm not in _NORMS:
            raise RuntimeError("Unknown value for attention norm type")
        for v, what in ((in_features, "in_features"), (prenet_dim, "prenet_dim"), (rnn_dim, "rnn_dim"),
                        (attention_dim, "attention_dim")):
            if v <= 0 or v % 16:
                raise NotImplementedError(f"layers.Decoder does not implement a {what} that is no multiple of 16")
        self.mel_channels, self.r, self.encoder_embedding_dim = inputs_dim, r, in_features
        self.separate_stopnet = separate_stopnet
        self.attention_rnn_dim = self.decoder_rnn_dim = rnn_dim
        self.prenet_dim, self.attention_dim = prenet_dim, attention_dim
        self.max_decoder_steps, self.gate_threshold = 1000, 0.5
        self.p_attention_dropout = self.p_decoder_dropout = 0.1
        MR = inputs_dim * r
        self.prenet = nn.Module()
        self.prenet.prenet_type, self.prenet.prenet_dropout = prenet_type, prenet_dropout
        self.prenet.layers = nn.ModuleList([_Linear(MR, prenet_dim, bias=False), _Linear(prenet_dim, prenet_dim, bias=False)])
        self.attention_rnn = nn.LSTMCell(prenet_dim + in_features, rnn_dim)
        att = nn.Module()
        att.query_layer = _Linear(rnn_dim, attention_dim, bias=False, init_gain="tanh")
        att.inputs_layer = _Linear(in_features, attention_dim, bias=False, init_gain="tanh")
        att.v = _Linear(attention_dim, 1, bias=True)
        att.windowing, att.norm, att.forward_attn, att.trans_agent = attn_win, attn_norm, forward_attn, trans_agent
        att.forward_attn_mask, att.location_attention = forward_attn_mask, location_attn
        self.attention_layer = att
        self.decoder_rnn = nn.LSTMCell(rnn_dim + in_features, rnn_dim, 1)
        self.linear_projection = _Linear(rnn_dim + in_features, MR)
        self.stopnet = nn.Sequential(nn.Dropout(0.1), _Linear(rnn_dim + MR, 1, bias=True, init_gain="sigmoid"))
        self.attention_rnn_init = nn.Embedding(1, rnn_dim)
        self.go_frame_init = nn.Embedding(1, MR)
        self.decoder_rnn_inits = nn.Embedding(1, rnn_dim)
        self.memory_truncated = None
        self._h = None
        self._packed_key = None
        self.repacks = 0
        self.last_reserve_floats = 0
        self.last_masks = None

    def __del__(self):
        try:
            if self._h is not None:
                self._h[0].tts_dectrain_destroy(self._h[1])
        except Exception:
            pass

    def inference(self, *args, **kwargs):
        raise NotImplementedError("layers.Decoder trains; synthesis is the package's Tacotron2.inference")

    inference_truncated = inference_step = inference

    # ------------------------------------------------------------------ the handle and its weights
    def _params(self):
        named = dict(self.named_parameters())
        return [named[n] for n in _native.DECTRAIN_PARAMS]

    def _key(self):
        return tuple((p.data_ptr(), p._version) for p in self._params())

    def _handle(self):
        lib = _native.lib()  # raises without a GPU / library: no CPU fallback
        if self._h is None:
            h = ctypes.c_void_p()
            a = self.attention_layer
            _native.check(lib.tts_dectrain_create(self.encoder_embedding_dim, self.prenet_dim, self.attention_rnn_dim,
                                                  self.attention_dim, self.mel_channels * self.r, _NORMS[a.norm],
                                                  int(bool(a.forward_attn)), int(bool(self.prenet.prenet_dropout)),
                                                  int(bool(self.separate_stopnet)), ctypes.byref(h)),
                          "tts_dectrain_create")
            self._h = (lib, h)
        return self._h

    def _sync_weights(self):
        lib, h = self._handle()
        key = self._key()
        if key == self._packed_key:
            return
        ps = self._params()
        for p in ps:
            if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                raise ValueError("layers.Decoder: parameters must be contiguous CUDA float32 tensors")
        table = _native.DectrainTensors(*[p.data_ptr() for p in ps])
        _native.check(lib.tts_dectrain_set_weights(h, ctypes.byref(table), _native.stream_handle()),
                      "tts_dectrain_set_weights")
        self._packed_key = key
        self.repacks += 1

    def _mask_table(self, masks):
        if masks is None:
            return None
        pn = masks.get("prenet") if self.prenet.prenet_dropout else None
        ptr = lambda t: t.data_ptr()
        return _native.DectrainMasks(ptr(pn[0]) if pn is not None else None, ptr(pn[1]) if pn is not None else None,
                                     ptr(masks["att"][0]), ptr(masks["att"][1]), ptr(masks["dec"][0]),
                                     ptr(masks["dec"][1]), ptr(masks["stop"]), 1.0 / (1.0 - _P_PRENET),
                                     1.0 / (1.0 - self.p_attention_dropout), 1.0 / (1.0 - self.stopnet[0].p))

    # ------------------------------------------------------------------ the two calls
    def _run_forward(self, inputs, memories, mask, masks, want_reserve):
        lib, h = self._handle()
        self._sync_weights()
        B, L, _ = inputs.shape
        T, MR = memories.shape[1] // self.r, self.mel_channels * self.r
        inputs, memories = inputs.detach().contiguous(), memories.detach().contiguous()
        dev = inputs.device
        out = torch.empty(B, T, MR, dtype=torch.float32, device=dev)
        stop = torch.empty(B, T, dtype=torch.float32, device=dev)
        align = torch.empty(B, T, L, dtype=torch.float32, device=dev)
        reserve = None
        if want_reserve:
            reserve = torch.empty(lib.tts_dectrain_reserve_floats(h, B, L, T), dtype=torch.float32, device=dev)
        self.last_reserve_floats = 0 if reserve is None else reserve.numel()
        table = self._mask_table(masks)
        _native.check(lib.tts_dectrain_forward(h, _ptr(inputs), _ptr(memories), _ptr(mask), B, L, T,
                                               int(masks is not None), ctypes.byref(table) if table else None,
                                               _ptr(out), _ptr(stop), _ptr(align), _ptr(reserve),
                                               _native.stream_handle()), "tts_dectrain_forward")
        return out, stop, align, reserve

    def _run_backward(self, shape, mask, masks, reserve, grad_out, grad_stop, need_inputs, need_memories, need_params):
        lib, h = self._handle()
        B, L, T = shape
        dev = reserve.device
        grad_out = grad_out.contiguous() if grad_out is not None else None
        grad_stop = grad_stop.contiguous() if grad_stop is not None else None
        g_in = torch.empty(B, L, self.encoder_embedding_dim, dtype=torch.float32, device=dev) if need_inputs else None
        g_mem = torch.empty(B, T * self.r, self.mel_channels, dtype=torch.float32, device=dev) if need_memories else None
        gp = [torch.empty_like(p) if need else None for p, need in zip(self._params(), need_params)]
        table = _native.DectrainTensors(*[g.data_ptr() if g is not None else None for g in gp])
        mt = self._mask_table(masks)
        _native.check(lib.tts_dectrain_backward(h, _ptr(mask), B, L, T, ctypes.byref(mt), _ptr(reserve), _ptr(grad_out),
                                                _ptr(grad_stop), _ptr(g_in), _ptr(g_mem), ctypes.byref(table),
                                                _native.stream_handle()), "tts_dectrain_backward")
        return [g_in, g_mem] + gp

    def _draw_masks(self, B, T, device):
        R, MR = self.attention_rnn_dim, self.mel_channels * self.r
        shapes = dict(prenet=(2, T, B, self.prenet_dim), att=(2, T, B, R), dec=(2, T, B, R), stop=(T, B, R + MR))
        p = dict(prenet=_P_PRENET, att=self.p_attention_dropout, dec=self.p_decoder_dropout, stop=self.stopnet[0].p)
        return {k: (torch.rand(s, device=device) >= p[k]).to(torch.uint8) for k, s in shapes.items()}

    def forward(self, inputs, memories, mask, masks=None):
        a = self.attention_layer
        if not self.training and (a.windowing or a.forward_attn_mask):
            raise NotImplementedError("layers.Decoder implements neither attn_win nor forward_attn_mask in eval(); "
                                      "synthesis is the package's Tacotron2.inference")
        if inputs.dim() != 3 or inputs.shape[2] != self.encoder_embedding_dim:
            raise ValueError(f"expected inputs [B, L, {self.encoder_embedding_dim}], got {tuple(inputs.shape)}")
        if memories.dim() != 3 or memories.shape[0] != inputs.shape[0] or memories.shape[2] != self.mel_channels \
                or memories.shape[1] % self.r or memories.shape[1] < self.r:
            raise ValueError(f"expected memories [B, T * {self.r}, {self.mel_channels}], got {tuple(memories.shape)}")
        if not inputs.is_cuda:
            _native.lib()  # the "no GPU" error where there is none
            raise RuntimeError("layers.Decoder: the inputs must be CUDA tensors (there is no CPU path)")
        if inputs.dtype != torch.float32 or memories.dtype != torch.float32:
            raise ValueError("layers.Decoder: inputs and memories must be float32")
        B, L, _ = inputs.shape
        T = memories.shape[1] // self.r
        if mask is not None:
            if tuple(mask.shape) != (B, L):
                raise ValueError(f"expected a mask of shape {(B, L)}, got {tuple(mask.shape)}")
            mask = (mask != 0).to(inputs.device, torch.uint8).contiguous()
        if self.training:
            if masks is None:
                masks = self._draw_masks(B, T, inputs.device)
            else:
                R, MR = self.attention_rnn_dim, self.mel_channels * self.r
                shapes = dict(prenet=(2, T, B, self.prenet_dim), att=(2, T, B, R), dec=(2, T, B, R), stop=(T, B, R + MR))
                fixed = {}
                for k in _MASK_GROUPS:
                    if k == "prenet" and not self.prenet.prenet_dropout and masks.get(k) is None:
                        fixed[k] = torch.ones(shapes[k], dtype=torch.uint8, device=inputs.device)
                        continue
                    t = masks[k]
                    if tuple(t.shape) != shapes[k] or t.dtype not in (torch.uint8, torch.bool):
                        raise ValueError(f"expected a uint8 or bool mask group {k!r} of shape {shapes[k]}, got "
                                         f"{t.dtype} {tuple(t.shape)}")
                    fixed[k] = t.to(inputs.device, torch.uint8).contiguous()
                masks = fixed
        else:
            masks = None
        self.last_masks = masks
        params = self._params()
        track = self.training and torch.is_grad_enabled() and (
            inputs.requires_grad or memories.requires_grad or any(p.requires_grad for p in params))
        if not track:
            out, stop, align, _ = self._run_forward(inputs, memories, mask, masks, False)
        else:
            out, stop, align, reserve = _DecoderFunction.apply(inputs, memories, self, mask, masks, *params)
            if self.separate_stopnet:
                stop = _StopFunction.apply(stop, self, mask, masks, reserve, (B, L, T), *params)
        return out.view(B, T * self.r, self.mel_channels).transpose(1, 2), stop, align


def _is_reference_decoder(dec):
    need = ("prenet", "attention_rnn", "attention_layer", "decoder_rnn", "linear_projection", "stopnet",
            "attention_rnn_init", "go_frame_init", "decoder_rnn_inits")
    return all(hasattr(dec, n) for n in need) and isinstance(getattr(dec, "attention_rnn"), nn.LSTMCell) \
        and isinstance(getattr(dec, "decoder_rnn"), nn.LSTMCell) and hasattr(dec.prenet, "layers") \
        and hasattr(dec.attention_layer, "query_layer")


def use_device_decoder(model):
    """Swap ``model.decoder`` (the reference's ``Decoder``, layers/tacotron2.py:97-247, recognised by its structure
    and attributes) for a ``layers.Decoder`` that carries the same weights on the same device in the same training
    mode; returns the model.  Raises ``NotImplementedError`` naming the option, before the model is touched, for
    ``location_attn``, ``trans_agent`` and ``prenet_type="bn"``.  Calling it again changes nothing.  Build the optimizer
    afterwards: the parameters are new tensors (``model.decoder.stopnet`` is the module ``optimizer_st`` walks).
    Measured against the same decoder in torch ops on an MI355X: profiles/decoder_train.json ("timing")."""
    old = model.decoder
    if isinstance(old, Decoder):
        return model
    if not _is_reference_decoder(old):
        raise TypeError("use_device_decoder: model.decoder is not the reference's Decoder")
    a, pre = old.attention_layer, old.prenet
    location = bool(getattr(a, "location_attention", False)) or hasattr(a, "location_layer")
    trans = bool(getattr(a, "trans_agent", False)) or hasattr(a, "ta")
    ptype = getattr(pre, "prenet_type", "original")
    _decoder_unsupported(ptype, trans, location)
    rnn = old.attention_rnn.hidden_size
    new = Decoder(old.encoder_embedding_dim, old.mel_channels, old.r, getattr(a, "windowing", False), a.norm, ptype,
                  getattr(pre, "prenet_dropout", True), a.forward_attn, trans, getattr(a, "forward_attn_mask", False),
                  location, old.separate_stopnet, prenet_dim=pre.layers[-1].linear_layer.out_features, rnn_dim=rnn,
                  attention_dim=a.query_layer.linear_layer.out_features)
    new.load_state_dict(old.state_dict())
    new.p_attention_dropout = getattr(old, "p_attention_dropout", 0.1)
    new.p_decoder_dropout = getattr(old, "p_decoder_dropout", 0.1)
    new.stopnet[0].p = old.stopnet[0].p
    new.to(next(old.parameters()).device)
    new.train(old.training)
    model.decoder = new
    return model


# ---------------------------------------------------------------------- the GRU of the Tacotron / GST family
_GRU_SUFFIXES = ("", "_reverse")


class _GRUFunction(torch.autograd.Function):
    """forward(x [B, T, I], module, h0, *parameters) -> (out, h_n), both differentiable.  The parameters ride along
    so that autograd asks for their gradients; the kernels read the module's repacked copies."""

    @staticmethod
    def forward(ctx, x, module, h0, *params):
        out, h_n, reserve = module._run_forward(x, h0, True)
        ctx.save_for_backward(x, out, reserve, *([] if h0 is None else [h0]))
        ctx.module, ctx.has_h0 = module, h0 is not None
        ctx.versions = module._key()
        ctx.set_materialize_grads(False)  # an unused output's gradient stays None: it is not loaded at all
        return out, h_n

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out, grad_h_n):
        x, out, reserve, *h0 = ctx.saved_tensors
        m = ctx.module
        if m._key() != ctx.versions:
            raise RuntimeError("layers.GRU: the parameters were modified between this forward and its backward")
        need = ctx.needs_input_grad
        if grad_out is None and grad_h_n is None:
            return (None,) * len(need)
        grads = m._run_backward(x, reserve, out, h0[0] if ctx.has_h0 else None, grad_out, grad_h_n, need[0], need[3:])
        return (grads[0], None, None) + tuple(grads[1:])


class GRU(nn.Module):
    """``nn.GRU(input_size, hidden_size, num_layers=1, bias=True, batch_first=True, bidirectional=...)`` on the
    device, a drop-in for the three GRUs of the reference's Tacotron / TacotronGST: the CBHG's
    ``nn.GRU(128, 128, 1, batch_first=True, bidirectional=True)`` of the encoder and of the postnet
    (layers/tacotron.py:165-170, :204-205: ``outputs, _ = gru(x)``) and the GST reference encoder's
    ``nn.GRU(256, 128, batch_first=True)`` (layers/gst_layers.py:53-56, :74-78: ``_, out = gru(x)``, so only ``h_n`` is
    differentiated).  ``tts_gru_forward`` / ``tts_gru_backward`` (csrc/gru_train.hip) run the whole time loop of a
    forward, and of a backward, in one launch each.

    Parameter names, shapes and initialisation are ``nn.GRU``'s, so state dicts load both ways.  ``forward(input,
    hx=None)`` takes a padded ``[B, T, I]`` tensor, every sentence at full length, and returns ``(out, h_n)``; both
    join autograd.  ``hx`` is a constant: an ``hx`` that requires grad raises.  A ``PackedSequence`` raises
    ``NotImplementedError`` (the reference never packs here).  All arithmetic is fp32 on fixed summation orders: the
    same operands give the same bits, forward and backward.

    With grad mode off, in ``eval()`` mode, or when neither the input nor a parameter requires grad, the forward
    keeps nothing for a backward (``last_reserve_floats`` is 0) and ``out``, ``h_n`` have the same bits.  The weights
    are repacked when the parameters' version counters or addresses have changed since the last call (``repacks``
    counts).  Without a GPU a call raises the package's "no GPU" RuntimeError; there is no CPU fallback."""

    def __init__(self, input_size, hidden_size, num_layers=1, bias=True, batch_first=False, dropout=0.0,
                 bidirectional=False, device=None, dtype=None):
        super().__init__()
        for ok, what in ((num_layers == 1, "num_layers != 1"), (bias, "bias=False"),
                         (batch_first, "batch_first=False"), (dropout == 0, "dropout"),
                         (dtype in (None, torch.float32), "a dtype other than float32"),
                         (input_size > 0 and input_size % 16 == 0, "an input_size that is no multiple of 16"),
                         (hidden_size > 0 and hidden_size % 16 == 0, "a hidden_size that is no multiple of 16"),
                         (hidden_size <= 128, "a hidden_size > 128")):
            if not ok:
                raise NotImplementedError(f"layers.GRU does not implement {what}")
        self.input_size, self.hidden_size, self.bidirectional = input_size, hidden_size, bool(bidirectional)
        self.num_layers, self.bias, self.batch_first, self.dropout = 1, True, True, 0.0
        G = 3 * hidden_size
        for suffix in _GRU_SUFFIXES[:self.num_directions]:
            for name, shape in zip(_NAMES, ((G, input_size), (G, hidden_size), (G,), (G,))):
                self.register_parameter(name + suffix, nn.Parameter(torch.empty(shape, device=device)))
        self.reset_parameters()
        self._h = None
        self._packed_key = None
        self.repacks = 0
        self.last_reserve_floats = 0

    @property
    def num_directions(self):
        return 2 if self.bidirectional else 1

    def reset_parameters(self):  # nn.GRU's: U(-1 / sqrt(H), 1 / sqrt(H)) on every parameter
        k = 1.0 / math.sqrt(self.hidden_size)
        for p in self.parameters():
            nn.init.uniform_(p, -k, k)

    def flatten_parameters(self):  # nothing to flatten here
        pass

    def extra_repr(self):
        return f"{self.input_size}, {self.hidden_size}, batch_first=True, bidirectional={self.bidirectional}"

    def __del__(self):
        try:
            if self._h is not None:
                self._h[0].tts_gru_destroy(self._h[1])
        except Exception:
            pass

    # ------------------------------------------------------------------ the handle and its weights
    def _params(self):
        return [getattr(self, n + s) for s in _GRU_SUFFIXES[:self.num_directions] for n in _NAMES]

    def _key(self):
        return tuple((p.data_ptr(), p._version) for p in self._params())

    def _handle(self):
        lib = _native.lib()  # raises without a GPU / library: no CPU fallback
        if self._h is None:
            h = ctypes.c_void_p()
            _native.check(lib.tts_gru_create(self.input_size, self.hidden_size, int(self.bidirectional),
                                             ctypes.byref(h)), "tts_gru_create")
            self._h = (lib, h)
        return self._h

    def _sync_weights(self):
        lib, h = self._handle()
        key = self._key()
        if key == self._packed_key:
            return
        ps = self._params()
        for p in ps:
            if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous() or p.data_ptr() % 16:
                raise ValueError("layers.GRU: parameters must be contiguous 16-byte aligned CUDA float32 tensors")
        per = [_ptr_pair([ps[d * 4 + k] for d in range(self.num_directions)] + [None] * (2 - self.num_directions))
               for k in range(4)]
        _native.check(lib.tts_gru_set_weights(h, *per, _native.stream_handle()), "tts_gru_set_weights")
        self._packed_key = key
        self.repacks += 1

    # ------------------------------------------------------------------ the two calls
    def _run_forward(self, x, h0, want_reserve):
        lib, h = self._handle()
        self._sync_weights()
        B, T, _ = x.shape
        D, H = self.num_directions, self.hidden_size
        x = _aligned(x.detach())
        out = torch.empty(B, T, D * H, dtype=torch.float32, device=x.device)
        h_n = torch.empty(D, B, H, dtype=torch.float32, device=x.device)
        reserve = None
        if want_reserve:
            reserve = torch.empty(lib.tts_gru_reserve_floats(h, B, T), dtype=torch.float32, device=x.device)
        self.last_reserve_floats = 0 if reserve is None else reserve.numel()
        _native.check(lib.tts_gru_forward(h, _ptr(x), B, T, _ptr(h0), _ptr(out), _ptr(h_n), _ptr(reserve),
                                          _native.stream_handle()), "tts_gru_forward")
        return out, h_n, reserve

    def _run_backward(self, x, reserve, out, h0, grad_out, grad_h_n, need_x, need_params):
        lib, h = self._handle()
        B, T, _ = x.shape
        D = self.num_directions
        x = _aligned(x.detach())
        grad_out = None if grad_out is None else _aligned(grad_out)
        grad_h_n = None if grad_h_n is None else _aligned(grad_h_n)
        grad_x = torch.empty_like(x) if need_x else None
        ps = self._params()
        gp = [torch.empty_like(p) if need else None for p, need in zip(ps, need_params)]
        per = [_ptr_pair([gp[d * 4 + k] for d in range(D)] + [None] * (2 - D)) for k in range(4)]
        _native.check(lib.tts_gru_backward(h, _ptr(x), B, T, _ptr(reserve), _ptr(out), _ptr(h0), _ptr(grad_out),
                                           _ptr(grad_h_n), _ptr(grad_x), *per, _native.stream_handle()),
                      "tts_gru_backward")
        return [grad_x] + gp

    def forward(self, input, hx=None):
        if isinstance(input, PackedSequence):
            raise NotImplementedError("layers.GRU does not implement a PackedSequence input (the reference never "
                                      "packs here)")
        x = input
        if x.dim() != 3 or x.shape[2] != self.input_size:
            raise ValueError(f"expected input [B, T, {self.input_size}], got {tuple(x.shape)}")
        if not x.is_cuda:
            _native.lib()  # the "no GPU" error where there is none
            raise RuntimeError("layers.GRU: the input must be a CUDA tensor (there is no CPU path)")
        if x.dtype != torch.float32:
            raise ValueError(f"layers.GRU: the input must be float32, got {x.dtype}")
        B, T, _ = x.shape
        if B < 1 or T < 1:
            raise ValueError(f"layers.GRU: an empty batch or sequence, input {tuple(x.shape)}")
        h0 = None
        if hx is not None:
            if hx.requires_grad:
                raise NotImplementedError("layers.GRU: hx is a constant; gradients with respect to it are not "
                                          "implemented")
            shape = (self.num_directions, B, self.hidden_size)
            if tuple(hx.shape) != shape:
                raise ValueError(f"expected hx {shape}, got {tuple(hx.shape)}")
            h0 = _aligned(hx.detach().to(x.device, torch.float32))
        params = self._params()
        if not (self.training and torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params))):
            return self._run_forward(x, h0, False)[:2]
        return _GRUFunction.apply(x, self, h0, *params)


def _gru_implemented(m):
    return (type(m) is nn.GRU and m.num_layers == 1 and m.bias and m.batch_first and m.dropout == 0
            and getattr(m, "proj_size", 0) == 0 and m.input_size % 16 == 0 and m.hidden_size % 16 == 0
            and m.hidden_size <= 128 and m.weight_ih_l0.dtype == torch.float32)


def use_device_gru(model):
    """Swap every ``nn.GRU`` under ``model`` that ``layers.GRU`` implements (one layer, biases, ``batch_first``, no
    dropout, float32, sizes multiples of 16, ``hidden_size <= 128``) for a ``layers.GRU`` with the same weights on the
    same device in the same training mode; returns the model.  In the reference's ``Tacotron`` / ``TacotronGST`` those
    are exactly ``encoder.cbhg.cbhg.gru``, ``postnet.cbhg.gru`` (layers/tacotron.py:165-170) and
    ``gst.encoder.recurrence`` (layers/gst_layers.py:53-56).  Any other ``nn.GRU`` is left alone; each parameter keeps
    its ``requires_grad``; a ``model`` that is itself such an ``nn.GRU`` comes back as the ``layers.GRU``.  Calling it
    again changes nothing.  Build the optimizer afterwards: the parameters are new tensors."""
    for path, old in list(model.named_modules()):
        if not _gru_implemented(old):
            continue
        new = GRU(old.input_size, old.hidden_size, num_layers=1, bias=True, batch_first=True,
                  bidirectional=old.bidirectional)
        new.load_state_dict(old.state_dict())
        new.to(next(old.parameters()).device)
        new.train(old.training)
        for name, p in old.named_parameters():  # a frozen parameter stays frozen
            getattr(new, name).requires_grad_(p.requires_grad)
        if not path:  # the model is itself the GRU
            return new
        parent = model
        *head, leaf = path.split(".")
        for name in head:
            parent = getattr(parent, name)
        setattr(parent, leaf, new)
    return model
