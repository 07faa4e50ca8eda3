"""Config surface of the reference (utils/generic_utils.py:18-32, 254-289), unchanged formats.

``load_config`` accepts the reference's JSON files as they are (``//`` comments and backslash
line continuations stripped, as utils/generic_utils.py:24-32).  ``setup_model`` accepts both the
3-argument signature of the reference function (``setup_model(num_chars, num_speakers, c)``)
and the 2-argument call its callers make (``synthesize.py:93``, ``server/synthesizer.py:55``),
which raises TypeError in the reference; ``c.num_speakers`` may be absent (it is absent from
every reference config, generic_utils.py:278).

The training helpers of the same file: ``weight_decay`` and ``check_update`` (generic_utils.py:155-182) run on
the device through ``optim.decay_`` / ``optim.clip_`` (csrc/optim.hip) with the reference's signatures and
return values; ``lr_decay``, ``NoamLR``, ``mk_decay`` and ``count_parameters`` are host arithmetic, restated.
"""
from __future__ import annotations

import json
import os
import re

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
CONFIG_DIR = os.path.join(PKG_DIR, "configs")


class AttrDict(dict):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.__dict__ = self


def load_config(config_path: str) -> AttrDict:
    with open(config_path, "r") as f:
        s = f.read()
    s = re.sub(r"\\\n", "", s)
    s = re.sub(r"//.*\n", "\n", s)
    cfg = AttrDict()
    cfg.update(json.loads(s))
    return cfg


def default_config(name: str = "config_tacotron2.json") -> AttrDict:
    return load_config(os.path.join(CONFIG_DIR, name))


def sequence_mask(sequence_length, max_len=None):  # utils/generic_utils.py:209-220
    """Bool [B, max_len]: position t of row b is True for t < sequence_length[b] (on the lengths' device)."""
    import torch
    if max_len is None:
        max_len = int(sequence_length.max())
    seq_range = torch.arange(0, max_len, device=sequence_length.device).long()
    return seq_range.unsqueeze(0) < sequence_length.unsqueeze(1)


def check_update(model, grad_clip):  # utils/generic_utils.py:155-162
    """``clip_grad_norm_`` in place on the device plus the reference's inf test: ``(grad_norm, skip_flag)``.
    ``model`` is an ``nn.Module`` or an iterable of parameters; ``grad_norm`` is a 0-dim CUDA float32 tensor.
    Waits for the device where the reference's ``np.isinf(grad_norm)`` does."""
    import math
    from . import optim
    params = model.parameters() if hasattr(model, "parameters") else model
    grad_norm, value = optim.clip_(params, grad_clip)
    skip_flag = False
    if math.isinf(value):
        print(" | > Gradient is INF !!")
        skip_flag = True
    return grad_norm, skip_flag


def lr_decay(init_lr, global_step, warmup_steps):  # utils/generic_utils.py:165-171
    warmup_steps = float(warmup_steps)
    step = global_step + 1.
    return init_lr * warmup_steps**0.5 * min(step * warmup_steps**-1.5, step**-0.5)


def weight_decay(optimizer, wd):  # utils/generic_utils.py:174-182
    """The reference's custom weight decay, ``p <- p + (-wd * lr) * p`` on every parameter of every group, on
    the device and in place (the reference binds a new tensor to ``param.data``).  ``optimizer`` is an
    ``optim.Adam`` or any torch optimizer over CUDA float32 parameters.  Returns ``(optimizer, current_lr)``."""
    from . import optim
    for group in optimizer.param_groups:
        current_lr = group['lr']
        optim.decay_(group['params'], current_lr, wd)
    return optimizer, current_lr


def __getattr__(name):  # NoamLR subclasses a torch class: made on first use, importing this module stays cheap
    if name != "NoamLR":
        raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
    import torch

    class NoamLR(torch.optim.lr_scheduler._LRScheduler):  # utils/generic_utils.py:185-196
        def __init__(self, optimizer, warmup_steps=0.1, last_epoch=-1):
            self.warmup_steps = float(warmup_steps)
            super().__init__(optimizer, last_epoch)

        def get_lr(self):
            step = max(self.last_epoch, 1)
            return [base_lr * self.warmup_steps**0.5 * min(step * self.warmup_steps**-1.5, step**-0.5)
                    for base_lr in self.base_lrs]

    globals()["NoamLR"] = NoamLR
    return NoamLR


def mk_decay(init_mk, max_epoch, n_epoch):  # utils/generic_utils.py:199-200
    return init_mk * ((max_epoch - n_epoch) / max_epoch)


def count_parameters(model):  # utils/generic_utils.py:203-205
    r"""Count number of trainable parameters in a network"""
    return sum(p.numel() for p in model.parameters() if p.requires_grad)


def setup_model(num_chars, num_speakers_or_c, c=None, **kw):
    if c is None:
        c, num_speakers = num_speakers_or_c, getattr(num_speakers_or_c, "num_speakers", 0) or 0
    else:
        num_speakers = num_speakers_or_c
    model = c.model.lower()
    if model == "tacotron2":
        from .tacotron2 import Tacotron2
        return Tacotron2(num_chars=num_chars, num_speakers=num_speakers, r=c.r, attn_win=c.windowing,
                         attn_norm=c.attention_norm, prenet_type=c.prenet_type, prenet_dropout=c.prenet_dropout,
                         forward_attn=c.use_forward_attn, trans_agent=c.transition_agent,
                         forward_attn_mask=c.forward_attn_mask, location_attn=c.location_attn,
                         separate_stopnet=c.separate_stopnet, **kw)
    if model in ("tacotron", "tacotrongst"):  # utils/generic_utils.py:258-274
        from .tacotron import Tacotron, TacotronGST
        cls = TacotronGST if model == "tacotrongst" else Tacotron
        return cls(num_chars=num_chars, num_speakers=num_speakers, r=c.r, linear_dim=1025, mel_dim=80,
                   memory_size=c.memory_size, attn_win=c.windowing, attn_norm=c.attention_norm,
                   prenet_type=c.prenet_type, prenet_dropout=c.prenet_dropout, forward_attn=c.use_forward_attn,
                   trans_agent=c.transition_agent, forward_attn_mask=c.forward_attn_mask,
                   location_attn=c.location_attn, separate_stopnet=c.separate_stopnet, **kw)
    raise NotImplementedError(f"model {c.model!r} is not one of Tacotron2, Tacotron, TacotronGST")
