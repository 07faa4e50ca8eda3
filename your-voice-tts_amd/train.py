"""One iteration of the reference's ``train()`` (train.py:92-169) on the device criteria and ``optim.Adam``.

``train_batch`` takes a collated batch (``datasets.collate_fn``) and runs, in the reference's order: the
speaker ids, the grouped stop targets, ``scheduler.step()``, ``zero_grad()``, the model's teacher-forced
forward, the three criteria of train.py:462-465 (``losses``: the values are bitwise those ``evaluate_batch``
reports for the same outputs), ``loss.backward()``, and the update: ``optim.Adam.step_fused`` when the optimizer
is the package's, ``weight_decay(); check_update(); optimizer.step()`` otherwise.  Forward and backward of the
*model* stay the caller's torch, except for the encoder's LSTM once ``layers.use_device_lstm(model)`` has swapped
it for ``layers.LSTM`` (``tts_lstm_forward`` / ``tts_lstm_backward``; build the optimizer after the swap); the
criteria's backward is ``tts_loss_backward``.  ``layers.use_device_convs(model)`` does the same for every conv-BN
block of ``encoder.convolutions`` and ``postnet.convolutions`` (``layers.ConvBNBlock``: ``tts_convbn_forward`` /
``tts_convbn_backward``), after which the whole encoder and the whole Postnet train on the device, and
``layers.use_device_decoder(model)`` for the decoder (``layers.Decoder``: ``tts_dectrain_forward`` /
``tts_dectrain_backward``); with the three swaps every trainable layer of the shipped Tacotron2 configuration runs in
HIP, and only the embedding lookup and the tensor glue stay torch.  With a separate stopnet the stop tokens of
``layers.Decoder`` are an autograd node of their own that reads the forward's reserve alone, so the second
``stop_loss.backward()`` works after the first backward and the main optimizer's step.  For a Tacotron-family model
(``c.model in ("Tacotron", "TacotronGST")``) ``layers.use_device_gru(model)`` swaps the three ``nn.GRU``s
(``encoder.cbhg.cbhg.gru``, ``postnet.cbhg.gru``, ``gst.encoder.recurrence``) for ``layers.GRU`` (``tts_gru_forward`` /
``tts_gru_backward``; build the optimizer after the swap); the family's other layers stay the caller's torch.

Not part of it: the epoch loop, the logging, checkpoints, ``reduce_tensor`` across ranks and the diagnostic
audio of train.py:171-260.
"""
from __future__ import annotations

import torch

from . import optim
from .evaluate import _criteria, group_stop_targets
from .generic_utils import check_update, weight_decay


def train_batch(model, c, batch, optimizer, optimizer_st=None, scheduler=None, speaker_mapping=None):
    """train.py:92-169 for one collated batch.  ``model`` is the caller's ``torch.nn.Module`` in ``train()``
    mode, with the reference's ``forward(text, text_lengths, mel, speaker_ids=...)`` and, for
    ``c.separate_stopnet``, a ``decoder.stopnet`` that ``optimizer_st`` updates.  The operands go to the device of
    the model's parameters; ``mel_lengths`` stays on the host, where the criteria read it.  ``loss_masking``,
    ``stopnet`` and ``separate_stopnet`` default to true and ``lr_decay`` to false when the config lacks them;
    the separate stopnet update needs ``c.stopnet`` (the reference's ``torch.zeros(1)`` has nothing to walk back
    through).

    Returns dict(decoder_loss, postnet_loss, stop_loss, loss: Python floats, the criteria's fp64 values, ``loss``
    the sum of those that went into ``loss.backward()``; grad_norm, grad_norm_st: 0-dim tensors, the second 0
    without a separate stopnet; current_lr: the learning rate used; stop_targets: the grouped targets; outputs:
    the forward's (decoder_output, postnet_output, alignments, stop_tokens))."""
    text, text_lengths, speaker_names, linear, mel, mel_lengths, stop_targets, _ = batch
    tacotron = c.model in ("Tacotron", "TacotronGST")
    stopnet = c.get("stopnet", True)
    separate = c.get("separate_stopnet", True) and stopnet
    speaker_ids = None
    if c.get("use_speaker_embedding", False):
        speaker_ids = torch.LongTensor([speaker_mapping[name] for name in speaker_names])
    stop_targets = group_stop_targets(stop_targets, c.r)

    if c.get("lr_decay", False) and scheduler is not None:
        scheduler.step()
    optimizer.zero_grad()
    if optimizer_st:
        optimizer_st.zero_grad()

    device = next(model.parameters()).device
    text, text_lengths, mel, stop_targets = (t.to(device, non_blocking=True)
                                             for t in (text, text_lengths, mel, stop_targets))
    linear = linear.to(device, non_blocking=True) if tacotron else None
    if speaker_ids is not None:
        speaker_ids = speaker_ids.to(device, non_blocking=True)

    decoder_output, postnet_output, alignments, stop_tokens = model(text, text_lengths, mel, speaker_ids=speaker_ids)

    criterion, criterion_st = _criteria(c)
    stop_loss, stop_value = None, 0.0
    if criterion_st is not None:
        stop_loss = criterion_st(stop_tokens, stop_targets)
        stop_value = criterion_st.last_value
    length = (mel_lengths,) if c.get("loss_masking", True) else ()
    decoder_loss = criterion(decoder_output, mel, *length)
    decoder_value = criterion.last_value
    postnet_loss = criterion(postnet_output, linear if tacotron else mel, *length)
    postnet_value = criterion.last_value
    loss, value = decoder_loss + postnet_loss, decoder_value + postnet_value
    if stopnet and not separate:
        loss, value = loss + stop_loss, value + stop_value

    loss.backward()
    if isinstance(optimizer, optim.Adam):
        grad_norm, current_lr = optimizer.step_fused(c.wd, c.grad_clip)
    else:
        optimizer, current_lr = weight_decay(optimizer, c.wd)
        grad_norm, _ = check_update(model, c.grad_clip)
        optimizer.step()

    if separate:
        stop_loss.backward()
        optimizer_st, _ = weight_decay(optimizer_st, c.wd)
        grad_norm_st, _ = check_update(model.decoder.stopnet, 1.0)
        optimizer_st.step()
    else:
        grad_norm_st = torch.zeros((), device=grad_norm.device)

    return dict(decoder_loss=decoder_value, postnet_loss=postnet_value, stop_loss=stop_value, loss=value,
                grad_norm=grad_norm, grad_norm_st=grad_norm_st, current_lr=current_lr, stop_targets=stop_targets,
                outputs=(decoder_output, postnet_output, alignments, stop_tokens))
