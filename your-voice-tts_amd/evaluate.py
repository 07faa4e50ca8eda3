"""The batch step and the loop of the reference's ``evaluate()`` (train.py:264-394) on the device.

``evaluate_batch`` takes a collated batch (``datasets.collate_fn``), runs the model's teacher-forced
``forward`` and the three criteria of train.py:462-465; the forward's outputs go into the loss calls as
they come, and only the scalars reach the host.  ``evaluate`` collates ``items`` batch by batch and
averages as train.py:385-394 does.  Evaluation only; ``reduce_tensor`` across ranks, the TensorBoard
logging and the eval-time test sentences of the reference are not part of it.
"""
from __future__ import annotations

import torch

from . import losses
from .datasets import collate_fn


def group_stop_targets(stop_targets, r):
    """One stop target per decoder step: 1 when any of the step's r frames' targets is
    (train.py:306-309).  [B, Tpad] -> [B, Tpad // r]."""
    B, T = stop_targets.shape
    return (stop_targets.view(B, T // r, -1).sum(2) > 0.0).float()


def _criteria(c):
    """(criterion, criterion_st) as train.py:461-465 picks them; both keys default to the value every
    reference config has (true)."""
    tacotron = c.model in ("Tacotron", "TacotronGST")
    if c.get("loss_masking", True):
        criterion = losses.L1LossMasked() if tacotron else losses.MSELossMasked()
    else:
        criterion = losses.L1Loss() if tacotron else losses.MSELoss()
    return criterion, (losses.BCEWithLogitsLoss() if c.get("stopnet", True) else None)


def evaluate_batch(model, c, batch, speaker_mapping=None):
    """train.py:289-340 for one collated batch.  Returns dict(decoder_loss, postnet_loss, stop_loss, loss:
    Python floats, the criteria's fp64 values; per_sentence: dict(decoder, postnet) of CUDA float64 [B]
    sums over each sentence's valid rows; stop_targets: the grouped targets; outputs: the forward's
    (decoder_output, postnet_output, alignments, stop_tokens))."""
    text, text_lengths, speaker_names, linear, mel, mel_lengths, stop_targets, _ = batch
    tacotron = c.model in ("Tacotron", "TacotronGST")
    speaker_ids = None
    if c.get("use_speaker_embedding", False):
        speaker_ids = torch.LongTensor([speaker_mapping[name] for name in speaker_names])
    stop_targets = group_stop_targets(stop_targets, c.r)
    criterion, criterion_st = _criteria(c)
    decoder_output, postnet_output, alignments, stop_tokens = model.forward(text, text_lengths, mel,
                                                                            speaker_ids=speaker_ids)
    stop_loss = 0.0
    if criterion_st is not None:
        criterion_st(stop_tokens, stop_targets)
        stop_loss = criterion_st.last_value
    length = (mel_lengths,) if c.get("loss_masking", True) else ()
    criterion(decoder_output, mel, *length)
    decoder_loss, per_decoder = criterion.last_value, criterion.last_per_sentence
    criterion(postnet_output, linear if tacotron else mel, *length)
    postnet_loss, per_postnet = criterion.last_value, criterion.last_per_sentence
    return dict(decoder_loss=decoder_loss, postnet_loss=postnet_loss, stop_loss=stop_loss,
                loss=decoder_loss + postnet_loss + stop_loss,
                per_sentence=dict(decoder=per_decoder, postnet=per_postnet), stop_targets=stop_targets,
                outputs=(decoder_output, postnet_output, alignments, stop_tokens))


def evaluate(model, c, ap, items, batch_size, speaker_mapping=None):
    """The validation loop of train.py:286-394 over ``items`` (dicts as MyDataset.load_data yields them) in
    batches of ``batch_size``.  Returns the batch averages under the reference's keys: loss_postnet,
    loss_decoder, stop_loss."""
    sums = dict(loss_postnet=0.0, loss_decoder=0.0, stop_loss=0.0)
    batches = 0
    for i in range(0, len(items), batch_size):
        out = evaluate_batch(model, c, collate_fn(items[i:i + batch_size], ap, c.r), speaker_mapping)
        sums["loss_postnet"] += out["postnet_loss"]
        sums["loss_decoder"] += out["decoder_loss"]
        sums["stop_loss"] += out["stop_loss"]
        batches += 1
    return {k: v / batches for k, v in sums.items()}
