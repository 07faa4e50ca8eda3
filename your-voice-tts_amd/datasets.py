"""``MyDataset.collate_fn`` (datasets/TTSDataset.py:167-228) with the features computed on the device.

``collate_fn(batch, ap, outputs_per_step)`` takes the dicts ``MyDataset.load_data`` yields and returns the
reference's 8-tuple in the reference's order.  The wavs are uploaded once as one ragged float64 batch
(float32 -> float64 is exact, and the reference's pre-emphasis ``lfilter`` promotes to float64 as well);
``AudioProcessor.features_batch`` writes both spectrograms frame-major with ``Tpad`` rows per sentence and
zeroes every row at and beyond a sentence's frames: the zero frame and the padding.  ``linear``, ``mel``
and ``stop_targets`` stay on the device (train.py:312-317 moves them there anyway); the integer tensors
stay on the host like the reference's.
"""
from __future__ import annotations

import numpy as np
import torch

from .data import padded_length, prepare_data


def collate_plan(text_lens, samples, hop, r):
    """The integers of a collated batch, from the items' text lengths and wav lengths alone.

    Returns (order, frames, Tpad, mel_lengths): ``order[i]`` is the item that becomes sentence i (a STABLE
    descending sort by text length), ``frames[i]`` = 1 + samples // hop its spectrogram frames,
    ``mel_lengths[i]`` = frames[i] + 1 (the zero frame) and ``Tpad`` = max frames + 1 rounded up to a
    multiple of r."""
    order = sorted(range(len(text_lens)), key=lambda i: -int(text_lens[i]))
    frames = [1 + int(samples[i]) // int(hop) for i in order]
    return order, frames, padded_length(max(frames), int(r)), [f + 1 for f in frames]


def collate_fn(batch, ap, outputs_per_step):
    """batch: list of dicts with ``text`` (int32 ids), ``wav`` (float32 ndarray), ``item_idx`` and
    ``speaker_name``.  Returns (text LongTensor [B, Lmax], text_lengths LongTensor [B] descending,
    speaker_name list, linear CUDA float32 [B, Tpad, num_freq], mel CUDA float32 [B, Tpad, num_mels],
    mel_lengths LongTensor [B], stop_targets CUDA float32 [B, Tpad], item_idxs list).

    The sort by text length is stable: items of equal text length keep their order in ``batch``.  The
    reference's ``torch.sort`` leaves the order of equal lengths unspecified."""
    ap._handle()  # raises without a GPU / library: no CPU fallback
    text_lens = [len(d["text"]) for d in batch]
    order, frames, Tpad, mel_lengths = collate_plan(text_lens, [len(d["wav"]) for d in batch], ap.hop_length,
                                                    outputs_per_step)
    items = [batch[i] for i in order]
    text = prepare_data([np.asarray(d["text"]) for d in items]).astype(np.int32)
    N = [len(d["wav"]) for d in items]
    host = np.zeros((len(items), max(N)), dtype=np.float64)
    for b, d in enumerate(items):
        host[b, :N[b]] = d["wav"]
    mel, linear, F = ap.features_batch(torch.from_numpy(host).cuda(), N, Fmax=Tpad)
    assert F == frames
    # 0 for a sentence's frames, 1 from its zero frame on (datasets/TTSDataset.py:197-203)
    stop_targets = (torch.arange(Tpad, device=mel.device)[None, :] >=
                    torch.tensor(frames, device=mel.device)[:, None]).float()
    return (torch.LongTensor(text), torch.LongTensor([text_lens[i] for i in order]),
            [d["speaker_name"] for d in items], linear, mel, torch.LongTensor(mel_lengths), stop_targets,
            [d["item_idx"] for d in items])
