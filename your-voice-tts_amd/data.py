"""The reference's batch padding helpers (utils/data.py), host numpy."""
from __future__ import annotations

import numpy as np


def _pad_data(x, length):
    assert x.ndim == 1
    return np.pad(x, (0, length - x.shape[0]), mode="constant", constant_values=0)


def prepare_data(inputs):  # utils/data.py:11-13
    max_len = max((len(x) for x in inputs))
    return np.stack([_pad_data(x, max_len) for x in inputs])


def _pad_tensor(x, length):
    assert x.ndim == 2
    return np.pad(x, [[0, 0], [0, length - x.shape[1]]], mode="constant", constant_values=0)


def padded_length(max_len, out_steps):
    """max_len + 1 (the zero frame) rounded up to a multiple of out_steps (utils/data.py:27-29, 41-43)."""
    max_len = max_len + 1
    remainder = max_len % out_steps
    return max_len + (out_steps - remainder) if remainder > 0 else max_len


def prepare_tensor(inputs, out_steps):  # utils/data.py:26-30
    pad_len = padded_length(max((x.shape[1] for x in inputs)), out_steps)
    return np.stack([_pad_tensor(x, pad_len) for x in inputs])


def _pad_stop_target(x, length):
    assert x.ndim == 1
    return np.pad(x, (0, length - x.shape[0]), mode="constant", constant_values=1.)


def prepare_stop_target(inputs, out_steps):  # utils/data.py:40-44
    pad_len = padded_length(max((x.shape[0] for x in inputs)), out_steps)
    return np.stack([_pad_stop_target(x, pad_len) for x in inputs])


def pad_per_step(inputs, pad_len):  # utils/data.py:47-52
    return np.pad(inputs, [[0, 0], [0, 0], [0, pad_len]], mode="constant", constant_values=0.0)
