"""Shared by test_audio_analysis_cpu.py and test_gpu_audio_analysis.py: the audio_analysis*.npz fixture
(tests/golden/make_golden_audio_analysis.py), its settings as AudioProcessor arguments, and spectrogram /
out_linear_to_mel composed from the oracle's pieces."""
import ast

import numpy as np

from conftest import golden
from oracle.griffin_lim_oracle import stft

Z = {k: v for name in ("audio_analysis", "audio_analysis_lin0", "audio_analysis_lin1", "audio_analysis_lin2")
     for k, v in golden(name).items()}
SETTINGS = [tuple(s) for s in Z["settings"]]
EXCERPTS = ("a", "b")


def cfg(i, **over):
    audio = ast.literal_eval(str(Z["audio"]))
    max_norm, signal_norm, symmetric_norm, clip_norm = SETTINGS[i]
    return {**audio, "max_norm": max_norm, "signal_norm": bool(signal_norm),
            "symmetric_norm": bool(symmetric_norm), "clip_norm": bool(clip_norm), **over}


def oracle_spectrogram(o, y):  # utils/audio.py:138-144 composed from the oracle's pieces
    y = o.apply_preemphasis(y) if o.preemphasis != 0 else y
    D = stft(y, o.n_fft, o.hop_length, o.win_length)
    return o.normalize(o.amp_to_db(np.abs(D)) - o.ref_level_db)


def oracle_out_linear_to_mel(o, linear_spec):  # utils/audio.py:174-180
    S = o.db_to_amp(o.denormalize(linear_spec) + o.ref_level_db)
    S = np.dot(o.mel_basis(), np.abs(S))
    return o.normalize(o.amp_to_db(S) - o.ref_level_db)
