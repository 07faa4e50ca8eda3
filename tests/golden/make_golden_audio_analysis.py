"""Generate tests/golden/audio_analysis*.npz by running the REFERENCE AudioProcessor's analysis half.

Run in the build container only (needs /root/reference; nothing here runs on the GPU box):

    python tests/golden/make_golden_audio_analysis.py

Built as make_golden.py's make_audio_test_fixture is: the reference's own ``AudioProcessor``
(``utils/audio.py``) with ``librosa`` / ``soundfile`` replaced by the oracle's librosa-0.6.2 restatement,
the audio block of ``tests/test_config.json``, the ten (max_norm, signal_norm, symmetric_norm, clip_norm)
settings of ``AUDIO_TEST_SETTINGS`` and ``tests/inputs/example_1.wav`` read as int16 / 32768.

Two excerpts of the wav (float64), both of a length that is no multiple of the hop:
  xa = x[8000 : 8000 + 20*275 + 37]    21 frames
  xb = x[20000 : 20000 + 4*275 + 100]   5 frames, every one of them touching the reflect padding
Per setting i and excerpt e in "a", "b":
  lin{i}{e}  spectrogram(x)                       [1025, frames] float64 (utils/audio.py:138-144)
  mel{i}{e}  melspectrogram(x)                    [80, frames]   float64 (:146-152)
  l2m{i}{e}  out_linear_to_mel(lin.astype(f32))   [80, frames]   float64 (:174-180)
lin32 is lin.astype(float32) and is not stored (the tests take it from lin).  The float64 lin arrays are
2.1 MB and do not compress, so they go into three archives of their own, each below the 1 MiB a committed
file may have: audio_analysis_lin0.npz (settings 0-3), _lin1 (4-7), _lin2 (8-9); audio_analysis.npz holds
everything else.
The host helpers, once, on a fixed small vector or the first 1000 samples of xa: _normalize at every
setting (norm{i}), _amp_to_db, apply_preemphasis, mulaw_encode at qc 8 and 10 and mulaw_decode of the
codes mapped back to [-1, 1], quantize / dequantize at 8 bits, encode_16bits, _linear_to_mel /
_mel_to_linear on one frame.
"""
from __future__ import annotations

import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (the stubs, the settings, REF)


def main():
    import scipy.io.wavfile
    mg._stub_text_deps()
    mg._stub_audio_deps()
    sys.path.insert(0, mg.REF)
    from utils.audio import AudioProcessor
    txt = open(os.path.join(mg.REF, "tests", "test_config.json")).read()
    conf = json.loads(re.sub(r"//[^\n]*", "", txt))  # the reference's load_config strips // comments
    sr, pcm = scipy.io.wavfile.read(os.path.join(mg.REF, "tests", "inputs", "example_1.wav"))
    assert pcm.dtype == np.int16 and sr == conf["audio"]["sample_rate"]
    x = pcm.astype(np.float64) / 32768.0
    ap = AudioProcessor(**conf["audio"])
    hop = ap.hop_length
    assert hop == 275
    xs = dict(a=x[8000:8000 + 20 * hop + 37], b=x[20000:20000 + 4 * hop + 100])
    out = dict(xa=xs["a"], xb=xs["b"], audio=np.array(repr(conf["audio"])), settings=np.array(mg.AUDIO_TEST_SETTINGS))
    v = np.concatenate([np.linspace(-130.0, 10.0, 29), [-100.0, 0.0, -20.0, -99.999, 1e-3]])  # dB values
    out["norm_in"] = v
    for i, (max_norm, signal_norm, symmetric_norm, clip_norm) in enumerate(mg.AUDIO_TEST_SETTINGS):
        ap.max_norm, ap.signal_norm, ap.symmetric_norm, ap.clip_norm = max_norm, signal_norm, symmetric_norm, clip_norm
        for e, xe in xs.items():
            lin = ap.spectrogram(xe)
            mel = ap.melspectrogram(xe)
            l2m = ap.out_linear_to_mel(lin.astype(np.float32))
            assert lin.dtype == np.float64 and lin.shape == (1025, 1 + len(xe) // hop)
            out[f"lin{i}{e}"], out[f"mel{i}{e}"], out[f"l2m{i}{e}"] = lin, mel, l2m
            print(f"setting {i} {mg.AUDIO_TEST_SETTINGS[i]} x{e}: lin {lin.shape} [{lin.min():.2f}, {lin.max():.2f}] "
                  f"mel {mel.shape} l2m {l2m.dtype} max|l2m - mel| {np.abs(l2m - mel).max():.2e}")
        out[f"norm{i}"] = ap._normalize(v)
    # the small helpers (no normalisation flag reaches them)
    xa = xs["a"]
    xh = xa[:1000]
    amp = np.concatenate([np.logspace(-7, 1, 33), [0.0, 1e-5, 1.0]])
    out["amp_in"], out["amp_to_db"] = amp, ap._amp_to_db(amp)
    out["preemph"] = ap.apply_preemphasis(xh)
    for qc in (8, 10):
        enc = AudioProcessor.mulaw_encode(xh, qc)
        out[f"mulaw_enc{qc}"] = enc
        out[f"mulaw_dec{qc}"] = AudioProcessor.mulaw_decode(2 * enc / (2 ** qc - 1) - 1, qc)
    q = ap.quantize(xh, 8)
    out["quantize8"], out["dequantize8"] = q, ap.dequantize(q, 8)
    out["encode_16bits"] = ap.encode_16bits(xh * 8.0)  # (the loudest samples clip)
    D = np.abs(mg.glo.stft(ap.apply_preemphasis(xa), ap.n_fft, ap.hop_length, ap.win_length))[:, 10:11]
    out["frame_mag"] = D
    out["linear_to_mel"] = ap._linear_to_mel(D)
    out["mel_to_linear"] = ap._mel_to_linear(out["linear_to_mel"])
    parts = {"audio_analysis": {k: a for k, a in out.items() if not k.startswith("lin") or k == "linear_to_mel"}}
    for j, group in enumerate(((0, 1, 2, 3), (4, 5, 6, 7), (8, 9))):
        parts[f"audio_analysis_lin{j}"] = {f"lin{i}{e}": out[f"lin{i}{e}"] for i in group for e in "ab"}
    assert sum(len(p) for p in parts.values()) == len(out)
    for name, part in parts.items():
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **part)
        print(f"{path}: {os.path.getsize(path)} bytes")
        assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
