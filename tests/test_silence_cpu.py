"""CPU: the inputs of the device silence tests (silence_util.py) meet the condition that lets the GPU test
demand exact integers, the host comparators' results on them are pinned, and the C-ABI declares, binds and
exports tts_gl_trim_silence / tts_gl_find_endpoint / tts_gl_take_segments."""
import os
import re

import numpy as np

import silence_util as su
from conftest import REPO, golden, load_pkg

NEW_SYMBOLS = ("tts_gl_trim_silence", "tts_gl_find_endpoint", "tts_gl_take_segments")

# host trim_silence on the ten signals: (start, end) relative to the margin-stripped signal
TRIM_EXPECTED = [(0, 513), (0, 1024), (0, 1279), (0, 1280), (0, 768), (256, 1280), (768, 3000), (0, 2560),
                 (0, 1500), (0, 1500)]


def test_trim_inputs_keep_every_frame_a_decibel_from_the_threshold():
    """Every frame of every trim signal lies more than 1 dB from -top_db in the host restatement (6.3 dB
    at the least, the single loud sample; 39.6 dB for the background-only signal), so a device log10 or
    summation order that differs from numpy's in the last bits cannot move a frame across the threshold.
    A condition on the inputs: the GPU test allows no mismatch."""
    margins = [float(np.min(np.abs(su.trim_frame_db(y) + 40.0))) for y in su.trim_signals()]
    assert len(margins) == 10
    assert min(margins) > 1.0, margins
    assert abs(min(margins) - 6.3) < 0.1 and abs(margins[-1] - 39.6) < 0.1, margins


def test_real_audio_keeps_every_frame_a_decibel_from_the_threshold():
    """The same condition for the recording the GPU test trims (audio_example1.npz, 0.1 s margins at
    22 050 Hz): 147 frames, the nearest 9.7 dB from the threshold."""
    y = golden("audio_example1")["pcm"].astype(np.float64) / 32768.0
    db = su.trim_frame_db(y[2205:-2205])
    assert len(db) == 147 and float(np.min(np.abs(db + 40.0))) > 1.0


def test_host_trim_results_pinned():
    ap = su.processor(su.TRIM_SR)
    margin = int(ap.sample_rate * 0.1)
    assert margin == 200
    sigs, wavs = su.trim_signals(), su.trim_wavs(margin)
    assert [len(w) - len(y) for y, w in zip(sigs, wavs)] == [400] * 10
    got = [su.host_trim_bounds(ap, w) for w in wavs]
    assert got == TRIM_EXPECTED
    for (s, e), y, w in zip(got, sigs, wavs):
        assert np.array_equal(ap.trim_silence(w), y[s:e])


def test_host_endpoint_cases_cover_both_outcomes():
    """The endpoint inputs are not trivially all-N or all-found, for both windows (800 and 801)."""
    ap = su.processor(su.END_SR)
    for sec, window in ((0.8, 800), (0.801, 801)):
        assert int(ap.sample_rate * sec) == window and int(window / 4) == 200
        cases = su.endpoint_cases(ap, sec)
        assert all(700 <= len(y) <= 3000 for y in cases)
        ends = [ap.find_endpoint(y, min_silence_sec=sec) for y in cases]
        assert ends == [700, window, window + 200, 400, window + 201, 400, 400, 400, 600, 1200,
                        1000 + window, 2999, 800, 3000, 600, 3000, 600]


def test_new_entry_points_declared_bound_and_exported():
    n = load_pkg("_native")
    header = open(os.path.join(REPO, "include", "tts_hip.h")).read()
    lib = n.load_library()
    for s in NEW_SYMBOLS:
        assert s in n.EXPORTS, s
        assert re.search(r"\btts_status\s+" + s + r"\s*\(", header), s
        fn = getattr(lib, s)
        assert fn.argtypes is not None and fn.restype is not None
