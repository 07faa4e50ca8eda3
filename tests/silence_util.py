"""Shared by test_silence_cpu.py and test_gpu_silence.py: the deterministic inputs of the silence tests
and the processors they run on.  The comparators are the host AudioProcessor.trim_silence /
find_endpoint (utils/audio.py:203-217 restated)."""
import numpy as np

from conftest import load_pkg, tacotron2_config

# (n, a, b): 1e-4 * randn(n) background, sin(0.3 t) + 0.2 added on [a, b).  513 is the shortest signal the
# kernel takes; 1279 / 1280 / 1281 straddle the 1 + n // 256 frame-count edge; (1280, 512, 1280) needs the
# min(n, .) clamp; (2048, 700, 701) is one loud sample; (2560, 0, 2560) is loud throughout.
TRIM_CASES = [(513, 100, 300), (1024, 256, 768), (1279, 511, 513), (1280, 512, 1280), (1281, 0, 255),
              (2048, 700, 701), (3000, 1024, 2816), (2560, 0, 2560)]
TRIM_SR = 2000  # margin = 200 samples
END_SR = 1000   # min_silence_sec 0.8 -> window 800, hop 200; 0.801 -> window 801, hop 200


def processor(sample_rate=None, **over):
    """config_tacotron2.json's AudioProcessor, optionally at another sample rate (the mel band then spans
    the whole spectrum: the config's mel_fmax lies above a small rate's Nyquist)."""
    a = dict(tacotron2_config()["audio"])
    if sample_rate is not None:
        a.update(sample_rate=sample_rate, mel_fmin=0.0, mel_fmax=None)
    a.update(over)
    return load_pkg("audio").AudioProcessor(**a)


def trim_signals():
    """The ten margin-stripped trim signals, in a fixed order: TRIM_CASES, all-zero, background only."""
    rng = np.random.RandomState(7)
    out = []
    for n, a, b in TRIM_CASES:
        y = 1e-4 * rng.randn(n)
        t = np.arange(a, b)
        y[a:b] += np.sin(0.3 * t) + 0.2
        out.append(y)
    out.append(np.zeros(1500))
    out.append(1e-4 * rng.randn(1500))
    return out


def with_margins(y, margin, rng):
    """A wav whose margin-stripped signal is y (the margins hold loud samples: they must not be read)."""
    return np.concatenate([3.0 * rng.randn(margin), y, 3.0 * rng.randn(margin)])


def trim_wavs(margin):
    rng = np.random.RandomState(7 + 1)
    return [with_margins(y, margin, rng) for y in trim_signals()]


def host_trim_bounds(ap, wav):
    """(start, end) of the host trim_silence, relative to the margin-stripped signal: the slice it returns,
    located through numpy's view arithmetic (an empty result is (0, 0))."""
    margin = int(ap.sample_rate * 0.1)
    wav = np.ascontiguousarray(wav, dtype=np.float64)
    out = ap.trim_silence(wav)
    if out.size == 0:
        return 0, 0
    start = (out.__array_interface__["data"][0] - wav.__array_interface__["data"][0]) // wav.itemsize - margin
    return int(start), int(start + len(out))


def trim_frame_db(y, frame_length=1024, hop_length=256):
    """The host restatement's per-frame dB against the loudest frame (audio.py's trim_silence body)."""
    yp = np.pad(y, frame_length // 2, mode="reflect")
    n_frames = 1 + (len(yp) - frame_length) // hop_length
    idx = np.arange(frame_length)[:, None] + hop_length * np.arange(n_frames)[None, :]
    mse = np.sqrt(np.mean(np.abs(yp[idx]) ** 2, axis=0)) ** 2
    return 10.0 * np.log10(np.maximum(1e-10, mse)) - 10.0 * np.log10(np.maximum(1e-10, mse.max()))


def ragged(rows, fill):
    """[B, Nmax] float64 with row b's samples first and fill(b, count) behind them, and the lengths."""
    N = [len(r) for r in rows]
    out = np.empty((len(rows), max(N)), dtype=np.float64)
    for b, r in enumerate(rows):
        out[b, :N[b]] = r
        out[b, N[b]:] = fill(b, max(N) - N[b])
    return out, N


def endpoint_signal(N, silent):
    """0.5 * sin with the stretches [a, b) of `silent` at amplitude 1e-4."""
    t = np.arange(N)
    y = 0.5 * np.sin(0.37 * t + 2.0)
    for a, b in silent:
        y[a:b] = 1e-4 * np.sin(1.3 * t[a:b])
    return y


def endpoint_cases(ap, min_silence_sec):
    """Signals for find_endpoint at END_SR (N between 700 and 3000), cases (i)-(vi) of the GPU test."""
    window = int(ap.sample_rate * min_silence_sec)
    hop = int(window / 4)
    thr = float(ap._db_to_amp(-40))
    cases = []
    # (i) N <= window + hop: no candidate, the result is N
    for N in (700, window, window + hop):
        cases.append(endpoint_signal(N, [(0, N)]))
    # one candidate only (N = window + hop + 1), silent and loud
    cases.append(endpoint_signal(window + hop + 1, [(0, window + hop + 1)]))
    cases.append(endpoint_signal(window + hop + 1, []))
    # (ii) silence of window + 250 samples starting at 0, 199, 200, 201, 1000
    for s in (0, 199, 200, 201, 1000):
        cases.append(endpoint_signal(3000, [(s, s + window + 250)]))
    # (iii) silence only in the last `window` samples: the candidate x = N - window is excluded
    for N in (5 * hop + window, 2999):
        cases.append(endpoint_signal(N, [(N - window, N)]))
    # (iv) a stretch of -0.5: silent under the signed maximum
    y = endpoint_signal(2600, [])
    y[450:450 + window + 2 * hop] = -0.5
    cases.append(y)
    # (v) one sample exactly the threshold inside an otherwise silent window: not silent (strict <)
    y = endpoint_signal(3000, [(400, 400 + window)])
    y[400 + window - 1] = thr
    cases.append(y)
    y = endpoint_signal(3000, [(400, 400 + window)])
    y[400 + window - 1] = np.nextafter(thr, 0.0)
    cases.append(y)
    # (vi) a loud sample at x + window - 1 of the first otherwise silent window (window 801: the remainder
    # sample x + 800), and just behind the window
    for off in (window - 1, window):
        y = endpoint_signal(3000, [(2 * hop, 2 * hop + window + 3 * hop)])
        y[2 * hop + off] = 0.4
        cases.append(y)
    return cases
