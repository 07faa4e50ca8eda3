"""Shared by test_resample_cpu.py and test_gpu_resample.py: the comparator of the device resampler.

librosa and resampy are not installed, so the comparator is a numpy restatement of librosa 0.6.2
``load`` / ``resample`` / ``to_mono`` / ``fix_length`` and resampy 0.2.x ``resample_f`` (DESIGN
"Resampling": unpinned against the real libraries).  Everything is float64 with one rounding per
operation, except the accumulator, which is float32 as resampy's output array takes x's dtype.
``resample_ref`` is vectorised over the outputs and sequential over the taps; ``resample_literal`` is the
triple loop as resampy writes it, for the self-check."""
import numpy as np
import scipy.signal

KAISER_BEST = dict(num_zeros=64, precision=9, beta=14.769656459379492, rolloff=0.9475937167399596)

# the ragged batch of the GPU test: (orig_sr, target_sr, N)
CASES = [(48000, 22050, 3000), (48000, 22050, 50), (48000, 22050, 3), (44100, 22050, 3001),
         (16000, 22050, 3000), (16000, 22050, 40), (8000, 22050, 700), (22050, 16000, 2205),
         (96000, 22050, 4000), (22050, 22050, 600)]


def sinc_window(num_zeros=64, precision=9, beta=14.769656459379492, rolloff=0.9475937167399596):
    """resampy.filters.sinc_window with a Kaiser taper: (half_win, num_table)."""
    num_table = 2 ** precision
    n = num_table * num_zeros
    sinc_win = rolloff * np.sinc(rolloff * np.linspace(0, num_zeros, num=n + 1, endpoint=True))
    taper = scipy.signal.windows.kaiser(2 * n + 1, beta)[n:]
    return taper * sinc_win, num_table


_FILTERS = {}


def kaiser_best():
    if "best" not in _FILTERS:
        _FILTERS["best"] = sinc_window(**KAISER_BEST)
    return _FILTERS["best"]


def small_filter():
    """num_zeros=4, precision=3: 33 entries, num_table 8."""
    return sinc_window(num_zeros=4, precision=3)


def signal(N, sr):
    t = np.arange(N)
    return (0.5 * np.sin(2 * np.pi * 440 * t / sr) + 0.01 * np.random.RandomState(11).randn(N)).astype(np.float32)


def lengths(N, orig_sr, target_sr):
    ratio = float(target_sr) / orig_sr
    return int(N * ratio), int(np.ceil(N * ratio))


def time_register(n, inc, serial=True):
    """resampy's time_register at each output: a serial float64 sum of inc (or, for the teeth test, t * inc)."""
    if not serial:
        return np.arange(n) * inc
    tr = np.empty(n, dtype=np.float64)
    acc = 0.0
    for t in range(n):
        tr[t] = acc
        acc += inc
    return tr


def _setup(x, orig_sr, target_sr, filt):
    half_win, num_table = kaiser_best() if filt is None else filt
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 1
    ratio = float(target_sr) / orig_sr
    n_res, n_fix = lengths(len(x), orig_sr, target_sr)
    assert n_res >= 1
    win = half_win * ratio if ratio < 1 else half_win
    delta = np.zeros_like(win)
    delta[:-1] = win[1:] - win[:-1]
    scale = min(1.0, ratio)
    inc = 1.0 / ratio
    step = int(scale * num_table)
    return x, n_res, n_fix, win, delta, scale, inc, step, num_table


def resample_ref(x, orig_sr, target_sr, filt=None, serial_register=True, acc_dtype=np.float32):
    """librosa.resample(x, orig_sr, target_sr, res_type="kaiser_best", fix=True) of a float32 signal: float32
    [n_fix].  serial_register / acc_dtype select the two deviations the teeth test tells apart."""
    if orig_sr == target_sr:
        return np.asarray(x, dtype=np.float32).copy()
    x, n_res, n_fix, win, delta, scale, inc, step, num_table = _setup(x, orig_sr, target_sr, filt)
    N, nwin = len(x), len(win)
    x64 = x.astype(np.float64)
    tr = time_register(n_res, inc, serial_register)
    n = tr.astype(np.int64)
    assert n[-1] < N
    frac = scale * (tr - n)
    y = np.zeros(n_res, dtype=acc_dtype)
    for wing in (0, 1):
        if wing:
            frac = scale - frac
        idx = frac * num_table
        off = idx.astype(np.int64)
        eta = idx - off
        count = np.minimum(n + 1 if wing == 0 else N - n - 1, (nwin - off) // step)
        for i in range(int(count.max())):
            m = np.flatnonzero(count > i)
            o = off[m] + i * step
            w = win[o] + eta[m] * delta[o]
            src = n[m] - i if wing == 0 else n[m] + i + 1
            y[m] = (y[m].astype(np.float64) + w * x64[src]).astype(acc_dtype)
    out = np.zeros(n_fix, dtype=np.float32)
    out[:n_res] = y.astype(np.float32)
    return out


def resample_literal(x, orig_sr, target_sr, filt=None):
    """The same, as resampy.interpn.resample_f writes it: one output at a time, one tap at a time."""
    if orig_sr == target_sr:
        return np.asarray(x, dtype=np.float32).copy()
    x, n_res, n_fix, win, delta, scale, inc, step, num_table = _setup(x, orig_sr, target_sr, filt)
    N, nwin = len(x), len(win)
    out = np.zeros(n_fix, dtype=np.float32)
    time_reg = 0.0
    for t in range(n_res):
        n = int(time_reg)
        y = np.float32(0.0)
        frac = scale * (time_reg - n)
        index_frac = frac * num_table
        offset = int(index_frac)
        eta = index_frac - offset
        for i in range(min(n + 1, (nwin - offset) // step)):
            weight = win[offset + i * step] + eta * delta[offset + i * step]
            y = np.float32(np.float64(y) + weight * np.float64(x[n - i]))
        frac = scale - frac
        index_frac = frac * num_table
        offset = int(index_frac)
        eta = index_frac - offset
        for k in range(min(N - n - 1, (nwin - offset) // step)):
            weight = win[offset + k * step] + eta * delta[offset + k * step]
            y = np.float32(np.float64(y) + weight * np.float64(x[n + k + 1]))
        out[t] = y
        time_reg += inc
    return out


def to_mono_f32(x):
    """librosa.load's conversion of [N, C] samples: float32, then to_mono's mean over the channels (float32
    sum in channel order, divided by C)."""
    x = np.asarray(x, dtype=np.float32)
    if x.ndim == 1:
        return x
    acc = x[:, 0].copy()
    for c in range(1, x.shape[1]):
        acc = acc + x[:, c]
    return acc / np.float32(x.shape[1])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
