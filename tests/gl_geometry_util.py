"""Shared by test_gl_geometry_cpu.py and test_gpu_gl_geometry.py: the STFT geometries (hop / win pairs)
the Griffin-Lim and analysis kernels are run at, the inputs, a second restatement of STFT / iSTFT built
from the definition (the oracle's fixtures from the reference exist at 275 / 1102 only: this is what
anchors oracle/griffin_lim_oracle.py at the other geometries), two seeded mistakes of the oracle that the
tests must be able to see, and the host predicates of csrc/griffin_lim.hip that choose the iteration
loop (gl_fused_path, contrib_symmetric, gather_fits), restated so that the expected loop of a run is
derived and not measured."""
import contextlib

import numpy as np

import oracle.griffin_lim_oracle as glo

NFFT = 2048
NB = NFFT // 2 + 1
# csrc/griffin_lim.hip
OLA_MAX, GL_DMAX, GL_PAIRS, GL_THREADS = 5, 4, 9, 256
GL_SLOTS = 2 * GL_DMAX + 1

# name: (sample_rate, frame_shift_ms, frame_length_ms, hop, win); hop / win are asserted, not used to build
GEOMETRIES = {
    "de16k": (16000, 12.5, 50, 200, 800),       # reference config; even woff 624 > 512; winp == win
    "best20k": (20000, 12.5, 50, 250, 1000),    # reference config
    "kusal22k": (22000, 12.5, 50, 275, 1100),   # reference config; win / hop exactly 4
    "libri24k": (24000, 12.5, 50, 300, 1200),   # reference config; 2250 of the 2304 gather pairs
    "r45_fit": (16000, 12.5, 56.25, 200, 900),  # ceil(win / hop) 5 with a heavy fifth contributor
    "r45_big": (16000, 16, 72, 256, 1152),      # ceil 5; the persistent gather fits for F <= 6 only
    "oddwin": (22020, 12.5, 50, 275, 1101),     # odd win: fb = woff - 1, winp 1104
    "oddhop": (22050, 12.6, 50, 277, 1102),     # odd hop
    "full": (16000, 32, 128, 512, 2048),        # woff 0: the window fills the FFT
    "half": (16000, 32, 64, 512, 1024),         # ceil 2
    "sixth": (16000, 12.5, 75, 200, 1200),      # ceil 6 > OLA_MAX: generic overlap-add, never fused
    "eighth": (16000, 8, 64, 128, 1024),        # ceil 8 > OLA_MAX
}
NAMES = list(GEOMETRIES)
REFERENCE_CONFIGS = ["de16k", "best20k", "kusal22k", "libri24k"]
# the persistent loop's two host conditions (contrib_symmetric, gather_fits below) hold at every F
PERSISTENT = ["r45_fit", "oddwin", "oddhop"]
# last Fmax the persistent loop takes: the contributor relation is not symmetric beyond it (win = 2 k hop:
# an edge frame reads a frame that does not read it back), or the gather layout does not fit
LAST_PERSISTENT_F = {"de16k": 5, "best20k": 5, "kusal22k": 5, "libri24k": 5, "r45_big": 6, "full": 3, "half": 3}
UNFUSED_ONLY = ["sixth", "eighth"]

SHORT = [2, 3, 5, 12, 40]  # every STFT frame is reflected at both ends at 2, 3 and 5
BATCHED = SHORT + [210]    # B * Fmax = 1260 > 1024: the unfused loop
# hop * (F - 1) exactly 4096 and 8192: the de-emphasis scan's chunk edges
SCAN_EDGE = {256: [17, 33], 512: [9, 17]}


def audio_kwargs(audio_cfg, name, **over):
    sr, shift, length, _, _ = GEOMETRIES[name]
    return {**audio_cfg, "sample_rate": sr, "frame_shift_ms": shift, "frame_length_ms": length,
            "mel_fmax": min(8000, sr / 2), **over}


def hop_win(name):
    return GEOMETRIES[name][3], GEOMETRIES[name][4]


def frame_counts(name, batched):
    hop, _ = hop_win(name)
    return (BATCHED if batched else SHORT) + SCAN_EDGE.get(hop, [])


def gl_inputs(Fs, seed, n_in=80):
    """Seeded uniform(0, 1) spectrogram [B, Fmax, n_in] float32 and phases [B, 1025, Fmax] float64 of a
    ragged batch, zero beyond each sentence's frames."""
    rng = np.random.Generator(np.random.PCG64(seed))
    Fmax = max(Fs)
    spec = np.zeros((len(Fs), Fmax, n_in), np.float32)
    pu = np.zeros((len(Fs), NB, Fmax))
    for b, F in enumerate(Fs):
        spec[b, :F] = rng.uniform(0, 1, size=(F, n_in))
        pu[b, :, :F] = rng.uniform(0, 1, size=(NB, F))
    return spec, pu


def chirp_noise(n, seed):
    """Seeded noise plus a linear chirp from 0.01 to 0.21 cycles per sample, |x| < 0.1 (no spectrogram bin
    reaches the normalisation's clip)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(n) / n
    return 0.03 * rng.standard_normal(n).clip(-2.5, 2.5) / 2.5 + 0.05 * np.sin(2 * np.pi * n * (0.01 * t + 0.1 * t * t))


# ---------------------------------------------------------------- STFT / iSTFT from the definition
def direct_window(win):
    """The periodic Hann of win samples at lpad = (n_fft - win) // 2 of an n_fft buffer."""
    w = np.zeros(NFFT)
    lpad = (NFFT - win) // 2
    for n in range(win):
        w[lpad + n] = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / win)
    return w


def direct_stft(y, hop, win):
    """Centred STFT: frame t holds y (reflected about its first and last sample) at t hop - 1024 .. + 1023,
    times the window, through np.fft.rfft; complex64 [1025, 1 + len(y) // hop]."""
    y = np.asarray(y, np.float64)
    N = len(y)
    w = direct_window(win)
    T = 1 + N // hop
    out = np.empty((NB, T), np.complex64)
    n = np.arange(NFFT)
    for t in range(T):
        p = t * hop - NFFT // 2 + n
        while (p < 0).any() or (p > N - 1).any():        # short signals fold more than once
            p = np.abs(p)                                # reflection about sample 0
            p = np.where(p > N - 1, 2 * (N - 1) - p, p)  # ... and about sample N - 1
        out[:, t] = np.fft.rfft(w * y[p])
    return out


def direct_istft(S, hop, win):
    """Inverse of direct_stft as librosa 0.6.2 orders it: each frame's inverse real FFT times the window,
    added frame by frame into a float32 signal; the squared window added frame by frame into a float32
    sum-square; the quotient where the sum-square is above float32 tiny; n_fft / 2 cut from both ends."""
    T = S.shape[1]
    w = direct_window(win)
    w2 = w * w
    y = np.zeros(NFFT + hop * (T - 1), np.float32)
    ss = np.zeros_like(y)
    for t in range(T):
        fr = w * np.fft.irfft(S[:, t].astype(np.complex128), NFFT)
        y[t * hop:t * hop + NFFT] += fr
        ss[t * hop:t * hop + NFFT] += w2
    ok = ss > np.finfo(np.float32).tiny
    y[ok] = y[ok] / ss[ok]
    return y[NFFT // 2:len(y) - NFFT // 2]


# ---------------------------------------------------------------- seeded mistakes of the oracle
@contextlib.contextmanager
def mistake(kind, hop):
    """The oracle with a wrong window, in stft, istft and the window sum-square alike.
    "truncate": the window's samples from 4 * hop on are zero (a sample's fifth overlap-add contributor
    is lost in the frames and in the sum-square).  "roll": the padded window is rolled by one sample."""
    hann, pad = glo.hann_periodic, glo.pad_center

    def hann_truncated(n):
        w = hann(n)
        w[4 * hop:] = 0.0
        return w

    try:
        if kind == "truncate":
            glo.hann_periodic = hann_truncated
        elif kind == "roll":
            glo.pad_center = lambda w, size: np.roll(pad(w, size), 1)
        else:
            raise ValueError(kind)
        yield
    finally:
        glo.hann_periodic, glo.pad_center = hann, pad


# ---------------------------------------------------------------- the host's loop predicates, restated
def _geo(hop, win):
    woff = (NFFT - win) // 2
    fb = woff & ~1
    return woff, fb, (win + (woff - fb) + 3) // 4 * 4


def fused_geometry(hop, win):
    """gl_fused_path's geometry half: at most OLA_MAX overlap-add contributors per sample."""
    return (win + hop - 1) // hop <= OLA_MAX


def _contributors(hop, win, f, F):
    """for_contributors: (q, ilo, ihi) arrays over the samples of frame f's window whose reflected,
    untrimmed position q is at or beyond woff; the contributors of a sample are frames ilo .. ihi."""
    woff, _, _ = _geo(hop, win)
    N = hop * (F - 1)
    p = f * hop + np.arange(woff, woff + win) - NFFT // 2
    if N == 1:
        r = np.zeros_like(p)
    else:
        period = 2 * (N - 1)
        pp = np.mod(p, period)
        r = np.where(pp < N, pp, period - pp)
    q = r + NFFT // 2
    q = q[q >= woff]
    raw = q - woff - win + 1
    ilo = np.where(raw <= 0, 0, (raw + hop - 1) // hop)
    ihi = np.minimum((q - woff) // hop, F - 1)
    return q, ilo, ihi


def contrib_symmetric(hop, win, F):
    """contrib_symmetric, every pair of frames: frame f reads frame fi exactly when fi reads f."""
    c = np.zeros((F, F), bool)
    for f in range(F):
        _, ilo, ihi = _contributors(hop, win, f, F)
        for lo, hi in set(zip(ilo.tolist(), ihi.tolist())):
            c[f, lo:hi + 1] = True
    return bool((c == c.T).all())


def gather_fits(hop, win, F):
    """gather_fits: every contributor of every frame within GL_DMAX frames and OLA_MAX of the sample's
    first, and at most GL_PAIRS * GL_THREADS granule pairs per frame."""
    woff, fb, _ = _geo(hop, win)
    N = hop * (F - 1)

    def frame_ok(f):
        q, ilo, ihi = _contributors(hop, win, f, F)
        if (ihi - ilo >= OLA_MAX).any():
            return False
        lo, hi = {}, {}
        for k in range(OLA_MAX):
            fi = ilo + k
            m = fi <= ihi
            if not m.any():
                continue
            sl = fi[m] - f + GL_DMAX
            if sl.min() < 0 or sl.max() >= GL_SLOTS:
                return False
            off = q[m] - fi[m] * hop - fb
            for s in np.unique(sl):
                o = off[sl == s]
                lo[s] = min(lo.get(s, 1 << 30), int(o.min()))
                hi[s] = max(hi.get(s, -1), int(o.max()))
        pairs = sum((hi[s] - (lo[s] & ~1)) // 2 + 1 for s in hi)
        return pairs <= GL_PAIRS * GL_THREADS

    interior_done = False
    for f in range(F):
        edge = f * hop + woff - NFFT // 2 < 0 or f * hop + woff + win - 1 - NFFT // 2 >= N
        if not edge and interior_done:
            continue
        if not frame_ok(f):
            return False
        if not edge:
            interior_done = True
    return True


def persistent_geometry(hop, win, Fmax):
    """gl_persistent_path's geometry half for a batch whose longest sentence has Fmax frames."""
    if not fused_geometry(hop, win):
        return False
    return all(contrib_symmetric(hop, win, F) and gather_fits(hop, win, F) for F in range(2, Fmax + 1))


def expected_path(name, Fs, resident=True, forced_fused=False, iters=3):
    """The loop tts_gl_last_path reports for a batch of these frame counts on a 256-CU device.  The
    persistent launch's grid is B x Fmax workgroups, at most two per compute unit: a larger grid is not
    placed (launch_persistent) and the fused loop takes the iterations."""
    hop, win = hop_win(name)
    B, Fmax = len(Fs), max(Fs)
    if not (fused_geometry(hop, win) and (B * Fmax <= 1024 or forced_fused)):
        return "unfused"
    if resident and iters > 0 and sum(Fs) <= 512 and B * Fmax <= 512 and persistent_geometry(hop, win, Fmax):
        return "persistent"
    return "fused"
