"""Batch-1 tts_synth_run with the caller's stream still busy (sentences issued back to back with
sync=False) runs the next sentence's encoder stage on the handle's own stream, beside the previous
sentence's postnet and Griffin-Lim, and hands over to the caller's stream with one event ahead of the
decoder (csrc/synth_api.hip: synth_stages).  Nothing may change: every overlapped call's frames and
waveform are, bit for bit, the same sentence run alone with sync=True on another handle.

Each pipelined call after the first is issued behind a short device-side delay queued on the
caller's stream (torch.cuda._sleep, about 1 ms of device time): the previous call's tail is still in
flight then in any case, so whether a call takes the front stream does not depend on how fast this
host reaches the next call.  All comparisons are exact equality."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import golden, golden_flags, load_pkg, weights_mod
from encoder_util import _env

LENGTHS = [5, 40, 12, 40, 5, 12]  # short -> long -> short: buffer reuse, Lmax changes
BUSY_CYCLES = 2_000_000


def _flags():
    return golden_flags(golden("t2_fwdmask_L100"))


def _model(num_speakers=0):
    t2 = load_pkg("tacotron2")
    fl = _flags()
    m = t2.Tacotron2(130, num_speakers, r=1, attn_win=fl["attn_win"], attn_norm=fl["attn_norm"],
                     forward_attn=fl["forward_attn"], trans_agent=fl["trans_agent"],
                     forward_attn_mask=fl["forward_attn_mask"], location_attn=fl["location_attn"])
    if num_speakers:
        m.load_state_dict({k: torch.from_numpy(v)
                           for k, v in weights_mod().tacotron2_weights(0, num_speakers=num_speakers).items()})
    return m.cuda().eval()


def _ready(m, ap):
    """Create the native handles now and wait for what their creation queued: the first synthesis call
    then finds the caller's stream idle, as a lone sentence does."""
    m._handles(max(LENGTHS), 1)
    ap._handle()
    torch.cuda.synchronize()


def _sentences():
    w = weights_mod()
    return [w.synthetic_ids(L, 700 + k) for k, L in enumerate(LENGTHS)]  # different ids in every call


@pytest.fixture(scope="module")
def ap(audio_cfg):
    return load_pkg("audio").AudioProcessor(**audio_cfg)


@pytest.fixture(scope="module")
def alone(ap):
    """Every sentence run alone (sync=True, idle stream) on a handle of its own: (frames, waveform)."""
    m = _model()
    _ready(m, ap)
    out = []
    for k, ids in enumerate(_sentences()):
        torch.cuda.synchronize()  # (the clone below is work on the caller's stream too)
        wav, frames = m.synthesize_native([ids], ap, seed=10 + k, sync=True)
        assert m.last_timing["encoder_front"] is False, "a lone sentence took the front stream"
        out.append((list(frames), wav.clone()))
    return out


@pytest.fixture(scope="module")
def piped():
    return _model()


def _pipelined(m, ap, sentences, seeds, speakers=None):
    """Back-to-back sync=False calls into buffers of their own; returns ([(frames, wav)], [front])."""
    bufs = [torch.empty(m.native_wav_capacity(ap, 1), dtype=torch.float64, device="cuda") for _ in sentences]
    _ready(m, ap)
    got, front = [], []
    for k, ids in enumerate(sentences):
        if k:
            torch.cuda._sleep(BUSY_CYCLES)  # the caller's stream is busy at entry, whatever the host's pace
        spk = None if speakers is None else [speakers[k]]
        wav, frames = m.synthesize_native([ids], ap, seed=seeds[k], sync=False, out=bufs[k], speaker_ids=spk)
        got.append((list(frames), wav))
        front.append(m.last_timing["encoder_front"])
    m.synth_sync()
    return got, front


def _same(got, want):
    for k, ((f, w), (rf, rw)) in enumerate(zip(got, want)):
        assert f == rf, (k, f, rf)
        assert w.shape == rw.shape and torch.equal(w, rw), k


@pytest.mark.gpu
def test_overlapped_calls_equal_one_at_a_time(piped, ap, alone):
    got, front = _pipelined(piped, ap, _sentences(), [10 + k for k in range(len(LENGTHS))])
    assert front == [False] + [True] * (len(LENGTHS) - 1), front
    _same(got, alone)
    t = piped.last_timing
    assert t["resident"] and t["encoder_resident"]
    assert t["encoder_placement_failures"] == 0 and t["encoder_timeouts"] == 0


@pytest.mark.gpu
def test_knob_off_equals_knob_on(piped, ap, alone):
    with _env(TTS_SYNTH_FRONT=0):
        got, front = _pipelined(piped, ap, _sentences(), [10 + k for k in range(len(LENGTHS))])
    assert front == [False] * len(LENGTHS), front
    _same(got, alone)


@pytest.mark.gpu
def test_speaker_embedding_overlapped(ap):
    w = weights_mod()
    sents = [w.synthetic_ids(12, 720), w.synthetic_ids(24, 721)]
    spk, seeds = [2, 1], [30, 31]
    ref_m = _model(4)
    _ready(ref_m, ap)
    want = []
    for k, ids in enumerate(sents):
        torch.cuda.synchronize()
        wav, frames = ref_m.synthesize_native([ids], ap, seed=seeds[k], sync=True, speaker_ids=[spk[k]])
        want.append((list(frames), wav.clone()))
    plain, _ = ref_m.synthesize_native([sents[1]], ap, seed=seeds[1], sync=True)
    assert not torch.equal(plain, want[1][1]), "the speaker embedding changed nothing"
    got, front = _pipelined(_model(4), ap, sents, seeds, speakers=spk)
    assert front == [False, True], front
    _same(got, want)


@pytest.mark.gpu
def test_failed_call_between_two_good_ones(piped, ap, alone):
    """An invalid call (a waveform buffer too small for the decoded sentence: rejected after the
    encoder stage went to the front stream and the decoder ran) leaves every stream of the handle
    drained, and the next call is correct."""
    n = load_pkg("_native")
    lib = n.lib()
    sents = _sentences()
    cap = piped.native_wav_capacity(ap, 1)
    bufs = [torch.empty(cap, dtype=torch.float64, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    w0, f0 = piped.synthesize_native([sents[1]], ap, seed=11, sync=False, out=bufs[0])
    hs = piped._synth[0]
    torch.cuda._sleep(BUSY_CYCLES)
    ids = np.ascontiguousarray(sents[2], dtype=np.int32)
    frames = (ctypes.c_int32 * 1)()
    st = lib.tts_synth_run(hs, ids.ctypes.data_as(n.I32P), n.i32_array([len(ids)]), 1, len(ids),
                           int(piped.decoder.max_decoder_steps), int(ap.griffin_lim_iters), 12,
                           ctypes.c_void_p(bufs[1].data_ptr()), 16, frames, n.stream_handle())
    assert st == 1, st  # TTS_ERR_INVALID
    assert b"wav buffer too small" in lib.tts_last_error()
    front, busy = ctypes.c_int(-1), ctypes.c_int(-1)
    n.check(lib.tts_synth_state(hs, ctypes.byref(front), ctypes.byref(busy)), "tts_synth_state")
    assert front.value == 1, "the failed call's encoder stage did not take the front stream"
    assert busy.value == 0 and torch.cuda.current_stream().query(), "the failed call left work in flight"
    w2, f2 = piped.synthesize_native([sents[3]], ap, seed=13, sync=False, out=bufs[2])
    assert piped.last_timing["encoder_front"] is False  # every stream was drained: today's run
    piped.synth_sync()
    _same([(list(f0), w0), (list(f2), w2)], [alone[1], alone[3]])


def test_encoder_placement_retries():
    """The rule encoder_pending_status applies to a resident batch-1 launch's status word, driven with
    synthetic words (host arithmetic, no device): one placement failure keeps the resident form, the
    configured number in a row (the decoder's RES_PLACEMENT_RETRIES = 3) drops it; a clean run in
    between starts the row again; a timed-out wait changes nothing, another launch's word is no failure."""
    lib = load_pkg("_native").load_library()
    OK, PLACEMENT, TIMEOUT = 0, 1, 2
    fails, res, out = ctypes.c_int(0), ctypes.c_int(1), ctypes.c_int(-1)

    def rule(code, salt, word_salt=None):
        word = ((salt if word_salt is None else word_salt) << 8) | code
        assert lib.tts_encoder_status_rule(word, salt, ctypes.byref(fails), ctypes.byref(res), ctypes.byref(out)) == 0
        return out.value, fails.value, res.value

    assert rule(50, 7) == (PLACEMENT, 1, 1)  # one uneven dispatch: still resident
    assert rule(50, 8) == (PLACEMENT, 2, 1)
    assert rule(0, 9) == (OK, 0, 1)  # a clean run ends the row
    assert rule(50, 10) == (PLACEMENT, 1, 1)
    assert rule(1, 11) == (TIMEOUT, 1, 1)  # a timeout neither counts nor clears
    assert rule(50, 12, word_salt=11) == (OK, 0, 1)  # an earlier launch's word is no failure of this one
    assert rule(50, 13) == (PLACEMENT, 1, 1)
    assert rule(50, 14) == (PLACEMENT, 2, 1)
    assert rule(50, 0x3FFFF) == (PLACEMENT, 3, 0)  # three in a row: the handle gives the form up
