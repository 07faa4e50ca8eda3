"""CPU: the rbgen_* fixtures (the reference at batch 1 under location features, windowing and the
transition agent, tests/golden/make_golden_resident_batch_general.py) against the numpy oracle at
the fixtures' flags, with test_oracle_golden.py's checks, and the cap on the steps the argmax rule
leaves out (rbgen_util.py) recomputed from the fixtures.  Runs anywhere, no GPU."""
import numpy as np
import pytest

from conftest import golden, golden_flags, rel_rms, weights_mod
from oracle.tacotron2_oracle import Tacotron2Oracle
from rbgen_util import CONFIGS, KEYS, LENGTHS, assert_argmax, decided_steps, left_out_cap, rbgen, rbgen_file, rbgen_flags

SENTENCES = [(c, L) for c in CONFIGS for L in LENGTHS[c]]


@pytest.mark.parametrize("config,L", SENTENCES)
def test_rbgen_oracle_matches_reference(config, L):
    z = rbgen(config, L)
    fl = rbgen_flags(config)
    assert fl == golden_flags(golden(rbgen_file(config, L))) and fl["max_decoder_steps"] == 60
    sd = weights_mod().tacotron2_weights(0, location_attn=fl["location_attn"], trans_agent=fl["trans_agent"])
    o = Tacotron2Oracle(sd, dtype=np.float32, **fl)
    assert len(z["ids"]) == L and z["enc"].shape == (L, 512)
    assert rel_rms(o.encoder(z["ids"]), z["enc"]) < 1e-6
    mel, stop, align = o.decoder(z["enc"])
    # integer/index outputs: exact (the argmax at the steps the rule decides)
    assert mel.shape == z["mel"].shape, "frame count differs from the reference"
    assert_argmax(align, z["align"], f"{config} L={L}")
    np.testing.assert_array_equal(stop > 0.5, z["stop"] > 0.5)
    # float outputs: fp32 reference vs restatement
    assert rel_rms(mel, z["mel"]) < 1e-5
    assert np.abs(align - z["align"]).max() < 1e-5
    assert np.abs(stop - z["stop"]).max() < 1e-5
    assert rel_rms(o.postnet(z["mel"]), z["mel_post"]) < 1e-5


def test_rbgen_pool_layout_and_left_out_cap():
    """Every pool file holds its lengths in pool_fwdmask.npz's key scheme; frame counts are the
    runs' own (L = 2 stops by itself, the others run to the 60-step cap or just past it); no stop
    decision sits near 0.5; the argmax rule leaves out at most max(2, 1 %) steps of a sentence, and
    only under softmax."""
    for c in CONFIGS:
        files = sorted({rbgen_file(c, L) for L in LENGTHS[c]})
        assert sorted(int(L) for f in files for L in golden(f)["lengths"]) == sorted(LENGTHS[c])
        for f in files:
            z = golden(f)
            assert sorted(z.keys()) == sorted(["flags", "lengths"] + [f"{k}_L{int(L)}" for k in KEYS for L in z["lengths"]])
        for L in LENGTHS[c]:
            z = rbgen(c, L)
            T = z["mel"].shape[0]
            assert z["align"].shape == (T, L) and z["stop"].shape == (T,) and z["mel_post"].shape == z["mel"].shape
            assert T == 26 if L == 2 else 60 <= T <= 62
            assert np.abs(z["stop"] - 0.5).min() > 5e-3
            out = int((~decided_steps(z["align"])).sum())
            assert out <= left_out_cap(T) == 2
            if c != "loc_softmax":
                assert out == 0
