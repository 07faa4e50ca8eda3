"""GPU: the persistent Griffin-Lim loop's gather (csrc/griffin_lim.hip, gl_persistent_body), bitwise
against the non-persistent fused per-iteration loop (TTS_RESIDENT=0) on the same processor
configuration, mel and phases.  Written for a gather that takes the workgroup's own frame from a
copy its store leaves in the gather buffer (measured slower and dropped); the
cases hold for any form of the gather, the present one included.

- edge frames, F = 6, 10, 12 at 1, 2 and 3 iterations: every frame is an edge frame with
  reflection and few frames have all nine contributors; the iterations end on either granule-slot
  parity;
- F = 40, 5 iterations: frames on either side of an XCD run boundary;
- F = 257, 3 iterations: the smallest grid of the two-workgroups-per-CU form;
- an injected drop at F = 12 (TTS_GL_INJECT_DROP): a dropped neighbour must end in the timeout
  status and an error, never in a stale-but-accepted sum.
"""
import numpy as np
import pytest
import torch

from conftest import load_pkg
from encoder_util import _env

pytestmark = pytest.mark.gpu


def _inputs(F, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    mel = torch.from_numpy(rng.uniform(0, 1, size=(1, F, 80)).astype(np.float32)).cuda()
    return mel, rng.uniform(0, 1, size=(1, 1025, F))


def _both(audio_cfg, F, iters):
    ap = load_pkg("audio").AudioProcessor(**{**audio_cfg, "griffin_lim_iters": iters})
    mel, pu = _inputs(F, 1000 * iters + F)
    wav = ap.griffin_lim_batch(mel, [F], phase_u=pu).cpu()
    assert ap.last_gl_path() == "persistent"
    with _env(TTS_RESIDENT=0):
        fused = ap.griffin_lim_batch(mel, [F], phase_u=pu).cpu()
        assert ap.last_gl_path() != "persistent"
    assert torch.isfinite(wav).all()
    return wav, fused


@pytest.mark.parametrize("iters", [1, 2, 3])
@pytest.mark.parametrize("F", [6, 10, 12])
def test_edge_frames_bitwise_vs_fused(audio_cfg, F, iters):
    wav, fused = _both(audio_cfg, F, iters)
    assert torch.equal(wav, fused)


def test_xcd_run_boundary_bitwise_vs_fused(audio_cfg):
    wav, fused = _both(audio_cfg, 40, 5)
    assert torch.equal(wav, fused)


def test_two_per_cu_smallest_grid_bitwise_vs_fused(audio_cfg):
    wav, fused = _both(audio_cfg, 257, 3)
    assert torch.equal(wav, fused)


def test_injected_drop_times_out_and_poisons(audio_cfg):
    """Frame 3 stops storing after its first iteration: its neighbours' waits time out (a status
    path, not a fault); the error surfaces and the same handle then works again."""
    audio = load_pkg("audio")
    with _env(TTS_GL_WAIT_TICKS=20000):  # 0.2 ms per wait at the 100 MHz wall clock
        ap = audio.AudioProcessor(**{**audio_cfg, "griffin_lim_iters": 4})
        mel, pu = _inputs(12, 5)
        good = ap.griffin_lim_batch(mel, [12], phase_u=pu)
        assert ap.last_gl_path() == "persistent" and torch.isfinite(good).all()
        with _env(TTS_GL_INJECT_DROP=3):
            with pytest.raises(RuntimeError, match="timed out"):
                ap.griffin_lim_batch(mel, [12], phase_u=pu)
        again = ap.griffin_lim_batch(mel, [12], phase_u=pu)
        assert torch.equal(again, good)
