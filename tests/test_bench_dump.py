"""CPU: bench.py's timed region runs exactly --steps steps after --warmup, and --dump-outputs'
writer (dump_outputs) keeps each sentence's finished part, stays inside its byte budget with a
fixed sample, and writes the same files for the same inputs."""
import argparse
import os

import numpy as np
import pytest
import torch

import conftest  # noqa: F401  (puts the repository root on sys.path)
import bench

HOP = 275


def _wav(frames):
    """[B, hop*(Fmax-1)] float64 rows holding their own flat position; -1 past each sentence's end."""
    n = HOP * (max(frames) - 1)
    w = torch.full((len(frames), n), -1.0, dtype=torch.float64)
    for k, T in enumerate(frames):
        w[k, :HOP * (T - 1)] = torch.arange(HOP * (T - 1), dtype=torch.float64) + 1e6 * k
    return w


def _size(d):
    return sum(os.path.getsize(os.path.join(d, n)) for n in os.listdir(d))


def test_timed_region_runs_exactly_steps_after_warmup():
    seeds = []

    def step(seed):
        seeds.append(seed)
        return [222]

    args = argparse.Namespace(steps=3, warmup=2)
    tm = bench.timed_region(step, args, 1, torch.device("cpu"), HOP, 22050)
    assert seeds == [0, 1, 1000, 1001, 1002]
    assert tm["frames_per_step"] == 222
    assert tm["ms_per_step"] == pytest.approx(1000.0 * tm["elapsed"] / 3, rel=1e-12)
    assert tm["value"] == pytest.approx(222 * 3 / tm["elapsed"], rel=1e-12)


def test_dump_outputs_keeps_each_sentences_finished_part(tmp_path):
    frames = [3, 7, 5]
    d = str(tmp_path / "a")
    bench.dump_outputs(d, frames, _wav(frames), HOP)
    assert sorted(os.listdir(d)) == ["frames.npy", "wav.npy"]
    f, w = np.load(os.path.join(d, "frames.npy")), np.load(os.path.join(d, "wav.npy"))
    assert f.dtype == np.float64 and w.dtype == np.float64
    assert f.tolist() == [3.0, 7.0, 5.0]
    want = np.concatenate([np.arange(HOP * (T - 1), dtype=np.float64) + 1e6 * k for k, T in enumerate(frames)])
    assert np.array_equal(w, want)  # nothing of the padding (-1), nothing dropped below the budget


def test_dump_outputs_samples_inside_the_budget_and_repeats(tmp_path, monkeypatch):
    budget = 16384
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", budget)
    frames = [9, 12, 4, 12]
    wav = _wav(frames)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, frames, wav, HOP)
    bench.dump_outputs(b, frames, wav.clone(), HOP)
    assert _size(a) <= budget and _size(b) <= budget
    for n in ("frames.npy", "wav.npy"):
        assert open(os.path.join(a, n), "rb").read() == open(os.path.join(b, n), "rb").read()
    w = np.load(os.path.join(a, "wav.npy"))
    full = np.concatenate([np.arange(HOP * (T - 1), dtype=np.float64) + 1e6 * k for k, T in enumerate(frames)])
    assert w.dtype == np.float64 and 0 < w.size < full.size
    assert w.size * 8 > budget // 2  # a sample that uses the budget, not a token one
    assert (np.diff(w) > 0).all() and np.isin(w, full).all()  # distinct positions of the output, in order
