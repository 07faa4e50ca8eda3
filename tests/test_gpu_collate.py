"""datasets.collate_fn against the reference's MyDataset.collate_fn (eval.npz, tests/golden/
make_golden_eval.py) on the four excerpts of example_1.wav, at r = 1, 2 and 5: the integer outputs, names
and stop targets exactly, the features within the analysis tests' tolerance, zero rows from each sentence's
zero frame on, and the same tuple whatever the order of the items."""
import ast

import numpy as np
import pytest
import torch

import eval_util as eu
from conftest import golden, load_pkg

pytestmark = pytest.mark.gpu
Z = golden("eval")


def _tol(ref):
    return 1e-5 * max(1.0, float(np.abs(ref).max()))  # test_gpu_audio_analysis.py's: float32 output


@pytest.fixture(scope="module")
def ap():
    return load_pkg("audio").AudioProcessor(**ast.literal_eval(str(Z["audio"])))


@pytest.fixture(scope="module")
def items():
    return eu.collate_items(golden("audio_example1")["pcm"])


@pytest.mark.parametrize("r", eu.RS)
def test_gpu_collate_vs_reference(ap, items, r):
    text, text_lengths, names, linear, mel, mel_lengths, stop_targets, idxs = load_pkg("datasets").collate_fn(items, ap, r)
    tpad = Z[f"stop_targets_r{r}"].shape[1]
    for t, key in ((text, "text"), (text_lengths, "text_lengths"), (mel_lengths, "mel_lengths")):
        assert t.dtype == torch.int64 and not t.is_cuda
        assert np.array_equal(t.numpy(), Z[f"{key}_r{r}"]), key
    assert names == Z[f"speaker_name_r{r}"].tolist() and idxs == Z[f"item_idxs_r{r}"].tolist()
    assert text_lengths.tolist() == sorted(text_lengths.tolist(), reverse=True)
    for t, n in ((linear, 1025), (mel, 80)):
        assert t.shape == (4, tpad, n) and t.dtype == torch.float32 and t.is_cuda and t.is_contiguous()
    assert stop_targets.shape == (4, tpad) and stop_targets.dtype == torch.float32 and stop_targets.is_cuda
    assert np.array_equal(stop_targets.cpu().numpy(), Z[f"stop_targets_r{r}"])
    for t, key in ((linear, "linear"), (mel, "mel")):
        ref = Z[key][:, :tpad]
        err = np.abs(t.cpu().numpy() - ref).max()
        print(f"r={r} {key}: max err {err:.3e} tol {_tol(ref):.3e}")
        assert err <= _tol(ref)
        for b, m in enumerate(mel_lengths.tolist()):
            assert not t[b, m - 1:].any(), (key, b)
            assert t[b, :m - 1].abs().sum(1).min() > 0


def test_gpu_collate_is_independent_of_item_order(ap, items):
    collate = load_pkg("datasets").collate_fn
    want = collate(items, ap, 2)
    got = collate([items[i] for i in (3, 1, 0, 2)], ap, 2)
    for w, g in zip(want, got):
        assert torch.equal(w, g) if torch.is_tensor(w) else w == g
