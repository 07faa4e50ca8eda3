"""CPU: the host half of the evaluation path against the reference's own outputs (eval.npz,
tests/golden/make_golden_eval.py): eval_util's float64 restatement of the five losses (what the GPU tests
of evaluate_batch compare with), prepare_* / sequence_mask / collate_plan, and the no-GPU behaviour."""
import numpy as np
import pytest
import torch

import eval_util as eu
from conftest import golden, load_pkg

Z = golden("eval")
ELEMENTWISE = [(case, kind, name) for case, (_, _, lengths) in eu.LOSS_CASES.items() for kind in ("l1", "mse")
               for name in (("plain", "masked") if lengths is not None else ("plain",))]


def test_fixture_is_the_issues():
    for r, tpad, sums in ((1, 9, [1, 3, 4, 6]), (2, 10, [2, 4, 5, 7]), (5, 10, [2, 4, 5, 7])):
        assert Z[f"order_r{r}"].tolist() == [1, 2, 0, 3]
        assert Z[f"mel_lengths_r{r}"].tolist() == [9, 7, 6, 4]
        assert Z[f"stop_targets_r{r}"].shape == (4, tpad)
        assert Z[f"stop_targets_r{r}"].sum(1).tolist() == sums
    assert Z["mel"].shape == (4, 10, 80) and Z["linear"].shape == (4, 10, 1025)


@pytest.mark.parametrize("case,kind,name", ELEMENTWISE)
def test_restated_elementwise_losses(case, kind, name):
    x, y, lengths = eu.loss_inputs(case)
    loss, count, per = eu.elementwise_loss(kind, x, y, lengths if name == "masked" else None)
    key = f"{case}_{kind}_{name}"
    assert count == int(Z[key + "_count"])
    print(f"{key}: {loss!r} vs {float(Z[key + '_64'])!r}, bound {eu.fp64_bound(count):.3e} relative")
    assert eu.within(loss, float(Z[key + "_64"]), count)
    for b, (got, ref) in enumerate(zip(per, Z[key + "_per"])):
        assert eu.within(got, ref, eu.sentence_terms(x.shape, lengths if name == "masked" else None, b)), b


def test_restated_bce():
    loss, n = eu.bce_with_logits(*eu.bce_inputs())
    assert n == int(Z["e_bce_count"]) == 257
    assert np.isfinite(loss) and eu.within(loss, float(Z["e_bce_64"]), n)


@pytest.mark.parametrize("r", eu.RS)
def test_restated_stop_target_grouping(r):
    assert np.array_equal(eu.group_stop_targets(Z[f"stop_targets_r{r}"], r), Z[f"stop_grouped_r{r}"])
    ev = load_pkg("evaluate")
    got = ev.group_stop_targets(torch.from_numpy(Z[f"stop_targets_r{r}"]), r)
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), Z[f"stop_grouped_r{r}"])


@pytest.mark.parametrize("r", eu.RS)
def test_collate_plan(r):
    ds = load_pkg("datasets")
    order, frames, tpad, mel_lengths = ds.collate_plan([L for _, _, L in eu.ITEMS], [n for _, n, _ in eu.ITEMS], 275, r)
    assert order == Z[f"order_r{r}"].tolist()
    assert mel_lengths == Z[f"mel_lengths_r{r}"].tolist() and frames == [m - 1 for m in mel_lengths]
    assert tpad == Z[f"stop_targets_r{r}"].shape[1]


def test_collate_plan_sort_is_stable():
    ds = load_pkg("datasets")
    order, frames, tpad, mel_lengths = ds.collate_plan([3, 7, 3, 7, 5], [275, 550, 825, 1100, 10], 275, 4)
    assert order == [1, 3, 4, 0, 2] and frames == [3, 5, 1, 2, 4] and tpad == 8 and mel_lengths == [4, 6, 2, 3, 5]


@pytest.mark.parametrize("r", eu.RS)
def test_prepare_helpers(r):
    d = load_pkg("data")
    order = Z[f"order_r{r}"].tolist()
    items = eu.collate_items(golden("audio_example1")["pcm"])
    text = d.prepare_data([items[i]["text"] for i in order]).astype(np.int32)
    assert np.array_equal(text, Z[f"text_r{r}"])
    assert [len(items[i]["text"]) for i in order] == Z[f"text_lengths_r{r}"].tolist()
    frames = [int(m) - 1 for m in Z[f"mel_lengths_r{r}"]]
    stop = d.prepare_stop_target([np.array([0.] * f) for f in frames], r)
    assert np.array_equal(stop, Z[f"stop_targets_r{r}"])
    tpad = stop.shape[1]
    # the features of the fixture, cut back to each sentence's frames, padded again
    for k, n in (("mel", 80), ("linear", 1025)):
        feats = [Z[k][b, :frames[b]].T for b in range(4)]
        assert np.array_equal(d.prepare_tensor(feats, r).transpose(0, 2, 1), Z[k][:, :tpad])
    assert d.pad_per_step(np.ones((2, 3, 4)), 2).shape == (2, 3, 6)


def test_sequence_mask():
    gu = load_pkg("generic_utils")
    m = gu.sequence_mask(torch.LongTensor([3, 0, 5]), max_len=4)
    assert m.dtype == torch.bool
    assert m.tolist() == [[True, True, True, False], [False] * 4, [True] * 4]
    assert gu.sequence_mask(torch.LongTensor([2, 1])).tolist() == [[True, True], [True, False]]


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_losses_have_no_cpu_fallback():
    lo = load_pkg("losses")
    x = torch.zeros(2, 3, 4)
    for cls in (lo.L1LossMasked, lo.MSELossMasked):
        with pytest.raises(RuntimeError, match="no GPU"):
            cls()(x, x, [3, 3])
    for cls in (lo.L1Loss, lo.MSELoss, lo.BCEWithLogitsLoss):
        with pytest.raises(RuntimeError, match="no GPU"):
            cls()(x, x)
    ds = load_pkg("datasets")
    ap = load_pkg("audio").AudioProcessor(**load_pkg("generic_utils").default_config()["audio"])
    with pytest.raises(RuntimeError, match="no GPU"):
        ds.collate_fn(eu.collate_items(golden("audio_example1")["pcm"]), ap, 1)
