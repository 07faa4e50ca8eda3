"""Generate tests/golden/eval.npz by running the REFERENCE collate_fn and loss modules.

Run in the build container only (needs /root/reference; nothing here runs on the GPU box):

    python tests/golden/make_golden_eval.py

Built as make_golden_audio_analysis.py is: the reference's own ``AudioProcessor`` with ``librosa`` replaced
by the oracle's librosa-0.6.2 restatement and the audio block of ``tests/test_config.json``.
``collections.Mapping`` (gone from Python 3.10) is pointed at ``collections.abc.Mapping`` so that
``MyDataset.collate_fn`` (datasets/TTSDataset.py:167-228) runs as it stands.

Collate part: ``collate_fn`` on an instance made with ``object.__new__`` (``ap`` and ``outputs_per_step``
set), on the four items of tests/eval_util.py (float32 excerpts of tests/inputs/example_1.wav), at r = 1, 2
and 5.  Per r: text, text_lengths, mel_lengths, stop_targets, speaker names, item idxs, and the grouped stop
targets of train.py:306-309 (case f).  ``mel`` and ``linear`` once, at r = 5; the r = 1 arrays are their
first 9 rows (asserted).

Loss part: ``L1LossMasked``, ``MSELossMasked`` (layers/losses.py), ``nn.L1Loss``, ``nn.MSELoss`` and
``nn.BCEWithLogitsLoss`` on the seeded inputs of tests/eval_util.py, once in float32 and once with the
tensors cast to float64; per case the two values, the number of terms and the per-sentence float64 sums.
Only seeds (in eval_util.py) and results are stored.
"""
from __future__ import annotations

import collections
import collections.abc
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402  (the stubs, REF)
import eval_util as eu  # noqa: E402  (the inputs)


def collate_part(out):
    import scipy.io.wavfile
    from datasets.TTSDataset import MyDataset
    from utils.audio import AudioProcessor
    txt = open(os.path.join(mg.REF, "tests", "test_config.json")).read()
    conf = json.loads(re.sub(r"//[^\n]*", "", txt))  # the reference's load_config strips // comments
    sr, pcm = scipy.io.wavfile.read(os.path.join(mg.REF, "tests", "inputs", "example_1.wav"))
    assert pcm.dtype == np.int16 and sr == conf["audio"]["sample_rate"]
    assert np.array_equal(pcm, np.load(os.path.join(HERE, "audio_example1.npz"))["pcm"])
    ap = AudioProcessor(**conf["audio"])
    assert ap.hop_length == 275
    out["audio"] = np.array(repr(conf["audio"]))
    items = eu.collate_items(pcm)
    for d in items:  # float32 in, as load_data hands it over: the float64 cast changes nothing
        assert np.array_equal(ap.melspectrogram(d["wav"]), ap.melspectrogram(d["wav"].astype(np.float64)))
    feats = {}
    for r in eu.RS:
        ds = object.__new__(MyDataset)
        ds.ap, ds.outputs_per_step = ap, r
        text, text_lengths, names, linear, mel, mel_lengths, stop_targets, idxs = ds.collate_fn(items)
        order = [[d["item_idx"] for d in items].index(i) for i in idxs]
        out[f"order_r{r}"] = np.array(order)
        out[f"text_r{r}"], out[f"text_lengths_r{r}"] = text.numpy(), text_lengths.numpy()
        out[f"mel_lengths_r{r}"], out[f"stop_targets_r{r}"] = mel_lengths.numpy(), stop_targets.numpy()
        out[f"speaker_name_r{r}"], out[f"item_idxs_r{r}"] = np.array(names), np.array(idxs)
        # case (f), train.py:306-309 as written there
        st = stop_targets.view(text.shape[0], stop_targets.size(1) // r, -1)
        out[f"stop_grouped_r{r}"] = (st.sum(2) > 0.0).unsqueeze(2).float().squeeze(2).numpy()
        feats[r] = (mel.numpy(), linear.numpy())
        print(f"r={r}: order {order} mel_lengths {mel_lengths.tolist()} Tpad {mel.shape[1]} "
              f"stop row sums {stop_targets.sum(1).tolist()} mel {tuple(mel.shape)} linear {tuple(linear.shape)}")
        assert mel.dtype == linear.dtype == stop_targets.dtype == __import__("torch").float32
    out["mel"], out["linear"] = feats[5]
    for k in (0, 1):
        assert np.array_equal(feats[1][k], feats[5][k][:, :9]) and not feats[5][k][:, 9:].any()
        assert np.array_equal(feats[2][k], feats[5][k])


def loss_part(out):
    import torch
    from torch import nn
    from torch.nn import functional
    from layers.losses import L1LossMasked, MSELossMasked
    from utils.generic_utils import sequence_mask
    masked = dict(l1=L1LossMasked(), mse=MSELossMasked())
    plain = dict(l1=nn.L1Loss(), mse=nn.MSELoss())
    for case in eu.LOSS_CASES:
        x, y, lengths = eu.loss_inputs(case)
        x, y = torch.from_numpy(x), torch.from_numpy(y)
        for kind in ("l1", "mse"):
            runs = [("plain", lambda a, b: plain[kind](a, b), None)]
            if lengths is not None:
                runs.append(("masked", lambda a, b: masked[kind](a, b, torch.LongTensor(lengths)), lengths))
            for name, fn, lens in runs:
                v32, v64 = fn(x.clone(), y.clone()), fn(x.double(), y.double())
                assert v32.dtype == torch.float32 and v64.dtype == torch.float64
                # per sentence: the reference's own expression (layers/losses.py:27-31) on that sentence, float64
                L = torch.LongTensor(lens if lens is not None else [x.shape[1]] * x.shape[0])
                mask = sequence_mask(sequence_length=L, max_len=x.size(1)).unsqueeze(2).double().expand_as(x)
                f = functional.l1_loss if kind == "l1" else functional.mse_loss
                per = np.array([f(x[b].double() * mask[b], y[b].double() * mask[b], reduction="sum").item()
                                for b in range(x.shape[0])])
                count = int(mask.sum().item())
                key = f"{case}_{kind}_{name}"
                out[key + "_32"], out[key + "_64"] = np.float32(v32.item()), np.float64(v64.item())
                out[key + "_count"], out[key + "_per"] = np.int64(count), per
                print(f"{key}: f32 {v32.item():.9g} f64 {v64.item():.17g} terms {count}")
    x, y = (torch.from_numpy(v) for v in eu.bce_inputs())
    v32, v64 = nn.BCEWithLogitsLoss()(x, y), nn.BCEWithLogitsLoss()(x.double(), y.double())
    out["e_bce_32"], out["e_bce_64"], out["e_bce_count"] = np.float32(v32.item()), np.float64(v64.item()), np.int64(len(x))
    print(f"e_bce: f32 {v32.item():.9g} f64 {v64.item():.17g}")
    assert np.isfinite(v32.item()) and np.isfinite(v64.item())


def main():
    collections.Mapping = collections.abc.Mapping
    mg._stub_text_deps()
    mg._stub_audio_deps()
    sys.path.insert(0, mg.REF)
    out = {}
    collate_part(out)
    loss_part(out)
    path = os.path.join(HERE, "eval.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
