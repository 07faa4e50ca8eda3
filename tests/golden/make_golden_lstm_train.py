"""Generate tests/golden/lstm_train.npz by running the REFERENCE encoder's LSTM with autograd.

Run in the build container only (needs /root/reference; nothing here runs on the GPU box):

    python tests/golden/make_golden_lstm_train.py

Built as make_golden_loss_grad.py is: make_golden's stubs, then ``layers.tacotron2.Encoder`` from the reference.
Its ``.lstm`` (rebuilt with the case's sizes where they are not 512 / 256 / bidirectional) gets the seeded weights
of tests/lstm_train_util.py and runs as ``Encoder.forward`` runs it (layers/tacotron2.py:68-75:
``pack_padded_sequence`` -> lstm -> ``pad_packed_sequence``; ``enforce_sorted=False`` for the unsorted cases), then
``(out * upstream).sum().backward()``, once in float32 and once with ``.double()``.  Stored per case and
precision: out, h_n, c_n, grad_x and the parameter gradients, tensors above ``SAMPLE`` elements at the seeded
index sample of ``lstm_train_util.sample_indices``.  Only seeds (in lstm_train_util.py) and results are stored.

Also writes the reference's own float32-against-float64 error per case and tensor, in the bound's form, into
the "reference_fp32" section of profiles/lstm_train.json (the other sections are left as they are).
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402  (the stubs, REF)
import lstm_train_util as lu  # noqa: E402


def run_reference(Encoder, case, dtype):
    import torch
    from torch import nn
    c = lu.CASES[case] if isinstance(case, str) else case
    inp = lu.inputs(case)
    lstm = Encoder(512).lstm
    if (c["I"], c["H"], c["bi"]) != (512, 256, True):
        lstm = nn.LSTM(c["I"], c["H"], num_layers=1, batch_first=True, bidirectional=c["bi"])
    lstm.load_state_dict({k: torch.from_numpy(v) for k, v in inp["weights"].items()})
    lstm = lstm.to(dtype)
    x = torch.from_numpy(inp["x"]).to(dtype).requires_grad_(True)
    up = torch.from_numpy(inp["up"]).to(dtype)
    hx = None
    if inp["h0"] is not None:
        hx = (torch.from_numpy(inp["h0"]).to(dtype), torch.from_numpy(inp["c0"]).to(dtype))
    packed = nn.utils.rnn.pack_padded_sequence(x, np.asarray(inp["lens"]), batch_first=True, enforce_sorted=False)
    lstm.flatten_parameters()
    outputs, (h_n, c_n) = lstm(packed, hx)
    outputs, _ = nn.utils.rnn.pad_packed_sequence(outputs, batch_first=True)
    assert outputs.dtype == dtype
    (outputs * up).sum().backward()
    r = {"out": outputs.detach().numpy(), "h_n": h_n.detach().numpy(), "c_n": c_n.detach().numpy(),
         "grad_x": x.grad.numpy()}
    for name, p in lstm.named_parameters():
        r["grad_" + name] = p.grad.numpy()
    return r


def reference_errors(Encoder, case):
    r32, r64 = run_reference(Encoder, case, __import__("torch").float32), \
        run_reference(Encoder, case, __import__("torch").float64)
    return r32, r64, {n: lu.ratio(r32[n], r64[n]) for n in r64}


def main():
    mg._stub_text_deps()
    mg._stub_audio_deps()
    sys.path.insert(0, mg.REF)
    from layers.tacotron2 import Encoder
    out, errors = {}, {}
    for case in lu.CASES:
        r32, r64, errors[case] = reference_errors(Encoder, case)
        for name in lu.tensor_names(lu.CASES[case]["bi"]):
            out[lu.key(case, name, 32)] = lu.stored(case, name, r32[name])
            out[lu.key(case, name, 64)] = lu.stored(case, name, r64[name])
        print(f"{case}: worst fp32-vs-fp64 ratio {max(errors[case].values()):.3e}")
    _, _, errors["bench_shape"] = reference_errors(Encoder, lu.BENCH)
    print(f"bench shape: worst fp32-vs-fp64 ratio {max(errors['bench_shape'].values()):.3e}")
    path = os.path.join(HERE, "lstm_train.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 1 << 20
    prof = os.path.join(REPO, "profiles", "lstm_train.json")
    doc = json.load(open(prof)) if os.path.exists(prof) else {}
    doc["bound"] = "max|got - ref64| <= 4e-6 * max(1, max|ref64|) per tensor"
    doc["reference_fp32"] = dict(what="max|ref32 - ref64| / max(1, max|ref64|) of the reference's nn.LSTM on the CPU",
                                 worst_over_test_cases=max(max(v.values()) for k, v in errors.items()
                                                           if k != "bench_shape"),
                                 worst_at_bench_shape=max(errors["bench_shape"].values()), per_case=errors)
    json.dump(doc, open(prof, "w"), indent=1, sort_keys=True)
    print(prof)


if __name__ == "__main__":
    main()
