"""Generate tests/golden/gru_train.npz by running the REFERENCE's GRU modules with autograd.

Runs on the CPU, where the reference checkout is (make_golden.REF); nothing here runs on the GPU:

    python tests/golden/make_golden_gru_train.py

Built as make_golden_lstm_train.py is: make_golden's stubs, then the GRU modules as the reference constructs
them, ``layers.tacotron.CBHG(128, ...).gru`` (the encoder's and the postnet's, layers/tacotron.py:165-170) and
``layers.gst_layers.ReferenceEncoder(80, 256).recurrence`` (layers/gst_layers.py:53-56), rebuilt with a case's
sizes where they differ.  Each gets the seeded weights of tests/gru_train_util.py and runs as the reference calls it
(``outputs, h_n = gru(x)`` on a padded batch, layers/tacotron.py:204-205, layers/gst_layers.py:76-77), then
``((out * up_out).sum() + (h_n * up_hn).sum()).backward()`` with the upstreams the case has, once in float32 and
once with ``.double()``.  Stored per case and precision: out, h_n, grad_x and the parameter gradients, tensors above
``SAMPLE`` elements at the seeded index sample of ``gru_train_util.sample_indices``.  ``meta`` (a JSON string) holds
the reference's own float32-against-float64 figure per case and tensor in the bound's form ("reference_fp32"; "swap":
the util's small model through ``torch_train_step``), the state-dict keys and shapes of the two modules
("state_dict") and ``gru_sites``: (module path, input_size, hidden_size, bidirectional) of every ``nn.GRU`` that
``named_modules()`` finds in the reference's ``TacotronGST``.  Only seeds (in gru_train_util.py), names and results
are stored.

The same figures go into the "reference_fp32" section of profiles/gru_train.json (the other sections are left as
they are).
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
import gru_train_util as gu  # noqa: E402


def reference_module(mods, c):
    from torch import nn
    CBHG, ReferenceEncoder = mods
    gru = CBHG(128).gru if c["bi"] else ReferenceEncoder(80, 256).recurrence
    if (gru.input_size, gru.hidden_size) != (c["I"], c["H"]):
        gru = nn.GRU(c["I"], c["H"], 1, batch_first=True, bidirectional=c["bi"])
    assert (gru.input_size, gru.hidden_size, gru.bidirectional, gru.batch_first) == (c["I"], c["H"], c["bi"], True)
    return gru


def run_reference(mods, case, dtype):
    import torch
    c = gu._case(case)
    inp = gu.inputs(case)
    gru = reference_module(mods, c)
    gru.load_state_dict({k: torch.from_numpy(v) for k, v in inp["weights"].items()})
    gru = gru.to(dtype)
    x = torch.from_numpy(inp["x"]).to(dtype).requires_grad_(True)
    hx = None if inp["h0"] is None else torch.from_numpy(inp["h0"]).to(dtype)
    gru.flatten_parameters()
    outputs, h_n = gru(x) if hx is None else gru(x, hx)
    assert outputs.dtype == dtype
    loss = 0.0
    if inp["up_out"] is not None:
        loss = loss + (outputs * torch.from_numpy(inp["up_out"]).to(dtype)).sum()
    if inp["up_hn"] is not None:
        loss = loss + (h_n * torch.from_numpy(inp["up_hn"]).to(dtype)).sum()
    loss.backward()
    r = {"out": outputs.detach().numpy(), "h_n": h_n.detach().numpy(), "grad_x": x.grad.numpy()}
    for name, p in gru.named_parameters():
        r["grad_" + name] = p.grad.numpy()
    return r


def reference_errors(mods, case):
    import torch
    r32, r64 = run_reference(mods, case, torch.float32), run_reference(mods, case, torch.float64)
    return r32, r64, {n: gu.ratio(r32[n], r64[n]) for n in r64}


def swap_errors():
    """The util's small model through one torch training step, float32 against float64, in the bound's form."""
    import torch

    import train_util as tu
    c = tu.config("TacotronGST", grad_clip=1e9)
    r32, r64 = gu.torch_train_step(gu.tiny_model(), c, torch.float32), gu.torch_train_step(gu.tiny_model(), c, torch.float64)
    err = {k: gu.ratio(r32["losses"][k], r64["losses"][k]) for k in r64["losses"]}
    for part in ("grads", "params"):
        for n in r64[part]:
            err[f"{part}.{n}"] = gu.ratio(r32[part][n], r64[part][n])
    return err


def reference_sites():
    from utils.generic_utils import load_config, setup_model
    C = load_config(os.path.join(mg.REF, "config_tacotron_gst.json"))
    assert C.model == "TacotronGST"
    model = setup_model(130, 0, C)
    assert type(model).__name__ == "TacotronGST"
    return gu.gru_sites(model)


def main():
    mg._stub_text_deps()
    mg._stub_audio_deps()
    sys.path.insert(0, mg.REF)
    from layers.gst_layers import ReferenceEncoder
    from layers.tacotron import CBHG
    mods = (CBHG, ReferenceEncoder)
    out, errors = {}, {}
    for case in gu.CASES:
        r32, r64, errors[case] = reference_errors(mods, case)
        for name in gu.tensor_names(gu.CASES[case]["bi"]):
            out[gu.key(case, name, 32)] = gu.stored(case, name, r32[name])
            out[gu.key(case, name, 64)] = gu.stored(case, name, r64[name])
        print(f"{case}: worst fp32-vs-fp64 ratio {max(errors[case].values()):.3e}")
    bench = {}
    for site, c in gu.BENCH.items():
        _, _, bench[site] = reference_errors(mods, c)
        print(f"bench shape {site}: worst fp32-vs-fp64 ratio {max(bench[site].values()):.3e}")
    errors["swap"] = swap_errors()
    print(f"swap: worst fp32-vs-fp64 ratio {max(errors['swap'].values()):.3e}")
    sites = reference_sites()
    print("gru_sites:", sites)
    state = {"cbhg.gru": {k: list(v.shape) for k, v in CBHG(128).gru.state_dict().items()},
             "recurrence": {k: list(v.shape) for k, v in ReferenceEncoder(80, 256).recurrence.state_dict().items()}}
    out["meta"] = np.array(json.dumps(dict(reference_fp32=errors, state_dict=state, gru_sites=sites), sort_keys=True))
    path = os.path.join(HERE, "gru_train.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 1 << 20
    prof = os.path.join(REPO, "profiles", "gru_train.json")
    doc = json.load(open(prof)) if os.path.exists(prof) else {}
    doc["bound"] = "max|got - ref64| <= max(4e-6, 4 x reference_fp32) * max(1, max|ref64|) per tensor"
    doc["reference_fp32"] = dict(what="max|ref32 - ref64| / max(1, max|ref64|) of the reference's nn.GRU on the CPU",
                                 worst_over_test_cases=max(max(v.values()) for k, v in errors.items() if k != "swap"),
                                 worst_at_bench_shapes=max(max(v.values()) for v in bench.values()),
                                 per_case=errors, bench_shapes=bench)
    json.dump(doc, open(prof, "w"), indent=1, sort_keys=True)
    print(prof)


if __name__ == "__main__":
    main()
