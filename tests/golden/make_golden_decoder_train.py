"""Generate tests/golden/decoder_train.npz by running the REFERENCE Decoder with autograd.

Run where the reference checkout is (``make_golden.REF``); nothing here needs a GPU:

    python tests/golden/make_golden_decoder_train.py

Built as make_golden_lstm_train.py is: make_golden's stubs, then ``layers.tacotron2.Decoder`` from the reference,
unmodified, in ``train()`` mode (the "eval" case in ``eval()``), in float32 and in float64, with the seeded weights,
inputs, masks and upstream gradients of tests/decoder_train_util.py.

Dropout.  ``F`` in the namespaces of the reference's ``layers.tacotron2`` and ``layers.common_layers`` is replaced by
a stand-in whose ``dropout`` multiplies by the util's masks in the order the reference calls it (the prenet's two
layers over all T + 1 frames - the last frame's output is never used, its mask is ones -, then per step h and c of
the attention LSTM, h and c of the decoder LSTM); every other attribute is torch's.  The stopnet's ``nn.Dropout``
gets a forward hook that returns ``input * mask / (1 - p)``.  The text mask is handed over as a tensor subclass
whose ``1 - mask`` is the boolean complement (common_layers.py:234 cannot subtract from a bool tensor on a current
torch); the reference's text is not touched.

Stored per case: every tensor of ``decoder_train_util.tensor_names`` in float32 and float64 (tensors above
``SAMPLE`` elements at the seeded index sample), the reference's own float32-against-float64 figure per tensor
("ref32") in the bound's form, and the reference's state-dict keys and shapes.  Results and seeds only.  The same
figures go into the "reference_fp32" section of profiles/decoder_train.json (other sections are left as they are).
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
import decoder_train_util as du  # noqa: E402


class _Feeder:
    """Stands in for torch.nn.functional in the reference's namespaces: ``dropout`` applies the queued masks."""

    def __init__(self, real):
        self._real, self.queue = real, []

    def __getattr__(self, name):
        return getattr(self._real, name)

    def dropout(self, x, p=0.5, training=True, inplace=False):
        if not training:
            return x
        m = self.queue.pop(0)
        assert tuple(m.shape) == tuple(x.shape), (tuple(m.shape), tuple(x.shape))
        return x * m.to(x.dtype) * (1.0 / (1.0 - p))


def run(ref_mods, case, dtype):
    import torch
    t2, cl = ref_mods

    class TextMask(torch.Tensor):  # 1 - mask -> the boolean complement
        def __rsub__(self, other):
            return torch.logical_not(self.as_subclass(torch.Tensor).bool())

    c, inp = du.CASES[case], du.inputs(case)
    d, T, B = c["dims"], c["T"], len(c["lens"])
    dec = t2.Decoder(d["E"], d["mel"], c["r"], False, c["norm"], "original", c["pdrop"], c["fwd"], False, False, False,
                     c["sep"])
    dec.load_state_dict({k: torch.from_numpy(v) for k, v in inp["weights"].items()})
    dec = dec.to(dtype).train(c["training"])
    feeder = _Feeder(torch.nn.functional)
    t2.F = cl.F = feeder
    hook = None
    if c["training"]:
        mk = {k: torch.from_numpy(v) for k, v in inp["masks"].items()}
        if c["pdrop"]:
            one = torch.ones(1, B, d["PN"], dtype=torch.uint8)
            feeder.queue += [torch.cat([mk["prenet"][0], one]), torch.cat([mk["prenet"][1], one])]
        for t in range(T):
            feeder.queue += [mk["att"][0][t], mk["att"][1][t], mk["dec"][0][t], mk["dec"][1][t]]
        step = [0]

        def stop_hook(mod, args, output):
            t = step[0]
            step[0] += 1
            return args[0] * mk["stop"][t].to(args[0].dtype) * (1.0 / (1.0 - mod.p))

        hook = dec.stopnet[0].register_forward_hook(stop_hook)
    x = torch.from_numpy(inp["inputs"]).to(dtype).requires_grad_(c["training"])
    mem = torch.from_numpy(inp["memories"]).to(dtype).requires_grad_(c["training"])
    mask = torch.from_numpy(inp["mask"]).bool().as_subclass(TextMask)
    try:
        o, s, a = dec(x, mem, mask)
        assert not feeder.queue, "the reference called dropout fewer times than masks were queued"
        r = {"outputs": o, "stop_tokens": s, "alignments": a}
        if c["training"]:
            up = inp["up"]
            ((o * torch.from_numpy(up["outputs"]).to(dtype)).sum()
             + (s * torch.from_numpy(up["stop_tokens"]).to(dtype)).sum()).backward()
            r["grad_inputs"], r["grad_memories"] = x.grad, mem.grad
            for n, p in dec.named_parameters():
                r["grad_" + n] = p.grad if p.grad is not None else torch.zeros_like(p)
    finally:
        t2.F = cl.F = feeder._real
        if hook is not None:
            hook.remove()
    # (grad_inputs of the reference is not zero on masked rows only through P = inputs_layer(inputs): the energies
    #  there are overwritten, so it is; the util's restatement writes 0 there as well)
    return {k: v.detach().numpy().copy() for k, v in r.items()}, dec


def main():
    import torch
    mg._stub_text_deps()
    mg._stub_audio_deps()
    sys.path.insert(0, mg.REF)
    import layers.common_layers as cl
    import layers.tacotron2 as t2
    out, errors, against_restatement = {}, {}, {}
    dec = None
    for case in du.FIXTURE_CASES:
        r32, dec = run((t2, cl), case, torch.float32)
        r64, _ = run((t2, cl), case, torch.float64)
        rs = du.restated(case)
        errors[case], against_restatement[case] = {}, {}
        for name in du.tensor_names(case):
            scale = du.scale_of(case, name, rs)
            errors[case][name] = du.ratio(r32[name], r64[name], scale)
            against_restatement[case][name] = du.ratio(rs[name], r64[name], scale)
            out[du.key(case, name, 32)] = du.stored(case, name, r32[name])
            out[du.key(case, name, 64)] = du.stored(case, name, r64[name])
            out[du.key(case, name, "ref32")] = np.float64(errors[case][name])
        print(f"{case}: worst fp32-vs-fp64 {max(errors[case].values()):.3e}; restatement vs the reference's fp64 "
              f"{max(against_restatement[case].values()):.3e}", flush=True)
    sd = dec.state_dict()
    out["state_keys"] = np.asarray(list(sd))
    out["state_shapes"] = np.asarray([",".join(str(d) for d in v.shape) for v in sd.values()])
    path = os.path.join(HERE, "decoder_train.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 1 << 20
    prof = os.path.join(REPO, "profiles", "decoder_train.json")
    doc = json.load(open(prof)) if os.path.exists(prof) else {}
    doc["bound"] = ("max|got - ref64| <= tol * max(1, max|ref64|) per tensor, tol = max(4e-6, 4 x the reference's own "
                    "float32 figure for that case and tensor); v's bias gradient under softmax against "
                    "S = max_t sum|de64|")
    doc["reference_fp32"] = dict(
        what="the bound's figure of the reference's Decoder in float32 against float64 on the CPU, the same masks on "
             "both sides", worst=max(max(v.values()) for v in errors.values()), per_case=errors,
        restatement_against_reference_fp64=against_restatement)
    json.dump(doc, open(prof, "w"), indent=1, sort_keys=True)
    print(prof)


if __name__ == "__main__":
    main()
