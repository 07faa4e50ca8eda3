"""Generate tests/golden/model_train.npz by running the REFERENCE Tacotron2 through one training iteration.

Run where the reference checkout is (``make_golden.REF``); nothing here needs a GPU:

    python tests/golden/make_golden_model_train.py

Built as make_golden_decoder_train.py is: make_golden's stubs, then ``models.tacotron2.Tacotron2`` from the
reference, unmodified, with ``location_attn=False``, in ``train()`` mode, in float32 and in float64, with the seeded
weights, token ids, mel targets and masks of tests/model_train_util.py.

Dropout.  ``F`` in the namespaces of the reference's ``layers.tacotron2`` and ``layers.common_layers`` is replaced by
the decoder generator's stand-in, whose ``dropout`` multiplies by the util's masks in the order the reference calls
it (the prenet's two layers over all T + 1 frames, then per step h and c of the attention LSTM, h and c of the
decoder LSTM).  Every ``nn.Dropout`` of the conv-BN blocks and of the stopnet gets a forward hook that returns
``input * mask / (1 - p)``.  ``sequence_mask`` in the namespace of ``models.tacotron2`` hands the text mask over as
a tensor subclass whose ``1 - mask`` is the boolean complement (common_layers.py:234 cannot subtract from a bool
tensor on a current torch).  The reference's text is not touched.

The losses are model_train_util's float64 criteria (on the float32 run too: its outputs are cast up), backwards in
train_batch's order: ``loss.backward()``, then ``stop_loss.backward()`` for a separate stopnet.

Stored per fixture case, float64 only: every tensor of ``model_train_util.tensor_names`` (tensors above ``SAMPLE``
elements at the seeded index sample), the loss values and the two gradient norms, and per tensor and scalar the
reference's own float32-against-float64 figure ("ref32") in the bound's form; once, the reference's state-dict keys
and shapes per decoder width.  Results and seeds only.  The same figures go into the "reference_fp32" section of
profiles/model_train.json, with the twin's figure against the reference's float64 run (other sections are left as
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
import model_train_util as mu  # noqa: E402
from make_golden_decoder_train import _Feeder  # noqa: E402


def run(mods, case, dtype):
    import torch
    m2, t2, cl = mods

    class TextMask(torch.Tensor):  # 1 - mask -> the boolean complement
        def __rsub__(self, other):
            return torch.logical_not(self.as_subclass(torch.Tensor).bool())

    c, inp = mu.CASES[case], mu.inputs(case)
    B, T = len(c["text_lens"]), c["frames"] // c["r"]
    model = m2.Tacotron2(c["dims"]["chars"], 0, c["r"], False, c["norm"], "original", c["pdrop"], c["fwd"], False, False,
                         False, c["sep"])
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in inp["weights"].items()})
    model = model.to(dtype).train()
    mk = mu.tensor_masks(inp["masks"])
    feeder = _Feeder(torch.nn.functional)
    one = torch.ones(1, B, c["dims"]["PN"], dtype=torch.uint8)
    feeder.queue += [torch.cat([mk["prenet"][0], one]), torch.cat([mk["prenet"][1], one])]
    for t in range(T):
        feeder.queue += [mk["att"][0][t], mk["att"][1][t], mk["dec"][0][t], mk["dec"][1][t]]
    hooks, step = [], [0]

    def fixed(mask):
        return lambda mod, args, output: args[0] * mask.to(args[0].dtype) * (1.0 / (1.0 - mod.p))

    for part, convs in (("encoder", model.encoder.convolutions), ("postnet", model.postnet.convolutions)):
        for block, mask in zip(convs, mk[part]):
            hooks.append(block.net[-1].register_forward_hook(fixed(mask)))

    def stop_hook(mod, args, output):
        t = step[0]
        step[0] += 1
        return fixed(mk["stop"][t])(mod, args, output)

    def keep_encoder_outputs(mod, args, output):
        output.retain_grad()
        model.encoder_outputs = output

    hooks.append(model.decoder.stopnet[0].register_forward_hook(stop_hook))
    hooks.append(model.encoder.register_forward_hook(keep_encoder_outputs))
    real = (t2.F, cl.F, m2.sequence_mask)
    t2.F = cl.F = feeder
    m2.sequence_mask = lambda lengths: real[2](lengths).as_subclass(TextMask)
    try:
        text, mel = torch.from_numpy(inp["text"]), torch.from_numpy(inp["mel"]).to(dtype)
        dec, post, align, stop = model(text, torch.LongTensor(inp["text_lens"]), mel)
        assert not feeder.queue and step[0] == T, "the reference called dropout fewer times than masks were queued"
        length = (inp["mel_lens"],) if c["masked"] else ()
        stop_loss, stop_value = mu.bce64(stop, torch.from_numpy(inp["stop_targets"]))
        decoder_loss, decoder_value = mu.mse64(dec, mel, *length)
        postnet_loss, postnet_value = mu.mse64(post, mel, *length)
        loss = decoder_loss + postnet_loss + (0 if c["sep"] else stop_loss)
        loss.backward()
        r = dict(zip(mu.OUTPUTS, (dec, post, align, stop)))
        r.update(decoder_loss=decoder_value, postnet_loss=postnet_value, stop_loss=stop_value,
                 grad_norm=mu._norm(p.grad for p in model.parameters()), grad_norm_st=0.0)
        if c["sep"]:
            stop_loss.backward()
            r["grad_norm_st"] = mu._norm(p.grad for p in model.decoder.stopnet.parameters())
        r["grad_encoder_outputs"] = model.encoder_outputs.grad
        for n, p in model.named_parameters():
            r["grad_" + n] = p.grad if p.grad is not None else torch.zeros_like(p)
    finally:
        t2.F, cl.F, m2.sequence_mask = real
        for h in hooks:
            h.remove()
    return {k: (v.detach().numpy().copy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}, model


def main():
    import torch
    mg._stub_text_deps()
    mg._stub_audio_deps()
    sys.path.insert(0, mg.REF)
    import layers.common_layers as cl
    import layers.tacotron2 as t2
    import models.tacotron2 as m2
    out, errors, against_twin = {}, {}, {}
    for case in mu.FIXTURE_CASES:
        r32, model = run((m2, t2, cl), case, torch.float32)
        r64, _ = run((m2, t2, cl), case, torch.float64)
        tw = mu.twin(case)
        errors[case], against_twin[case] = {}, {}
        for name in mu.tensor_names(case) + list(mu.SCALARS):
            scale = mu.scale_of(case, name, tw)
            errors[case][name] = mu.ratio(r32[name], r64[name], scale)
            against_twin[case][name] = mu.ratio(tw[name], r64[name], scale)
            out[mu.key(case, name, 64)] = np.float64(r64[name]) if name in mu.SCALARS else mu.stored(case, name, r64[name])
            out[mu.key(case, name, "ref32")] = np.float64(errors[case][name])
        sd = model.state_dict()
        out[f"state_keys_r{mu.CASES[case]['r']}"] = np.asarray(list(sd))
        out[f"state_shapes_r{mu.CASES[case]['r']}"] = np.asarray([",".join(str(d) for d in v.shape) for v in sd.values()])
        print(f"{case}: worst fp32-vs-fp64 {max(errors[case].values()):.3e}; twin vs the reference's fp64 "
              f"{max(against_twin[case].values()):.3e}", flush=True)
    path = os.path.join(HERE, "model_train.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 1 << 20
    prof = os.path.join(REPO, "profiles", "model_train.json")
    doc = json.load(open(prof)) if os.path.exists(prof) else {}
    doc["bound"] = ("max|got - ref64| <= tol * max|ref64| per tensor, relative to the tensor's own maximum, tol = "
                    "max(4e-6, 4 x the reference's own float32 figure for that case and tensor); conv bias gradients "
                    "under batch norm against S = max_c sum|dy64|, v's bias gradient under softmax against "
                    "S = max_t sum|de64|; scalars relative to their own value")
    doc["reference_fp32"] = dict(
        what="the bound's figure of the reference's Tacotron2 in float32 against float64 on the CPU, one training "
             "iteration, the same masks on both sides", worst=max(max(v.values()) for v in errors.values()),
        per_case=errors, twin_against_reference_fp64=against_twin)
    json.dump(doc, open(prof, "w"), indent=1, sort_keys=True)
    print(prof)


if __name__ == "__main__":
    main()
