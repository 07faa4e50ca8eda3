"""Generate tests/golden/convbn_train.npz by running the REFERENCE ConvBNBlock, Encoder and Postnet with autograd.

Run in the build container only (needs /root/reference; nothing here runs on the GPU box):

    python tests/golden/make_golden_convbn_train.py

Built as make_golden_lstm_train.py is: make_golden's stubs, then ``layers.tacotron2.ConvBNBlock`` (single-block
cases), ``Encoder(512).convolutions`` ("enc_stack") and ``Postnet(80).convolutions`` ("postnet") from the reference,
unmodified, in ``train()`` mode, with the seeded weights of tests/convbn_train_util.py.

The dropout masks are the reference run's own: a forward hook on every block's ``net[-1]`` records ``output != 0``
wherever ``input != 0`` (elsewhere the mask cannot change any result: 1 is stored).  The float32 run is then
reproduced through ``net[:-1](x) * mask * 2`` and must be BITWISE the hooked run; the float64 pass takes that route
with the float32 pass's masks.  ``(out * upstream).sum().backward()`` gives the gradients; a second forward on the
same input with the same masks gives the running statistics after two steps.

Stored per case: the masks as packed bits per block, and in float32 and float64 out, grad_x, the four parameter
gradients per block, running_mean / running_var after one forward and after two (tensors above ``SAMPLE``
elements at the seeded index sample of ``convbn_train_util.sample_indices``), num_batches_tracked, and the list of
state-dict keys and shapes of a reference block.  Only seeds (in convbn_train_util.py), masks and results are stored.

Also writes the reference's own float32-against-float64 error per case and tensor, in the bound's form, into the
"reference_fp32" section of profiles/convbn_train.json (the other sections are left as they are), the two bench
shapes included.
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
import convbn_train_util as cu  # noqa: E402


def build_blocks(ref, c, inp):
    """The reference's modules for a case, seeded weights loaded, in train() mode: a list of ConvBNBlock."""
    import torch
    if c["blocks"] == cu.ENC:
        blocks = list(ref.Encoder(512).convolutions)
    elif c["blocks"] == cu.POST:
        blocks = list(ref.Postnet(80).convolutions)
    else:
        blocks = [ref.ConvBNBlock(cin, cout, 5, act) for cin, cout, act in c["blocks"]]
    for blk, weights in zip(blocks, inp["blocks"]):
        blk.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in cu.state_dict(weights).items()})
        blk.train()
    return blocks


def collect(blocks, x, out, up):
    (out * up).sum().backward()
    r = {"out": out.detach().numpy().copy(), "grad_x": x.grad.numpy().copy()}
    for i, blk in enumerate(blocks):
        conv, norm = blk.net[0], blk.net[1]
        for p, t in zip(cu.PARAMS, (conv.weight, conv.bias, norm.weight, norm.bias)):
            r[f"grad_{p}{i}"] = t.grad.numpy().copy()
    return r


def stats(blocks, r, step):
    for i, blk in enumerate(blocks):
        r[f"rm{step}_{i}"] = blk.net[1].running_mean.numpy().copy()
        r[f"rv{step}_{i}"] = blk.net[1].running_var.numpy().copy()


def run_hooked(ref, case):
    """The reference's own forward (its Dropout draws the masks) and backward, float32."""
    import torch
    c, inp = cu.case_of(case), cu.inputs(case)
    torch.manual_seed(c["seed"])
    blocks = build_blocks(ref, c, inp)
    found = {}
    for i, blk in enumerate(blocks):
        blk.net[-1].register_forward_hook(
            lambda mod, args, output, i=i: found.__setitem__(i, torch.where(args[0] != 0, output != 0,
                                                                            torch.ones_like(output, dtype=torch.bool))))
    x = torch.from_numpy(inp["x"]).requires_grad_(True)
    h = x
    for blk in blocks:
        h = blk(h)
    r = collect(blocks, x, h, torch.from_numpy(inp["up"]))
    stats(blocks, r, 1)
    return r, [found[i].numpy().astype(np.uint8) for i in range(len(blocks))]


def run_masked(ref, case, masks, dtype):
    """``net[:-1](x) * mask * 2`` per block: forward, backward, then a second forward with the same masks."""
    import torch
    c, inp = cu.case_of(case), cu.inputs(case)
    blocks = [b.to(dtype) for b in build_blocks(ref, c, inp)]
    x = torch.from_numpy(inp["x"]).to(dtype).requires_grad_(True)

    def forward():
        h = x
        for blk, m in zip(blocks, masks):
            h = blk.net[:-1](h) * torch.from_numpy(m).to(dtype) * (1.0 / (1.0 - blk.net[-1].p))
        return h

    r = collect(blocks, x, forward(), torch.from_numpy(inp["up"]).to(dtype))
    stats(blocks, r, 1)
    with torch.no_grad():
        forward()
    stats(blocks, r, 2)
    r["num_batches_tracked"] = [int(b.net[1].num_batches_tracked) for b in blocks]
    return r


def reference_errors(ref, case, conditions=True):
    r_hook, masks = run_hooked(ref, case)
    r32, r64 = run_masked(ref, case, masks, __import__("torch").float32), \
        run_masked(ref, case, masks, __import__("torch").float64)
    for name, v in r_hook.items():
        assert np.array_equal(v.view(np.uint32), r32[name].view(np.uint32)), f"{case} {name}: the masked route differs"
    restated = cu.restate(cu.inputs(case), masks)
    if conditions:  # (the bench shapes are only measured: millions of elements, some of them next to the kink)
        assert restated["n"] >= cu.MIN_N, (case, restated["n"])
        assert restated["minz"] >= cu.MIN_Z, f"{case}: min |z64| = {restated['minz']:.3e}: try another seed"
    errors = {n: cu.ratio(r32[n], r64[n], cu.bias_scale(n, restated)) for n in cu.tensor_names(case)}
    errors["conv_bias_gradient_in_the_plain_form"] = max(
        cu.ratio(r32[n], r64[n]) for n in cu.tensor_names(case) if n.startswith("grad_bias"))
    return r32, r64, masks, errors


def main():
    mg._stub_text_deps()
    mg._stub_audio_deps()
    sys.path.insert(0, mg.REF)
    import layers.tacotron2 as ref
    out, errors = {}, {}
    for case in cu.CASES:
        r32, r64, masks, errors[case] = reference_errors(ref, case)
        for i, m in enumerate(masks):
            out[cu.key(case, f"mask{i}", "bits")] = cu.pack_mask(m)
        for name in cu.tensor_names(case):
            out[cu.key(case, name, 32)] = cu.stored(case, name, r32[name])
            out[cu.key(case, name, 64)] = cu.stored(case, name, r64[name])
        assert r32["num_batches_tracked"] == r64["num_batches_tracked"]
        out[cu.key(case, "num_batches_tracked", "i")] = np.asarray(r64["num_batches_tracked"], np.int64)
        worst = max(v for k, v in errors[case].items() if not k.startswith("conv_bias"))
        print(f"{case}: worst fp32-vs-fp64 ratio {worst:.3e}", flush=True)
    sd = ref.ConvBNBlock(512, 512, 5, "relu").state_dict()
    out["state_keys"] = np.asarray(list(sd))
    out["state_shapes"] = np.asarray([",".join(str(d) for d in v.shape) for v in sd.values()])
    path = os.path.join(HERE, "convbn_train.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 1 << 20
    bench = {}
    for name, c in cu.BENCH.items():
        _, _, _, bench[name] = reference_errors(ref, c, conditions=False)
        print(f"bench shape {name}: {bench[name]}", flush=True)
    prof = os.path.join(REPO, "profiles", "convbn_train.json")
    doc = json.load(open(prof)) if os.path.exists(prof) else {}
    doc["bound"] = ("max|got - ref64| <= 4e-6 * max(1, max|ref64|) per tensor; the conv bias gradient: "
                    "<= 4e-6 * max(1, S), S = max_c sum|dy64|")
    plain = lambda e: max(v for k, v in e.items() if not k.startswith("conv_bias"))
    doc["reference_fp32"] = dict(
        what="the bound's figure of the reference's ConvBNBlock / Encoder.convolutions / Postnet.convolutions in "
             "float32 against float64 on the CPU, the same masks on both sides",
        worst_over_test_cases=max(plain(v) for v in errors.values()),
        worst_at_bench_shapes={k: plain(v) for k, v in bench.items()}, per_case=errors, bench_shapes=bench)
    json.dump(doc, open(prof, "w"), indent=1, sort_keys=True)
    print(prof)


if __name__ == "__main__":
    main()
