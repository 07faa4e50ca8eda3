"""Shared by tests/golden/make_golden_gru_train.py, test_gru_train_cpu.py, test_gpu_gru_train.py and
tools/bench_gru_train.py: the cases of the gru_train.npz fixture (inputs, upstream gradients and weights
regenerated from seeds, never stored), the index sample the large tensors are stored at, a float64 numpy
restatement of the forward and the backward of the single-layer GRU the reference's Tacotron / TacotronGST use
at three sites (layers/tacotron.py:165-170, :204-205; layers/gst_layers.py:53-56, :74-78), a plain-torch
Tacotron-shaped small model with a GRU at each of the three module paths, and the bound.

The cell (ATen's):  xi = W_ih x_t + b_ih,  hh = W_hh h_prev + b_hh,
    r = s(xi_r + hh_r)   z = s(xi_z + hh_z)   n = tanh(xi_n + r * hh_n)   h = (1 - z) * n + z * h_prev
The backward, dh_t = upstream of out[:, t] + carry, the carry starting as the upstream of h_n:
    da_n = dh * (1 - z) * (1 - n^2)   da_z = dh * (h_prev - n) * z * (1 - z)   da_r = da_n * hh_n * r * (1 - r)
    dpre_i = [da_r | da_z | da_n]       grad_W_ih += dpre_i^T x_t,    grad_b_ih += sum_b dpre_i,  grad_x_t = dpre_i W_ih
    dpre_h = [da_r | da_z | da_n * r]   grad_W_hh += dpre_h^T h_prev, grad_b_hh += sum_b dpre_h
    carry  = dh * z + dpre_h W_hh

Bound.  The project's per-tensor form (decoder_train_util.py):

    max |got - ref64| <= tol * max(1, max |ref64|),   tol = max(4e-6, 4 x the reference's own float32 figure)

with the reference's figure (torch.nn.GRU in float32 against float64 on the CPU, the same form) read from the
fixture per case and tensor, never from a device run.  Those figures sit at a few 1e-7, so 4e-6 decides.
"""
import json

import numpy as np

TOL = 4e-6
MARGIN = 4.0
KC = 512      # GT_KC of csrc/gru_train.hip: rows per reduction chunk of the weight gradients
SAMPLE = 400  # elements a tensor larger than this is stored at

PARAMS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")

# the three sites of the reference's TacotronGST: (module path, input_size, hidden_size, bidirectional)
SITES = (("encoder.cbhg.cbhg.gru", 128, 128, True), ("gst.encoder.recurrence", 256, 128, False),
         ("postnet.cbhg.gru", 128, 128, True))

# name -> dict(seed, I, H, bi, B, T, ups ("out" | "h_n" | "both": where the upstream gradient arrives), state)
CASES = {
    "one": dict(seed=501, I=128, H=128, bi=True, B=1, T=1),          # the loop's first-is-last edge
    "t2": dict(seed=502, I=128, H=128, bi=True, B=2, T=2),           # both parities of the double-buffered state
    "t3": dict(seed=503, I=128, H=128, bi=True, B=2, T=3),
    "t24": dict(seed=504, I=128, H=128, bi=True, B=3, T=24),         # a chain
    "b17": dict(seed=505, I=128, H=128, bi=True, B=17, T=3),         # past one 16-sentence tile; a tile with one live row
    "gst": dict(seed=506, I=256, H=128, bi=False, B=3, T=5, ups="h_n"),  # the GST site: grad_out == NULL
    "both_ups": dict(seed=507, I=128, H=128, bi=True, B=2, T=4, ups="both"),
    "small": dict(seed=508, I=32, H=48, bi=True, B=3, T=9),          # H no multiple of 32 or 64
    "h16": dict(seed=509, I=16, H=16, bi=True, B=2, T=4),            # one unit tile
    "chunks": dict(seed=510, I=128, H=128, bi=True, B=24, T=24),     # B * T past one reduction chunk, no multiple of it
    "state": dict(seed=511, I=128, H=128, bi=True, B=2, T=5, state=True),
}
assert KC < CASES["chunks"]["B"] * CASES["chunks"]["T"] < 2 * KC
# the training shapes of the three sites (tools/bench_gru_train.py)
BENCH = {
    "encoder": dict(seed=521, I=128, H=128, bi=True, B=32, T=150),
    "postnet": dict(seed=522, I=128, H=128, bi=True, B=32, T=600),
    "gst": dict(seed=523, I=256, H=128, bi=False, B=32, T=10, ups="h_n"),
}


def _case(case):
    return CASES[case] if isinstance(case, str) else case


def param_names(bi):
    return [n + s for s in (("", "_reverse") if bi else ("",)) for n in PARAMS]


def tensor_names(bi):
    return ["out", "h_n", "grad_x"] + ["grad_" + n for n in param_names(bi)]


def inputs(case):
    """dict(x [B, T, I], up_out [B, T, D * H] or None, up_hn [D, B, H] or None, weights {name: array}, h0 [D, B, H]
    or None, bi, I, H), all float32.  Weights U(-1 / sqrt(H), 1 / sqrt(H)) as nn.GRU draws them; x and the upstream
    gradients standard normal; h0 U(-1, 1)."""
    c = _case(case)
    g = np.random.Generator(np.random.PCG64(c["seed"]))
    I, H, D, B, T = c["I"], c["H"], 2 if c["bi"] else 1, c["B"], c["T"]
    k = 1.0 / np.sqrt(H)
    weights = {}
    for name in param_names(c["bi"]):
        shape = (3 * H, I) if "weight_ih" in name else (3 * H, H) if "weight_hh" in name else (3 * H,)
        weights[name] = g.uniform(-k, k, shape).astype(np.float32)
    x = g.standard_normal((B, T, I)).astype(np.float32)
    up_out = g.standard_normal((B, T, D * H)).astype(np.float32)
    up_hn = g.standard_normal((D, B, H)).astype(np.float32)
    h0 = g.uniform(-1.0, 1.0, (D, B, H)).astype(np.float32)
    ups = c.get("ups", "out")
    return dict(x=x, up_out=up_out if ups in ("out", "both") else None, up_hn=up_hn if ups in ("h_n", "both") else None,
                weights=weights, h0=h0 if c.get("state") else None, bi=c["bi"], I=I, H=H)


def sample_indices(case, name, size):
    """Flat indices a tensor of ``size`` elements is stored at (all of them up to SAMPLE elements)."""
    if size <= SAMPLE:
        return np.arange(size)
    seed = _case(case)["seed"] * 1000 + sum(ord(ch) for ch in name)
    return np.sort(np.random.Generator(np.random.PCG64(seed)).choice(size, SAMPLE, replace=False))


def stored(case, name, t):
    flat = np.asarray(t).reshape(-1)
    return flat[sample_indices(case, name, flat.size)]


def key(case, name, bits):
    return f"{case}__{name}__{bits}"


# ------------------------------------------------------------------ the GRU, restated in float64
def _sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


def restate(inp, mutant=None):
    """Forward and backward in float64 from the float32 operands of ``inputs()``: every tensor of
    ``tensor_names()``.  Per direction, gate rows r, z, n; the reverse direction walks T - 1 .. 0.  ``mutant`` breaks
    it on purpose (test_gru_train_cpu.py): "bias_hn_same" uses da_n instead of da_n * r in grad_b_hh and grad_W_hh,
    "no_carry" drops the dh * z carry, "rev_index" runs the reverse direction over 0 .. T - 1, "hn_grad_dropped"
    ignores the upstream gradient of h_n."""
    x = inp["x"].astype(np.float64)
    H, bi = inp["H"], inp["bi"]
    D = 2 if bi else 1
    B, T, I = x.shape
    up_out = np.zeros((B, T, D * H)) if inp["up_out"] is None else inp["up_out"].astype(np.float64)
    up_hn = np.zeros((D, B, H)) if inp["up_hn"] is None or mutant == "hn_grad_dropped" else inp["up_hn"].astype(np.float64)
    r_ = {"out": np.zeros((B, T, D * H)), "h_n": np.zeros((D, B, H)), "grad_x": np.zeros((B, T, I))}
    for d in range(D):
        sfx = "_reverse" if d else ""
        w_ih, w_hh, b_ih, b_hh = (inp["weights"][n + sfx].astype(np.float64) for n in PARAMS)
        g_ih, g_hh, g_bi, g_bh = np.zeros_like(w_ih), np.zeros_like(w_hh), np.zeros_like(b_ih), np.zeros_like(b_hh)
        order = list(range(T)) if (d == 0 or mutant == "rev_index") else list(range(T - 1, -1, -1))
        h = inp["h0"][d].astype(np.float64) if inp["h0"] is not None else np.zeros((B, H))
        saved = []
        for t in order:
            xi = x[:, t] @ w_ih.T + b_ih
            hh = h @ w_hh.T + b_hh
            r = _sigmoid(xi[:, :H] + hh[:, :H])
            z = _sigmoid(xi[:, H:2 * H] + hh[:, H:2 * H])
            n = np.tanh(xi[:, 2 * H:] + r * hh[:, 2 * H:])
            saved.append((t, h, r, z, n, hh[:, 2 * H:]))
            h = (1.0 - z) * n + z * h
            r_["out"][:, t, d * H:(d + 1) * H] = h
        r_["h_n"][d] = h
        carry = up_hn[d]
        for t, h_prev, r, z, n, hh_n in reversed(saved):
            dh = up_out[:, t, d * H:(d + 1) * H] + carry
            da_n = dh * (1.0 - z) * (1.0 - n * n)
            da_z = dh * (h_prev - n) * z * (1.0 - z)
            da_r = da_n * hh_n * r * (1.0 - r)
            dpre_i = np.concatenate([da_r, da_z, da_n], 1)
            dpre_h = np.concatenate([da_r, da_z, da_n * r], 1)
            r_["grad_x"][:, t] += dpre_i @ w_ih
            g_ih += dpre_i.T @ x[:, t]
            g_bi += dpre_i.sum(0)
            wrong = dpre_i if mutant == "bias_hn_same" else dpre_h
            g_hh += wrong.T @ h_prev
            g_bh += wrong.sum(0)
            carry = (0.0 if mutant == "no_carry" else dh * z) + dpre_h @ w_hh
        r_["grad_weight_ih_l0" + sfx], r_["grad_weight_hh_l0" + sfx] = g_ih, g_hh
        r_["grad_bias_ih_l0" + sfx], r_["grad_bias_hh_l0" + sfx] = g_bi, g_bh
    return r_


# ------------------------------------------------------------------ the bound
def ratio(got, ref64, scale=None):
    """max |got - ref64| / max(1, max |ref64|) (``scale`` in place of max |ref64|, for a sampled tensor)."""
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    s = float(np.abs(ref64).max()) if scale is None else float(scale)
    return float(np.abs(got - ref64).max() / max(1.0, s))


def reference_fp32(fixture):
    """{case: {tensor: the reference's float32-against-float64 figure}} of the fixture."""
    return json.loads(str(fixture["meta"]))["reference_fp32"]


def tolerance(ref32, case, name):
    """4e-6, or 4 x the reference's own float32 figure for this case and tensor if that is larger."""
    own = 0.0 if ref32 is None else float(ref32.get(case, {}).get(name, 0.0))
    return max(TOL, MARGIN * own)


def check(got, ref64, what, tol=TOL, scale=None):
    """Prints the figure, then asserts the bound.  Returns the ratio."""
    v = ratio(got, ref64, scale)
    print(f"{what}: max|got - ref64| / max(1, max|ref64|) = {v:.3e} (bound {tol:.1e})")
    assert np.isfinite(np.asarray(got)).all(), f"{what}: non-finite values"
    assert v <= tol, f"{what}: {v:.3e} above {tol:.1e}"
    return v


# ------------------------------------------------------------------ a Tacotron-shaped small model
def tiny_model():
    """A plain-torch model with the reference TacotronGST's forward signature and an ``nn.GRU`` of the reference's
    sizes at each of the three module paths of ``SITES``: embedding -> linear -> ``encoder.cbhg.cbhg.gru``; a linear
    over the mel -> ``gst.encoder.recurrence`` whose h_n (through a linear) is added to the encoder output; a linear
    teacher-forced "decoder"; ``postnet.cbhg.gru`` -> ``last_linear``.  No dropout.  Works on train_util's batch."""
    import torch
    from torch import nn

    import train_util as tu

    class CBHG(nn.Module):
        def __init__(self):
            super().__init__()
            self.gru = nn.GRU(128, 128, 1, batch_first=True, bidirectional=True)

        def forward(self, x):
            self.gru.flatten_parameters()
            outputs, _ = self.gru(x)  # layers/tacotron.py:204-205
            return outputs

    class Holder(nn.Module):
        def __init__(self, **kw):
            super().__init__()
            for k, v in kw.items():
                setattr(self, k, v)

    class RefEncoder(nn.Module):
        def __init__(self):
            super().__init__()
            self.pre = nn.Linear(tu.D, 256)
            self.recurrence = nn.GRU(input_size=256, hidden_size=128, batch_first=True)

        def forward(self, mel):
            self.recurrence.flatten_parameters()
            _, out = self.recurrence(self.pre(mel))  # layers/gst_layers.py:76-78
            return out.squeeze(0)

    class Tiny(nn.Module):
        def __init__(self):
            super().__init__()
            self.embedding = nn.Embedding(100, 32)
            self.encoder = Holder(pre=nn.Linear(32, 128), cbhg=Holder(cbhg=CBHG()))
            self.gst = Holder(encoder=RefEncoder(), style=nn.Linear(128, 256))
            self.to_mel = nn.Linear(256, tu.D)
            self.decoder = nn.Module()
            self.decoder.stopnet = nn.Linear(tu.D * tu.R, 1)
            self.postnet = Holder(pre=nn.Linear(tu.D, 128), cbhg=CBHG())
            self.last_linear = nn.Sequential(nn.Linear(256, tu.D_LINEAR), nn.Sigmoid())

        def forward(self, text, text_lengths, mel, speaker_ids=None):
            enc = self.encoder.cbhg.cbhg(self.encoder.pre(self.embedding(text)))
            enc = enc + self.gst.style(self.gst.encoder(mel))[:, None, :]
            dec = 0.5 * mel + self.to_mel(enc.mean(1))[:, None, :]
            post = self.last_linear(self.postnet.cbhg(self.postnet.pre(dec)))
            nb, nt, nd = mel.shape
            stop = self.decoder.stopnet(dec.detach().reshape(nb, nt // tu.R, nd * tu.R)).squeeze(-1)
            return dec, post, torch.zeros(nb, nt // tu.R, text.shape[1], device=mel.device, dtype=mel.dtype), stop

    torch.manual_seed(530)
    return Tiny()


def gru_sites(model):
    """[(module path, input_size, hidden_size, bidirectional)] of every GRU module (torch's or the package's) that
    ``named_modules()`` finds, in its order."""
    return [(path, m.input_size, m.hidden_size, bool(m.bidirectional)) for path, m in model.named_modules()
            if type(m).__name__ == "GRU"]


SWAP_LR = 0.01


def torch_train_step(model, c, dtype):
    """One iteration of train.train_batch (train.py:92-169) on the CPU in ``dtype`` with torch alone, on train_util's
    batch with plain SGD: dict(losses {name: float}, grads {parameter: array}, params {parameter: array after the
    step}).  SGD, because its step is linear in the gradient: Adam's first step is lr * g / (|g| + eps), which turns
    an error of 1e-7 in a gradient of that size into a whole lr, so no bound on the gradients bounds its result."""
    import torch

    import train_util as tu

    model = model.to(dtype).train()
    opt = torch.optim.SGD(model.parameters(), lr=SWAP_LR)
    opt_st = torch.optim.SGD(model.decoder.stopnet.parameters(), lr=SWAP_LR)
    text, text_lengths, _, linear, mel, mel_lengths, stop_targets, _ = tu.batch()
    linear, mel = linear.to(dtype), mel.to(dtype)
    stop_targets = (stop_targets.view(tu.B, tu.T // c.r, -1).sum(2) > 0.0).to(dtype)
    criterion, criterion_st = tu.torch_criteria(c)
    dec, post, _, stop = model(text, text_lengths, mel)
    stop_loss = criterion_st(stop, stop_targets)
    dec_loss, post_loss = criterion(dec, mel, mel_lengths), criterion(post, linear, mel_lengths)
    (dec_loss + post_loss).backward()
    tu.torch_weight_decay(opt, c.wd)
    tu.torch_check_update(model, c.grad_clip)
    opt.step()
    stop_loss.backward()
    tu.torch_weight_decay(opt_st, c.wd)
    tu.torch_check_update(model.decoder.stopnet, 1.0)
    opt_st.step()
    return dict(losses={k: float(v.detach()) for k, v in (("decoder_loss", dec_loss), ("postnet_loss", post_loss),
                                                            ("stop_loss", stop_loss))},
                grads={n: p.grad.detach().numpy().copy() for n, p in model.named_parameters()},
                params={n: p.detach().numpy().copy() for n, p in model.named_parameters()})
