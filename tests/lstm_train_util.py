"""Shared by tests/golden/make_golden_lstm_train.py, test_lstm_train_cpu.py, test_gpu_lstm_train.py and
tools/bench_lstm_train.py: the cases of the lstm_train.npz fixture (inputs, upstream gradients and weights
regenerated from seeds, never stored), the index sample the large tensors are stored at, a float64 numpy
restatement of the forward and the backward of the encoder's LSTM (layers/tacotron2.py:56-76), and the bound.

Bound.  The project's model-half tolerance (test_gpu_parity.py: 4e-6 max-abs) in the form encoder_util.py uses
for unbounded quantities: per tensor

    max |got - ref64| <= 4e-6 * max(1, max |ref64|)

It is not derived from what the kernels give.  The reference's own float32 run sits at <= 7.7e-7 of
max(1, max |ref64|) over these cases (profiles/lstm_train.json), 5x inside it.
"""
import numpy as np

TOL = 4e-6  # == encoder_util.ALIGN_ATOL == test_gpu_parity.ALIGN_ATOL (test_lstm_train_cpu.py checks it)
KC = 512    # LT_KC of csrc/lstm_train.hip: valid positions per reduction chunk of the weight gradients
SAMPLE = 400  # elements a tensor larger than this is stored at

PARAMS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")


def _b17_lens():
    return [int(v) for v in np.random.Generator(np.random.PCG64(411)).permutation(np.arange(8, 25))]


def _chunk_lens():
    return [int(v) for v in np.random.Generator(np.random.PCG64(412)).integers(16, 31, 48)]


# name -> dict(seed, I, H, bidirectional, lens, Tmax, form, state)
#   form: "lstm" = LSTM.lstm(x, lengths) on padded input, "packed" = the PackedSequence call of Encoder.forward
CASES = {
    "one": dict(seed=401, I=512, H=256, bi=True, lens=[1], form="packed"),
    "l24": dict(seed=402, I=512, H=256, bi=True, lens=[24], form="packed"),
    "unsorted": dict(seed=403, I=512, H=256, bi=True, lens=[7, 1, 24], form="lstm"),
    "packed": dict(seed=404, I=512, H=256, bi=True, lens=[24, 7, 1], form="packed"),
    "b17": dict(seed=405, I=512, H=256, bi=True, lens=_b17_lens(), form="lstm"),  # past one 16-row MFMA tile
    "small_bi": dict(seed=406, I=32, H=48, bi=True, lens=[5, 1, 9], form="lstm"),
    "small_uni": dict(seed=407, I=32, H=48, bi=False, lens=[5, 1, 9], form="lstm"),
    "chunks": dict(seed=408, I=512, H=256, bi=True, lens=_chunk_lens(), form="lstm"),  # 2 whole chunks + a partial one
    "state": dict(seed=409, I=512, H=256, bi=True, lens=[9, 4], form="packed", state=True),
}
assert 2 * KC < sum(CASES["chunks"]["lens"]) < 3 * KC and sum(CASES["chunks"]["lens"]) % KC
BENCH = dict(seed=420, I=512, H=256, bi=True, form="lstm",
             lens=[int(v) for v in np.random.Generator(np.random.PCG64(421)).integers(40, 151, 32)])


def param_names(bi):
    return [n + s for s in (("", "_reverse") if bi else ("",)) for n in PARAMS]


def tensor_names(bi):
    return ["out", "h_n", "c_n", "grad_x"] + ["grad_" + n for n in param_names(bi)]


def inputs(case):
    """dict(x [B, T, I], up [B, T, D * H] (the upstream gradient of out), lens, weights {name: array},
    h0, c0 ([D, B, H] or None)), all float32.  Weights U(-1 / sqrt(H), 1 / sqrt(H)) as nn.LSTM draws them; x and up
    standard normal on EVERY row (the padding rows too: nothing may read them)."""
    c = CASES[case] if isinstance(case, str) else case
    g = np.random.Generator(np.random.PCG64(c["seed"]))
    I, H, D, lens = c["I"], c["H"], 2 if c["bi"] else 1, c["lens"]
    B, T = len(lens), max(lens)
    k = 1.0 / np.sqrt(H)
    weights = {}
    for name in param_names(c["bi"]):
        shape = (4 * H, I) if "weight_ih" in name else (4 * H, H) if "weight_hh" in name else (4 * H,)
        weights[name] = g.uniform(-k, k, shape).astype(np.float32)
    x = g.standard_normal((B, T, I)).astype(np.float32)
    up = g.standard_normal((B, T, D * H)).astype(np.float32)
    h0 = c0 = None
    if c.get("state"):
        h0 = g.uniform(-1.0, 1.0, (D, B, H)).astype(np.float32)
        c0 = g.standard_normal((D, B, H)).astype(np.float32)
    return dict(x=x, up=up, lens=list(lens), weights=weights, h0=h0, c0=c0, bi=c["bi"], I=I, H=H)


def sample_indices(case, name, size):
    """Flat indices a tensor of ``size`` elements is stored at (all of them up to SAMPLE elements)."""
    if size <= SAMPLE:
        return np.arange(size)
    seed = CASES[case]["seed"] * 1000 + sum(ord(ch) for ch in name)
    return np.sort(np.random.Generator(np.random.PCG64(seed)).choice(size, SAMPLE, replace=False))


def stored(case, name, t):
    flat = np.asarray(t).reshape(-1)
    return flat[sample_indices(case, name, flat.size)]


def key(case, name, bits):
    return f"{case}__{name}__{bits}"


# ------------------------------------------------------------------ the LSTM, restated in float64
def _sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


def restate(inp, up=None, mutant=None):
    """Forward and backward in float64 from the float32 operands of ``inputs()``: every tensor of
    ``tensor_names()``.  Per direction, gate rows i, f, g, o, sentence b at its own length; the reverse direction
    visits L_b - 1 .. 0; rows t >= L_b of out and grad_x are 0; the gradients sum over valid positions only.
    ``up`` overrides the upstream gradient.  ``mutant`` breaks it on purpose (test_lstm_train_cpu.py):
    "no_carry" drops the dc * f carry, "rev_index" runs the reverse direction over 0 .. L_b - 1, "bias_pad"
    sums the bias gradients over the padding positions too (every sentence run at full length for them)."""
    x = inp["x"].astype(np.float64)
    up = (inp["up"] if up is None else np.asarray(up)).astype(np.float64)
    lens, H, bi = inp["lens"], inp["H"], inp["bi"]
    D = 2 if bi else 1
    B, T, I = x.shape
    r = {"out": np.zeros((B, T, D * H)), "h_n": np.zeros((D, B, H)), "c_n": np.zeros((D, B, H)),
         "grad_x": np.zeros((B, T, I))}
    for d in range(D):
        sfx = "_reverse" if d else ""
        w_ih, w_hh, b_ih, b_hh = (inp["weights"][n + sfx].astype(np.float64) for n in PARAMS)
        g_ih, g_hh, g_b = np.zeros_like(w_ih), np.zeros_like(w_hh), np.zeros_like(b_ih)
        for b in range(B):
            L = lens[b]
            order = list(range(L)) if (d == 0 or mutant == "rev_index") else list(range(L - 1, -1, -1))
            h = inp["h0"][d, b].astype(np.float64) if inp["h0"] is not None else np.zeros(H)
            c = inp["c0"][d, b].astype(np.float64) if inp["c0"] is not None else np.zeros(H)
            saved = []
            for t in order:
                pre = w_ih @ x[b, t] + b_ih + w_hh @ h + b_hh
                i, f, g, o = _sigmoid(pre[:H]), _sigmoid(pre[H:2 * H]), np.tanh(pre[2 * H:3 * H]), _sigmoid(pre[3 * H:])
                c_new = f * c + i * g
                tc = np.tanh(c_new)
                saved.append((t, h, c, i, f, g, o, tc))
                h, c = o * tc, c_new
                r["out"][b, t, d * H:(d + 1) * H] = h
            r["h_n"][d, b], r["c_n"][d, b] = h, c
            dh_rec, dc_carry = np.zeros(H), np.zeros(H)
            for t, h_prev, c_prev, i, f, g, o, tc in reversed(saved):
                dh = up[b, t, d * H:(d + 1) * H] + dh_rec
                do = dh * tc
                dc = dc_carry + dh * o * (1.0 - tc * tc)
                di, df, dg = dc * g, dc * c_prev, dc * i
                dc_carry = 0.0 * dc if mutant == "no_carry" else dc * f
                dpre = np.concatenate([di * i * (1 - i), df * f * (1 - f), dg * (1 - g * g), do * o * (1 - o)])
                r["grad_x"][b, t] += dpre @ w_ih
                g_ih += np.outer(dpre, x[b, t])
                g_hh += np.outer(dpre, h_prev)
                g_b += dpre
                dh_rec = dpre @ w_hh
        r["grad_weight_ih_l0" + sfx], r["grad_weight_hh_l0" + sfx] = g_ih, g_hh
        r["grad_bias_ih_l0" + sfx], r["grad_bias_hh_l0" + sfx] = g_b, g_b.copy()
    if mutant == "bias_pad":
        full = restate(dict(inp, lens=[T] * B), up=up)
        for n in tensor_names(bi):
            if "bias" in n:
                r[n] = full[n]
    return r


# ------------------------------------------------------------------ the bound
def ratio(got, ref64):
    """max |got - ref64| / max(1, max |ref64|): within the bound when <= TOL."""
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    return float(np.abs(got - ref64).max() / max(1.0, float(np.abs(ref64).max())))


def check(got, ref64, what):
    """Prints the figure, then asserts the bound.  Returns the ratio."""
    v = ratio(got, ref64)
    print(f"{what}: max|got - ref64| / max(1, max|ref64|) = {v:.3e} (bound {TOL:.1e})")
    assert np.isfinite(np.asarray(got)).all(), f"{what}: non-finite values"
    assert v <= TOL, f"{what}: {v:.3e} above {TOL:.1e}"
    return v


# ------------------------------------------------------------------ a small model for train.train_batch
def tiny_model(device_lstm_cls=None):
    """Embedding -> transpose -> an encoder whose ``lstm`` is packed exactly as Encoder.forward packs it
    (layers/tacotron2.py:64-76) -> linear heads that give train_batch's four outputs on train_util's batch."""
    import torch
    from torch import nn

    import train_util as tu

    class Encoder(nn.Module):
        def __init__(self):
            super().__init__()
            self.lstm = nn.LSTM(32, 16, num_layers=1, batch_first=True, bidirectional=True)

        def forward(self, x, input_lengths):
            x = x.transpose(1, 2)
            input_lengths = input_lengths.cpu().numpy()
            x = nn.utils.rnn.pack_padded_sequence(x, input_lengths, batch_first=True)
            self.lstm.flatten_parameters()
            outputs, _ = self.lstm(x)
            outputs, _ = nn.utils.rnn.pad_packed_sequence(outputs, batch_first=True)
            return outputs

    class Tiny(nn.Module):
        def __init__(self):
            super().__init__()
            self.embedding = nn.Embedding(100, 32)
            self.encoder = Encoder()
            self.to_mel = nn.Linear(32, tu.D)
            self.to_post = nn.Linear(32, tu.D)
            self.decoder = nn.Module()
            self.decoder.stopnet = nn.Linear(tu.D * tu.R, 1)
            self.seen = {}

        def forward(self, text, text_lengths, mel, speaker_ids=None):
            x = self.embedding(text).transpose(1, 2)
            self.seen["x"] = x.transpose(1, 2).detach().clone()
            enc = self.encoder(x, text_lengths)
            enc.register_hook(lambda g: self.seen.__setitem__("grad_out", g.detach().clone()))
            self.seen["out"] = enc.detach().clone()
            pooled = enc.sum(1) / text_lengths.float()[:, None]
            dec = 0.5 * mel + self.to_mel(pooled)[:, None, :]
            post = dec + self.to_post(pooled)[:, None, :]
            nb, nt, nd = mel.shape
            stop = self.decoder.stopnet(dec.detach().reshape(nb, nt // tu.R, nd * tu.R)).squeeze(-1)
            return dec, post, torch.zeros(nb, nt // tu.R, text.shape[1], device=mel.device), stop

    torch.manual_seed(430)
    return Tiny()
