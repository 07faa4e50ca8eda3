"""Shared by tests/golden/make_golden_convbn_train.py, test_convbn_train_cpu.py, test_gpu_convbn_train.py and
tools/bench_convbn_train.py: the cases of the convbn_train.npz fixture (inputs, upstream gradients and weights
regenerated from seeds, never stored; the dropout masks come from the fixture), the index sample the large tensors
are stored at, a float64 numpy restatement of the forward and the backward of the reference's ConvBNBlock
(layers/tacotron2.py:9-27: Conv1d(k=5, padding=2) -> BatchNorm1d -> ReLU | Tanh | nothing -> Dropout(0.5)), running
statistics included, with mutants, and the bound.

Bound.  The project's model-half tolerance (test_gpu_parity.py: 4e-6 max-abs) in the form encoder_util.py uses
for unbounded quantities: per tensor

    max |got - ref64| <= 4e-6 * max(1, max |ref64|)

except for the conv bias gradient.  Under batch norm it is mathematically zero (sum over positions of dy), so what a
run returns is a cancellation residue; it is bounded against the size of what cancels:

    |got - ref64| <= 4e-6 * max(1, S),   S = max_c sum_{b,t} |dy64[b][c][t]|

Neither is derived from what the kernels give.  The reference's own float32 run on the CPU sits at <= 1.1e-6 (plain
form) and <= 8e-8 (S form) over these cases (profiles/convbn_train.json, "reference_fp32").

Two conditions on the inputs make the bound meetable by any float32 run (test_convbn_train_cpu.py asserts both):
n = B * T >= 6 in every case (two values per channel make 1 / sqrt(var) ill-conditioned), and for relu blocks
min |z64| over the kept elements >= 1e-5, about ten times the forward's float32 error, so that no element can sit on
the other side of the kink from the float64 run.  The seeds below were chosen so that the second holds.
"""
import numpy as np

TOL = 4e-6  # == encoder_util.ALIGN_ATOL == test_gpu_parity.ALIGN_ATOL (test_convbn_train_cpu.py checks it)
KC = 1024   # CB_KC of csrc/convbn_train.hip: positions per reduction chunk of grad_W
SAMPLE = 400  # elements a tensor larger than this is stored at
MIN_N = 6
MIN_Z = 1e-5
EPS, MOMENTUM, P_DROP = 1e-5, 0.1, 0.5  # nn.BatchNorm1d's and the reference's nn.Dropout(p=0.5)

PARAMS = ("W", "bias", "gamma", "beta")
STATE_KEYS = {"W": "net.0.weight", "bias": "net.0.bias", "gamma": "net.1.weight", "beta": "net.1.bias"}

ENC = [(512, 512, "relu")] * 3                                              # Encoder(512).convolutions
POST = [(80, 512, "tanh")] + [(512, 512, "tanh")] * 3 + [(512, 80, None)]   # Postnet(80).convolutions

# name -> dict(seed, blocks [(cin, cout, act)], B, T)
CASES = {
    "t3": dict(seed=501, blocks=[(512, 512, "relu")], B=2, T=3),        # T shorter than the kernel, n = 6
    "b8t1": dict(seed=502, blocks=[(512, 512, "relu")], B=8, T=1),      # only the centre tap is in range
    "b4t2": dict(seed=503, blocks=[(512, 512, "tanh")], B=4, T=2),
    "post_in": dict(seed=504, blocks=[(80, 512, "tanh")], B=2, T=37),   # Cin = 5 tiles of 16, odd T, unaligned rows
    "post_out": dict(seed=505, blocks=[(512, 80, None)], B=2, T=70),    # Cout = 80
    "b17t19": dict(seed=546, blocks=[(512, 512, "relu")], B=17, T=19),  # n = 323: off every 16-multiple, B > 16
    "small": dict(seed=507, blocks=[(48, 32, "tanh")], B=3, T=9),
    "chunks": dict(seed=508, blocks=[(32, 48, "relu")], B=29, T=83),    # 2 whole grad_W chunks + a partial one
    "enc_stack": dict(seed=509, blocks=ENC, B=2, T=7),                  # gradient through three blocks
    "postnet": dict(seed=510, blocks=POST, B=2, T=9),
}
assert 2 * KC < CASES["chunks"]["B"] * CASES["chunks"]["T"] < 3 * KC
assert (CASES["chunks"]["B"] * CASES["chunks"]["T"]) % KC
BENCH = {
    "encoder": dict(seed=520, blocks=ENC, B=32, T=150),
    "postnet": dict(seed=521, blocks=POST, B=32, T=600),
}


def case_of(case):
    return CASES[case] if isinstance(case, str) else case


def tensor_names(case):
    """out, grad_x, then per block i: the four parameter gradients and the running statistics after one forward
    (rm1, rv1) and after a second forward on the same input with the same masks (rm2, rv2)."""
    names = ["out", "grad_x"]
    for i in range(len(case_of(case)["blocks"])):
        names += [f"grad_{p}{i}" for p in PARAMS] + [f"rm1_{i}", f"rv1_{i}", f"rm2_{i}", f"rv2_{i}"]
    return names


def inputs(case):
    """dict(x [B, Cin, T], up [B, Cout, T], blocks [dict(W, bias, gamma, beta, act, cin, cout)]), float32.  W and
    bias as nn.Conv1d draws them (U(-1 / sqrt(5 Cin), 1 / sqrt(5 Cin))), gamma U(0.5, 1.5), beta U(-0.5, 0.5), x and
    up standard normal.  The running statistics start at nn.BatchNorm1d's 0 and 1."""
    c = case_of(case)
    g = np.random.Generator(np.random.PCG64(c["seed"]))
    blocks = []
    for cin, cout, act in c["blocks"]:
        k = 1.0 / np.sqrt(5 * cin)
        blocks.append(dict(W=g.uniform(-k, k, (cout, cin, 5)).astype(np.float32),
                           bias=g.uniform(-k, k, cout).astype(np.float32),
                           gamma=g.uniform(0.5, 1.5, cout).astype(np.float32),
                           beta=g.uniform(-0.5, 0.5, cout).astype(np.float32), act=act, cin=cin, cout=cout))
    x = g.standard_normal((c["B"], c["blocks"][0][0], c["T"])).astype(np.float32)
    up = g.standard_normal((c["B"], c["blocks"][-1][1], c["T"])).astype(np.float32)
    return dict(x=x, up=up, blocks=blocks)


def state_dict(block):
    """A reference-shaped state dict of one block of ``inputs()`` (numpy arrays)."""
    sd = {STATE_KEYS[p]: block[p] for p in PARAMS}
    sd["net.1.running_mean"] = np.zeros(block["cout"], np.float32)
    sd["net.1.running_var"] = np.ones(block["cout"], np.float32)
    sd["net.1.num_batches_tracked"] = np.asarray(0, np.int64)
    return sd


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


def pack_mask(mask):
    return np.packbits(np.asarray(mask, np.uint8).reshape(-1))


def masks(fixture, case):
    """The dropout masks of the fixture's reference run, one uint8 [B, Cout, T] per block (1 = keep)."""
    c = case_of(case)
    out = []
    for i, (_, cout, _) in enumerate(c["blocks"]):
        shape = (c["B"], cout, c["T"])
        bits = np.unpackbits(fixture[key(case, f"mask{i}", "bits")])[:int(np.prod(shape))]
        out.append(bits.reshape(shape).astype(np.uint8))
    return out


# ------------------------------------------------------------------ the block, restated in float64
MUTANTS = ("unbiased_norm", "biased_running", "no_xhat_term", "no_flip", "edge_pad", "scale1")


def _pad(a, mutant=None):
    return np.pad(a, ((0, 0), (0, 0), (2, 2)), mode="edge" if mutant == "edge_pad" else "constant")


def block_forward(x, blk, mask, rm, rv, training=True, mutant=None, scale=None):
    """One block in float64.  Returns (out, saved, rm', rv'); ``saved`` feeds ``block_backward``.  With
    ``training`` false the running statistics normalise, nothing is dropped and nothing moves."""
    W, bias, gamma, beta = (np.asarray(blk[p], np.float64) for p in PARAMS)
    B, _, T = x.shape
    n = B * T
    xp = _pad(x, mutant)
    y = bias[None, :, None] + sum(np.einsum("oi,bit->bot", W[:, :, k], xp[:, :, k:k + T], optimize=True) for k in range(5))
    if training:
        mean, var = y.mean(axis=(0, 2)), y.var(axis=(0, 2))
        rm = (1 - MOMENTUM) * rm + MOMENTUM * mean
        rv = (1 - MOMENTUM) * rv + MOMENTUM * (var if mutant == "biased_running" else var * n / (n - 1))
        used = var * n / (n - 1) if mutant == "unbiased_norm" else var
    else:
        mean, used = np.asarray(rm, np.float64), np.asarray(rv, np.float64)
    invstd = 1.0 / np.sqrt(used + EPS)
    xhat = (y - mean[None, :, None]) * invstd[None, :, None]
    z = gamma[None, :, None] * xhat + beta[None, :, None]
    a = np.maximum(z, 0.0) if blk["act"] == "relu" else np.tanh(z) if blk["act"] == "tanh" else z
    if scale is None:
        scale = 1.0 if mutant == "scale1" else 1.0 / (1.0 - P_DROP)
    keep = np.asarray(mask, np.float64) * scale if training else 1.0
    return a * keep, dict(xp=xp, xhat=xhat, z=z, a=a, invstd=invstd, keep=keep, n=n), rm, rv


def block_backward(g, blk, s, mutant=None):
    """(grad_x, {grad_W, grad_bias, grad_gamma, grad_beta}, S) of one block, float64; S = max_c sum |dy|."""
    W, gamma = np.asarray(blk["W"], np.float64), np.asarray(blk["gamma"], np.float64)
    T = g.shape[2]
    dact = (s["z"] > 0).astype(np.float64) if blk["act"] == "relu" else 1.0 - s["a"] ** 2 if blk["act"] == "tanh" else 1.0
    dz = g * s["keep"] * dact
    s1, s2 = dz.sum(axis=(0, 2)), (dz * s["xhat"]).sum(axis=(0, 2))
    term = 0.0 if mutant == "no_xhat_term" else s["xhat"] * (s2 / s["n"])[None, :, None]
    dy = (gamma * s["invstd"])[None, :, None] * (dz - (s1 / s["n"])[None, :, None] - term)
    gW = np.stack([np.einsum("bot,bit->oi", dy, s["xp"][:, :, k:k + T], optimize=True) for k in range(5)], axis=2)
    dyp = _pad(dy)
    gx = sum(np.einsum("oi,bot->bit", W[:, :, k], dyp[:, :, (k if mutant == "no_flip" else 4 - k):][:, :, :T],
                       optimize=True)
             for k in range(5))
    return gx, dict(W=gW, bias=dy.sum(axis=(0, 2)), gamma=s2, beta=s1), float(np.abs(dy).sum(axis=(0, 2)).max())


def restate(inp, mask_list, up=None, mutant=None):
    """Every tensor of ``tensor_names()`` in float64 from the float32 operands of ``inputs()`` and the masks, plus
    ``S{i}`` (the bias gradient's scale), ``n`` and ``minz`` (min |z| over the kept elements of the relu blocks;
    inf without one).  The second forward runs on the same input with the same masks."""
    x = inp["x"].astype(np.float64)
    up = (inp["up"] if up is None else np.asarray(up)).astype(np.float64)
    r, saved, minz = {}, [], np.inf
    stats = [(np.zeros(b["cout"]), np.ones(b["cout"])) for b in inp["blocks"]]
    for fwd in (1, 2):
        h = x
        for i, (blk, m) in enumerate(zip(inp["blocks"], mask_list)):
            h, s, rm, rv = block_forward(h, blk, m, *stats[i], mutant=mutant)
            stats[i] = (rm, rv)
            r[f"rm{fwd}_{i}"], r[f"rv{fwd}_{i}"] = rm, rv
            if fwd == 1:
                saved.append(s)
                if blk["act"] == "relu" and np.asarray(m).any():
                    minz = min(minz, float(np.abs(s["z"][np.asarray(m) != 0]).min()))
        if fwd == 1:
            r["out"] = h
    g = up
    for i in reversed(range(len(saved))):
        g, grads, r[f"S{i}"] = block_backward(g, inp["blocks"][i], saved[i], mutant)
        for p in PARAMS:
            r[f"grad_{p}{i}"] = grads[p]
    r["grad_x"], r["n"], r["minz"] = g, x.shape[0] * x.shape[2], minz
    return r


# ------------------------------------------------------------------ the bound
def ratio(got, ref64, scale=None):
    """max |got - ref64| / max(1, max |ref64|) (``scale`` given: / max(1, scale)): within the bound when <= TOL."""
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    den = max(1.0, float(np.abs(ref64).max()) if scale is None else float(scale))
    return float(np.abs(got - ref64).max() / den)


def bias_scale(name, ref):
    """S of the block when ``name`` is a conv bias gradient, else None (the plain form)."""
    return ref["S" + name[len("grad_bias"):]] if name.startswith("grad_bias") else None


def check(got, ref64, what, scale=None):
    """Prints the figure, then asserts the bound.  Returns the ratio."""
    v = ratio(got, ref64, scale)
    form = "max(1, max|ref64|)" if scale is None else "max(1, S)"
    print(f"{what}: max|got - ref64| / {form} = {v:.3e} (bound {TOL:.1e})")
    assert np.isfinite(np.asarray(got)).all(), f"{what}: non-finite values"
    assert v <= TOL, f"{what}: {v:.3e} above {TOL:.1e}"
    return v


# ------------------------------------------------------------------ a small model for train.train_batch
def tiny_model():
    """A reference-shaped model in torch alone: embedding 32 -> ``encoder.convolutions`` (two relu blocks 32 -> 32)
    -> ``encoder.lstm`` packed as Encoder.forward packs it -> linear heads on train_util's batch, and a
    ``postnet.convolutions`` of three blocks (16 -> 32 tanh, 32 -> 32 tanh, 32 -> 16 none) between two linear maps
    from and to train_util's mel width (8 is no multiple of 16), residual outside.  Every conv block's input, output
    and upstream gradient of the last forward are kept in ``seen[(part, i)]``."""
    import torch
    from torch import nn

    import train_util as tu

    class Block(nn.Module):  # the structure of layers/tacotron2.py:9-27
        def __init__(self, cin, cout, nonlinear):
            super().__init__()
            act = {"relu": [nn.ReLU()], "tanh": [nn.Tanh()], None: []}[nonlinear]
            self.net = nn.Sequential(nn.Conv1d(cin, cout, 5, padding=2), nn.BatchNorm1d(cout), *act, nn.Dropout(p=0.5))

        def forward(self, x):
            return self.net(x)

    class Encoder(nn.Module):
        def __init__(self):
            super().__init__()
            self.convolutions = nn.Sequential(Block(32, 32, "relu"), Block(32, 32, "relu"))
            self.lstm = nn.LSTM(32, 16, num_layers=1, batch_first=True, bidirectional=True)

    class Postnet(nn.Module):
        def __init__(self):
            super().__init__()
            self.convolutions = nn.ModuleList([Block(16, 32, "tanh"), Block(32, 32, "tanh"), Block(32, 16, None)])

    class Tiny(nn.Module):
        def __init__(self):
            super().__init__()
            self.embedding = nn.Embedding(100, 32)
            self.encoder = Encoder()
            self.postnet = Postnet()
            self.to_mel = nn.Linear(32, tu.D)
            self.post_in = nn.Linear(tu.D, 16)
            self.post_out = nn.Linear(16, tu.D)
            self.decoder = nn.Module()
            self.decoder.stopnet = nn.Linear(tu.D * tu.R, 1)
            self.seen = {}

        def _convs(self, part, convs, x):
            for i, block in enumerate(convs):
                rec = self.seen[(part, i)] = dict(x=x.detach().clone())
                x = block(x)
                rec["out"] = x.detach().clone()
                x.register_hook(lambda g, rec=rec: rec.__setitem__("grad_out", g.detach().clone()))
            return x

        def forward(self, text, text_lengths, mel, speaker_ids=None):
            x = self._convs("encoder", self.encoder.convolutions, self.embedding(text).transpose(1, 2))
            packed = nn.utils.rnn.pack_padded_sequence(x.transpose(1, 2), text_lengths.cpu().numpy(), batch_first=True)
            self.encoder.lstm.flatten_parameters()
            enc, _ = nn.utils.rnn.pad_packed_sequence(self.encoder.lstm(packed)[0], batch_first=True)
            pooled = enc.sum(1) / text_lengths.float()[:, None]
            dec = 0.5 * mel + self.to_mel(pooled)[:, None, :]
            p = self._convs("postnet", self.postnet.convolutions, self.post_in(dec).transpose(1, 2))
            post = dec + self.post_out(p.transpose(1, 2))
            nb, nt, nd = mel.shape
            stop = self.decoder.stopnet(dec.detach().reshape(nb, nt // tu.R, nd * tu.R)).squeeze(-1)
            return dec, post, torch.zeros(nb, nt // tu.R, text.shape[1], device=mel.device), stop

    torch.manual_seed(530)
    return Tiny()
