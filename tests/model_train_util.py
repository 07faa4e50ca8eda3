"""Shared by tests/golden/make_golden_model_train.py, test_model_train_cpu.py, test_gpu_model_train.py and
tools/model_train_report.py: the composed Tacotron2 of the training path (embedding -> three conv-BN blocks -> BiLSTM
-> teacher-forced decoder -> Postnet, wired as the reference's Tacotron2.forward wires them,
models/tacotron2.py:47-60) as a builder with the reference's state-dict keys and shapes, the cases of the
model_train.npz fixture (weights, token ids, mel targets, dropout masks and lengths regenerated from PCG64 seeds,
never stored), one training iteration in train_batch's order on any such model (``iterate``), its float64 twin on
the CPU with mutants, and the bound.

Bound.  Per tensor, relative to the tensor's OWN maximum:

    max |got - ref64| <= tol * max |ref64|,   tol = max(4e-6, 4 x the reference's float32-against-float64 figure)

The per-layer tests divide by max(1, max |ref64|); their upstream gradients are standard normal, so that form bites
there.  Under a real loss the gradients are small (max |grad| runs from a few 1e-4 to a few 1e-1 over the
parameters), and against such a tensor an absolute 4e-6 is a check of a percent: the mutant "query_99" (the query
layer's gradient scaled by 0.99) passes the max(1, .) form and fails this one (test_model_train_cpu.py).  The
reference's float32 figure is read from the fixture, never from a device run; four times is the margin the conv-BN
and decoder bounds keep over the reference's float32 run.  Two kinds of tensor are mathematically zero and are
judged against the size of what cancels instead of their own maximum: a conv bias gradient under batch norm
(convbn_train_util.bias_scale: S = max_c sum |dy|) and v's bias gradient under softmax (decoder_train_util.scale_of:
S = max_t sum |de|).  No other exception.
"""
import functools
import re
import zlib

import numpy as np

import convbn_train_util as cu
import decoder_train_util as du
import eval_util as eu

TOL = 4e-6
MARGIN = 4.0
SAMPLE = 256   # elements a tensor larger than this is stored at
MIN_Z = 1e-5   # every kept conv-BN (encoder) and prenet pre-activation is at least this far from the ReLU kink
ATTEMPTS = 200

REF = dict(du.REF, chars=130, post=512, nblocks=5)    # models/tacotron2.py:26-40 with 130 symbols
SMALL = dict(du.MODEL, chars=100, post=32, nblocks=3)  # decoder_train_util.small_model's
GROUPS = ("prenet", "att", "dec", "stop")
OUTPUTS = ("decoder_output", "postnet_output", "alignments", "stop_tokens")
SCALARS = ("decoder_loss", "postnet_loss", "stop_loss", "grad_norm", "grad_norm_st")
MUTANTS = ("no_residual", "stop_leaks", "one_upstream", "padded_rows", "query_99")
QUERY = "grad_decoder.attention_layer.query_layer.linear_layer.weight"


def _case(seed, dims, text_lens, mel_lens, r, norm="sigmoid", fwd=True, sep=True, masked=True):
    assert list(text_lens) == sorted(text_lens, reverse=True) and max(mel_lens) % r == 0
    return dict(seed=seed, dims=dims, text_lens=list(text_lens), mel_lens=list(mel_lens), frames=max(mel_lens), r=r,
                norm=norm, fwd=fwd, sep=sep, pdrop=True, masked=masked)


def _uneven(seed, n, top):
    v = [int(x) for x in np.random.Generator(np.random.PCG64(seed)).integers(1, top + 1, n)]
    v[0] = top
    return v


CASES = {
    "ref": _case(601, REF, [6, 5, 3], [10, 7, 4], 2),
    "joint": _case(602, REF, [6, 5, 3], [6, 4, 2], 1, norm="softmax", fwd=False, sep=False, masked=False),
    "b17": _case(603, REF, sorted(du._perm(611, 17), reverse=True), _uneven(612, 17, 3), 1),  # past one 16-row tile
    "l70": _case(604, REF, [70, 33, 1], [8, 5, 2], 2, sep=False),  # past one wave of positions, a length-1 sentence
    "small": _case(605, SMALL, [6, 5, 3], [10, 7, 4], 2),          # against the twin only
}
FIXTURE_CASES = [c for c in CASES if c != "small"]


def case_of(case):
    return CASES[case] if isinstance(case, str) else case


def options(case):
    c = case_of(case)
    return dict(dims=c["dims"], r=c["r"], norm=c["norm"], fwd=c["fwd"], sep=c["sep"], pdrop=c["pdrop"])


# ------------------------------------------------------------------ the state dict and the seeded inputs
def _block_keys(prefix, cin, cout):
    return [(f"{prefix}.net.0.weight", (cout, cin, 5)), (f"{prefix}.net.0.bias", (cout,)),
            (f"{prefix}.net.1.weight", (cout,)), (f"{prefix}.net.1.bias", (cout,)),
            (f"{prefix}.net.1.running_mean", (cout,)), (f"{prefix}.net.1.running_var", (cout,)),
            (f"{prefix}.net.1.num_batches_tracked", ())]


def postnet_channels(dims):
    n, mel, p = dims["nblocks"], dims["mel"], dims["post"]
    return [(mel if i == 0 else p, mel if i == n - 1 else p, None if i == n - 1 else "tanh") for i in range(n)]


def state_shapes(dims, r):
    """The reference Tacotron2's state-dict keys and shapes, in its order, at ``dims``."""
    E, H = dims["E"], dims["E"] // 2
    out = [("embedding.weight", (dims["chars"], E))]
    for i in range(3):
        out += _block_keys(f"encoder.convolutions.{i}", E, E)
    for s in ("", "_reverse"):
        out += [(f"encoder.lstm.weight_ih_l0{s}", (4 * H, E)), (f"encoder.lstm.weight_hh_l0{s}", (4 * H, H)),
                (f"encoder.lstm.bias_ih_l0{s}", (4 * H,)), (f"encoder.lstm.bias_hh_l0{s}", (4 * H,))]
    out += [("decoder." + n, s) for n, s in du.param_shapes(dims, r).items()]
    for i, (cin, cout, _) in enumerate(postnet_channels(dims)):
        out += _block_keys(f"postnet.convolutions.{i}", cin, cout)
    return dict(out)


def is_buffer(key):
    return key.endswith(("running_mean", "running_var", "num_batches_tracked"))


def param_keys(case):
    c = case_of(case)
    return [k for k in state_shapes(c["dims"], c["r"]) if not is_buffer(k)]


def tensor_names(case):
    return list(OUTPUTS) + ["grad_encoder_outputs"] + ["grad_" + k for k in param_keys(case)]


def _rng(c, attempt, tag):
    return np.random.Generator(np.random.PCG64([c["seed"], attempt, zlib.crc32(tag.encode())]))


def _weight(c, attempt, key, shape):
    g, d = _rng(c, attempt, key), c["dims"]
    u = lambda k: g.uniform(-k, k, shape).astype(np.float32)
    if key.endswith("num_batches_tracked"):
        return np.asarray(0, np.int64)
    if key.endswith("running_mean"):
        return np.zeros(shape, np.float32)
    if key.endswith("running_var"):
        return np.ones(shape, np.float32)
    if key == "embedding.weight":
        return u(np.sqrt(3.0) * np.sqrt(2.0 / (d["chars"] + d["E"])))  # models/tacotron2.py:29-31
    if ".net.0." in key:
        return u(1.0 / np.sqrt(5 * state_shapes(d, c["r"])[key.replace("bias", "weight")][1]))
    if key.endswith(".net.1.weight"):
        return g.uniform(0.5, 1.5, shape).astype(np.float32)
    if key.endswith(".net.1.bias"):
        return u(0.5)
    if key.startswith("encoder.lstm"):
        return u(1.0 / np.sqrt(d["E"] // 2))
    if "rnn.weight" in key or "rnn.bias" in key:  # the decoder's, by decoder_train_util's rule
        return u(1.0 / np.sqrt(d["R"]))
    if key.endswith("bias"):
        return u(0.1)
    if "init" in key:
        return u(1.0)
    return u(np.sqrt(6.0 / (shape[0] + shape[1])))


def mask_shapes(case):
    """{"encoder": [3 shapes [B, E, L]], "postnet": [shapes [B, C, frames]], and the decoder's four groups}."""
    c = case_of(case)
    d, B, L, F = c["dims"], len(c["text_lens"]), max(c["text_lens"]), c["frames"]
    out = dict(encoder=[(B, d["E"], L)] * 3, postnet=[(B, cout, F) for _, cout, _ in postnet_channels(d)])
    out.update(du.mask_shapes(d, c["r"], B, F // c["r"]))
    return out


P_DROP = dict(du.P_DROP, encoder=cu.P_DROP, postnet=cu.P_DROP)


def _draw_mask(c, attempt, tag, shape, p):
    return (_rng(c, attempt, "mask." + tag).random(shape) >= p).astype(np.uint8)


_KINK_KEYS = ["embedding.weight"] + [f"encoder.convolutions.{i}.net.{j}" for i in range(3)
                                     for j in ("0.weight", "0.bias", "1.weight", "1.bias")] + [
    "decoder." + du.PARAMS[0], "decoder." + du.PARAMS[1], "decoder.go_frame_init.weight"]


def _draw(c, attempt, keys=None):
    """The inputs of an attempt; ``keys`` limits the weights drawn (every tensor has a seed of its own, so a part
    is the same part of the whole)."""
    d, r = c["dims"], c["r"]
    B, L, F = len(c["text_lens"]), max(c["text_lens"]), c["frames"]
    shapes = state_shapes(d, r)
    weights = {k: _weight(c, attempt, k, shapes[k]) for k in (shapes if keys is None else keys)}
    g = _rng(c, attempt, "batch")
    text = g.integers(1, d["chars"], (B, L)).astype(np.int64)
    mel = g.uniform(0.0, 1.0, (B, F, d["mel"])).astype(np.float32)
    stop = np.zeros((B, F), np.float32)
    for b, (n, m) in enumerate(zip(c["text_lens"], c["mel_lens"])):
        text[b, n:] = 0
        stop[b, m - 1:] = 1.0  # (the mel frames past a length stay random: a zero frame puts the prenet ON the kink)
    ms = mask_shapes(c)
    masks = {k: [_draw_mask(c, attempt, f"{k}{i}", s, P_DROP[k]) for i, s in enumerate(ms[k])] for k in ("encoder", "postnet")}
    masks.update({k: _draw_mask(c, attempt, k, ms[k], P_DROP[k]) for k in GROUPS})
    return dict(case=c, weights=weights, text=text, text_lens=list(c["text_lens"]), mel=mel, mel_lens=list(c["mel_lens"]),
                stop=stop, stop_targets=eu.group_stop_targets(stop, r), masks=masks)


def min_kept_preactivation(inp):
    """min |z| in float64 over the kept pre-activations of the three encoder conv-BN blocks (batch statistics, as in
    training) and of the two prenet layers."""
    c, w = inp["case"], inp["weights"]
    x = w["embedding.weight"].astype(np.float64)[inp["text"]].transpose(0, 2, 1)
    low = np.inf
    for i in range(3):
        p = f"encoder.convolutions.{i}.net."
        blk = dict(W=w[p + "0.weight"], bias=w[p + "0.bias"], gamma=w[p + "1.weight"], beta=w[p + "1.bias"], act="relu")
        m = inp["masks"]["encoder"][i]
        x, s, _, _ = cu.block_forward(x, blk, m, 0.0, 1.0)
        low = min(low, float(np.abs(s["z"][m != 0]).min()))
    dec = dict(case=dict(lens=c["text_lens"], T=c["frames"] // c["r"], training=True, pdrop=c["pdrop"]),
               weights={n: w["decoder." + n] for n in (du.PARAMS[0], du.PARAMS[1], "go_frame_init.weight")},
               memories=inp["mel"], masks=inp["masks"])
    return min(low, du.min_kept_preactivation(dec))


def inputs(case):
    """dict(case, weights {state-dict key: array}, text int64 [B, L], text_lens, mel [B, frames, mel], mel_lens,
    stop [B, frames], stop_targets [B, frames / r], masks {"encoder": [..], "postnet": [..], "prenet", "att", "dec",
    "stop"}: uint8, 1 = keep).  Re-seeded until ``min_kept_preactivation`` is at least MIN_Z."""
    if isinstance(case, str):
        return _inputs_cached(case)
    for attempt in range(ATTEMPTS):
        if min_kept_preactivation(_draw(case, attempt, _KINK_KEYS)) >= MIN_Z:
            inp = _draw(case, attempt)
            inp["attempt"] = attempt
            return inp
    raise AssertionError(f"no seed within {ATTEMPTS} attempts keeps the model off the ReLU kink")


@functools.lru_cache(maxsize=None)
def _inputs_cached(name):
    return inputs(CASES[name])


def batch(inp, device="cpu"):
    """The case as datasets.collate_fn returns a batch (no linear features: Tacotron2 trains on mel)."""
    import torch
    B = len(inp["text_lens"])
    mel = torch.from_numpy(inp["mel"]).to(device)
    return (torch.from_numpy(inp["text"]), torch.LongTensor(inp["text_lens"]), [f"spk{b}" for b in range(B)], mel, mel,
            torch.LongTensor(inp["mel_lens"]), torch.from_numpy(inp["stop"]).to(device), [f"item{b}.wav" for b in range(B)])


def sample_indices(case, name, size):
    if size <= SAMPLE:
        return np.arange(size)
    seed = [CASES[case]["seed"], zlib.crc32(name.encode())]
    return np.sort(np.random.Generator(np.random.PCG64(seed)).choice(size, SAMPLE, replace=False))


def stored(case, name, t):
    flat = np.asarray(t).reshape(-1)
    return flat[sample_indices(case, name, flat.size)]


def key(case, name, what):
    return f"{case}__{name}__{what}"


# ------------------------------------------------------------------ the model
def build_model(dims, r=2, norm="sigmoid", fwd=True, sep=True, pdrop=True):
    """decoder_train_util.small_model at any dimensions and decoder options, with the reference Tacotron2's
    state-dict keys, shapes and order (``state_shapes``).  ``forward(text, text_lengths, mel, speaker_ids=None,
    masks=None)``: ``masks`` (``inputs()["masks"]`` as tensors) fixes every dropout mask; a conv-BN block of torch
    multiplies by ``mask / (1 - p)`` where its ``nn.Dropout`` stood, ``layers.ConvBNBlock`` and ``layers.Decoder``
    (after the swaps) take theirs as arguments.  With ``masks=None`` every layer draws its own.  ``mutant`` (None
    or one of MUTANTS' first four) breaks the model on purpose; ``encoder_outputs`` is the last forward's."""
    import torch
    from torch import nn
    from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence
    acts = {"relu": nn.ReLU, "tanh": nn.Tanh}

    class Block(nn.Module):  # layers/tacotron2.py:9-27
        def __init__(self, cin, cout, act):
            super().__init__()
            mods = [nn.Conv1d(cin, cout, 5, padding=2), nn.BatchNorm1d(cout)] + ([acts[act]()] if act else [])
            self.net = nn.Sequential(*mods, nn.Dropout(0.5))

        def forward(self, x, mask=None):
            if mask is None or not self.training:
                return self.net(x)
            for mod in self.net[:-1]:
                x = mod(x)
            return x * (mask.to(x.dtype) / (1.0 - self.net[-1].p))

    def chain(blocks, x, masks):
        for i, block in enumerate(blocks):
            x = block(x) if masks is None else block(x, mask=masks[i])
        return x

    class Encoder(nn.Module):  # layers/tacotron2.py:48-76
        def __init__(self):
            super().__init__()
            E = dims["E"]
            self.convolutions = nn.Sequential(*[Block(E, E, "relu") for _ in range(3)])
            self.lstm = nn.LSTM(E, E // 2, num_layers=1, batch_first=True, bidirectional=True)
            self.mutant = None

        def forward(self, x, input_lengths, masks=None):
            x = chain(self.convolutions, x, masks).transpose(1, 2)
            packed = pack_padded_sequence(x, input_lengths.cpu().numpy(), batch_first=True)
            self.lstm.flatten_parameters()
            out = pad_packed_sequence(self.lstm(packed)[0], batch_first=True)[0]
            if self.mutant == "padded_rows":
                # The forward direction's backward walks the padded rows too (same values: a - a is 0), and the
                # gradient that arrives there is the sentence's first row's where zeros belong.
                H = self.lstm.hidden_size
                walked = self.lstm(x)[0][..., :H]
                out = torch.cat([out[..., :H].detach() + (walked - walked.detach()), out[..., H:]], -1)
                valid = (torch.arange(x.shape[1])[None, :] < input_lengths.cpu()[:, None])[:, :, None].to(x.device)
                out.register_hook(lambda g: torch.where(valid, g, g[:, :1]))
            return out

    class Postnet(nn.Module):  # layers/tacotron2.py:30-45
        def __init__(self):
            super().__init__()
            self.convolutions = nn.ModuleList([Block(*ch) for ch in postnet_channels(dims)])

        def forward(self, x, masks=None):
            return chain(self.convolutions, x, masks)

    class Model(nn.Module):  # models/tacotron2.py:11-60
        def __init__(self):
            super().__init__()
            self.embedding = nn.Embedding(dims["chars"], dims["E"])
            self.encoder = Encoder()
            self.decoder = du.torch_decoder(dict(dims=dims, r=r, norm=norm, fwd=fwd, sep=sep, pdrop=pdrop))
            self.postnet = Postnet()
            self.mutant, self.encoder_outputs = None, None

        def forward(self, text, text_lengths, mel, speaker_ids=None, masks=None):
            self.encoder.mutant = self.mutant
            mask = torch.arange(text.shape[1], device=text.device)[None, :] < text_lengths.to(text.device)[:, None]
            enc = self.encoder(self.embedding(text).transpose(1, 2), text_lengths, None if masks is None else masks["encoder"])
            if enc.requires_grad:
                enc.retain_grad()
            self.encoder_outputs = enc
            if masks is None:
                dec, stop, align = self.decoder(enc, mel, mask)
            else:
                dec, stop, align = self.decoder(enc, mel, mask, {k: masks[k] for k in GROUPS})
            post = self.postnet(dec, None if masks is None else masks["postnet"])
            if self.mutant != "no_residual":
                post = dec + post
            return dec.transpose(1, 2), post.transpose(1, 2), align, stop

    return Model()


def model_for(case, weights=None, dtype=None):
    """``build_model`` for a case in ``train()`` mode, optionally with a state dict of arrays loaded and cast."""
    import torch
    m = build_model(**options(case))
    if weights is not None:
        m.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in weights.items()})
    return (m if dtype is None else m.to(dtype)).train()


def tensor_masks(masks, device="cpu"):
    import torch
    t = lambda a: torch.as_tensor(a).to(device)
    return {k: [t(a) for a in v] if isinstance(v, (list, tuple)) else t(v) for k, v in masks.items()}


def device_masks(model):
    """The masks every device layer drew in its last forward (``last_mask`` / ``last_masks``), as ``inputs()["masks"]``."""
    out = dict(encoder=[b.last_mask for b in model.encoder.convolutions],
               postnet=[b.last_mask for b in model.postnet.convolutions])
    out.update(model.decoder.last_masks)
    return {k: [a.cpu().numpy() for a in v] if isinstance(v, list) else v.cpu().numpy() for k, v in out.items()}


# ------------------------------------------------------------------ the criteria in float64, differentiable
def mse64(x, y, lengths=None):
    """eval_util.elementwise_loss("mse", ...) as a float64 graph: (loss tensor, its value)."""
    import torch
    x, y = x.double(), y.double()
    B, T, D = x.shape
    if lengths is None:
        loss = ((x - y) ** 2).sum() / (B * T * D)
    else:
        rows = torch.as_tensor(lengths).clamp(max=T)
        m = (torch.arange(T)[None, :] < rows[:, None])[:, :, None].to(x.device)
        loss = (((x - y) ** 2) * m).sum() / (int(rows.sum()) * D)
    return loss, float(loss.detach())


def bce64(x, y):
    """eval_util.bce_with_logits as a float64 graph: (loss tensor, its value)."""
    import torch
    x, y = x.double().reshape(-1), y.double().reshape(-1)
    loss = (x.clamp(min=0) - x * y + torch.log1p(torch.exp(-x.abs()))).sum() / x.numel()
    return loss, float(loss.detach())


def _norm(grads):
    return float(np.sqrt(sum(float((g.detach().double() ** 2).sum()) for g in grads if g is not None)))


def iterate(model, inp, masks, mse=mse64, bce=bce64, mutant=None):
    """One training iteration in train.train_batch's order, without the optimizers: zero the gradients, the forward
    with ``masks`` (tensors on the model's device, or None), the criteria, ``loss.backward()``, and
    ``stop_loss.backward()`` for a separate stopnet.  Returns {the four OUTPUTS, grad_encoder_outputs, grad_<key> for
    every parameter (zeros where autograd left None), the SCALARS, loss}: numpy arrays and floats.  ``grad_norm`` is
    the norm over all parameters after the first backward, ``grad_norm_st`` the stopnet's after the second (0 without
    a separate stopnet)."""
    import torch
    c = inp["case"]
    dev = next(model.parameters()).device
    model.zero_grad(set_to_none=True)
    model.mutant = mutant if mutant in ("no_residual", "padded_rows") else None
    text, lens = torch.from_numpy(inp["text"]).to(dev), torch.LongTensor(inp["text_lens"]).to(dev)
    mel = torch.from_numpy(inp["mel"]).to(dev).to(next(model.parameters()).dtype)
    targets = torch.from_numpy(inp["stop_targets"]).to(dev)
    dec, post, align, stop = model(text, lens, mel, speaker_ids=None, masks=masks)
    length = (torch.LongTensor(inp["mel_lens"]),) if c["masked"] else ()
    stop_loss, stop_value = bce(stop, targets)
    decoder_loss, decoder_value = mse(dec.detach() if mutant == "one_upstream" else dec, mel, *length)
    postnet_loss, postnet_value = mse(post, mel, *length)
    loss, value = decoder_loss + postnet_loss, decoder_value + postnet_value
    if not c["sep"]:
        loss, value = loss + stop_loss, value + stop_value
    loss.backward(retain_graph=mutant == "stop_leaks")
    r = dict(zip(OUTPUTS, (dec, post, align, stop)))
    r.update(decoder_loss=decoder_value, postnet_loss=postnet_value, stop_loss=stop_value, loss=value,
             grad_norm=_norm(p.grad for p in model.parameters()), grad_norm_st=0.0)
    if c["sep"]:
        stop_loss.backward()
        r["grad_norm_st"] = _norm(p.grad for p in model.decoder.stopnet.parameters())
    r["grad_encoder_outputs"] = model.encoder_outputs.grad
    for k, p in model.named_parameters():
        r["grad_" + k] = p.grad if p.grad is not None else torch.zeros_like(p)
    out = {k: (v.detach().cpu().numpy().copy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}
    if mutant == "query_99":
        out[QUERY] = out[QUERY] * 0.99
    return out


# ------------------------------------------------------------------ the float64 twin
class Twin:
    """The model in float64 on the CPU with explicit masks; ``run`` is ``iterate`` plus the scales of the tensors
    that are mathematically zero (S_enc{i}, S_post{i}: max_c sum |dy| at the conv output of each block; S_de: max over
    steps of sum |de| at the energies) and ``buffers`` (the batch-norm statistics after the forward)."""

    def __init__(self, case, weights=None):
        self.case = case_of(case)
        self.model = model_for(self.case, weights, dtype=None)
        self.model.double()
        self.scales = {}
        for part, convs in (("enc", self.model.encoder.convolutions), ("post", self.model.postnet.convolutions)):
            for i, block in enumerate(convs):
                block.net[0].register_forward_hook(functools.partial(self._tap, f"S_{part}{i}", lambda g: g.abs().sum((0, 2)).max()))
        self.model.decoder.attention_layer.v.register_forward_hook(functools.partial(self._tap, "S_de", lambda g: g.abs().sum()))

    def _tap(self, name, reduce, module, args, output):
        if output.requires_grad:
            output.register_hook(lambda g: self.scales.__setitem__(name, max(self.scales.get(name, 0.0), float(reduce(g)))))

    def load(self, state_dict):
        """Parameters and buffers from a state dict of tensors or arrays of any float type."""
        import torch
        own = self.model.state_dict()
        self.model.load_state_dict({k: torch.as_tensor(np.asarray(v.detach().cpu() if hasattr(v, "detach") else v)).to(own[k].dtype)
                                    for k, v in state_dict.items()})

    def run(self, inp, masks=None, mutant=None):
        self.scales.clear()
        self.model.decoder.separate_stopnet = self.case["sep"] and mutant != "stop_leaks"
        r = iterate(self.model, inp, tensor_masks(inp["masks"] if masks is None else masks), mutant=mutant)
        self.model.decoder.separate_stopnet = self.case["sep"]
        r.update(self.scales)
        r["buffers"] = {k: v.numpy().copy() for k, v in self.model.state_dict().items() if is_buffer(k)}
        return r


@functools.lru_cache(maxsize=None)
def twin(case, mutant=None):
    """``Twin(case).run(inputs(case))`` for a named case, computed once and shared; do not modify."""
    inp = inputs(case)
    return Twin(case, inp["weights"]).run(inp, mutant=mutant)


def torch32(case):
    """The same iteration of the float32 torch model on the CPU (float64 criteria): what the reference alone gives."""
    inp = inputs(case)
    return iterate(model_for(case, inp["weights"]), inp, tensor_masks(inp["masks"]))


# ------------------------------------------------------------------ the bound
_BIAS = re.compile(r"grad_(encoder|postnet)\.convolutions\.(\d+)\.net\.0\.bias$")


def scale_of(case, name, twin_result):
    """The magnitude a mathematically zero tensor is judged against (None: the tensor's own maximum): a conv bias
    gradient under batch norm by convbn_train_util.bias_scale, v's bias gradient under softmax by
    decoder_train_util.scale_of."""
    m = _BIAS.match(name)
    if m:
        part = "enc" if m.group(1) == "encoder" else "post"
        return cu.bias_scale("grad_bias" + m.group(2), {"S" + m.group(2): twin_result[f"S_{part}{m.group(2)}"]})
    if name.startswith("grad_decoder."):
        return du.scale_of(dict(norm=case_of(case)["norm"]), "grad_" + name[len("grad_decoder."):], twin_result)
    return None


def ratio(got, ref64, scale=None):
    """max |got - ref64| / max |ref64| (``scale`` in its place when given): within the bound when <= tol."""
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    diff = float(np.abs(got - ref64).max()) if got.size else 0.0
    den = float(np.abs(ref64).max()) if scale is None else float(scale)
    if den == 0.0:
        return 0.0 if diff == 0.0 else float("inf")
    return diff / den


def tolerance(own):
    """4e-6, or 4x the reference's own float32-against-float64 figure for this case and tensor when that is larger."""
    return max(TOL, MARGIN * float(own))


def figure(got, ref64, what, tol=TOL, scale=None):
    """Prints the figure and returns it (inf for non-finite values); asserts nothing."""
    v = ratio(got, ref64, scale)
    if not np.isfinite(np.asarray(got, np.float64)).all():
        v = float("inf")
    print(f"{what}: max|got - ref64| / {'max|ref64|' if scale is None else 'scale'} = {v:.3e} (bound {tol:.1e})")
    return v


def check(got, ref64, what, tol=TOL, scale=None):
    """Prints the figure, then asserts the bound.  Returns the ratio."""
    v = figure(got, ref64, what, tol, scale)
    assert v <= tol, f"{what}: {v:.3e} above {tol:.1e}"
    return v


def scalar(v):
    return np.asarray(float(v), np.float64)


def compare(case, got, twin_result, fixture, report=None, what="device"):
    """Every tensor of ``tensor_names(case)`` and every scalar of ``got`` against the twin and, for a fixture case,
    against the reference's float64 run at the stored sample (judged against the whole tensor's maximum, the twin's:
    the sample's can be smaller); a scalar is judged relative to its own value.  The tolerance is ``tolerance`` of the
    fixture's float32 figure for the case and the tensor (4e-6 for a case the fixture does not hold).  Prints every
    figure, then asserts that none is above its bound.  ``report`` (a dict) receives {name: (the larger of the two
    figures, bound)} before the assertion."""
    held = fixture is not None and case in FIXTURE_CASES
    above = []
    for name in tensor_names(case) + list(SCALARS):
        scale = scale_of(case, name, twin_result)
        tol = tolerance(fixture[key(case, name, "ref32")]) if held else TOL
        g, t = (scalar(got[name]), scalar(twin_result[name])) if name in SCALARS else (got[name], twin_result[name])
        v = figure(g, t, f"{what} {case} {name} vs the twin", tol, scale)
        if held:
            whole = (float(np.abs(t).max()) if scale is None else scale) if name not in SCALARS else None
            v = max(v, figure(g if name in SCALARS else stored(case, name, g), fixture[key(case, name, 64)],
                              f"{what} {case} {name} vs the reference", tol, whole))
        if report is not None:
            report[name] = (v, tol)
        if not v <= tol:
            above.append(f"{name}: {v:.3e} above {tol:.1e}")
    assert not above, f"{what} {case}: " + "; ".join(above)


# ------------------------------------------------------------------ the model on the device
def device_model(case, layers, weights):
    """The case's model on the device in ``train()`` mode with the three swaps applied (``layers``: the package's)."""
    m = model_for(case, weights).cuda().train()
    layers.use_device_decoder(layers.use_device_convs(layers.use_device_lstm(m)))
    assert isinstance(m.decoder, layers.Decoder) and isinstance(m.encoder.lstm, layers.LSTM)
    assert all(isinstance(b, layers.ConvBNBlock) for b in list(m.encoder.convolutions) + list(m.postnet.convolutions))
    return m


def package_criteria(losses, masked):
    """The package's criteria in ``iterate``'s form: (loss tensor, the criterion's fp64 value)."""
    crit, crit_st = (losses.MSELossMasked() if masked else losses.MSELoss()), losses.BCEWithLogitsLoss()

    def mse(x, y, *length):
        loss = crit(x, y, *length)
        return loss, crit.last_value

    def bce(x, y):
        loss = crit_st(x, y)
        return loss, crit_st.last_value

    return mse, bce


def device_iterate(case, layers, losses):
    """``iterate`` of a fresh device model with the case's weights and masks and the package's criteria."""
    inp = inputs(case)
    mse, bce = package_criteria(losses, case_of(case)["masked"])
    return iterate(device_model(case, layers, inp["weights"]), inp, tensor_masks(inp["masks"], "cuda"), mse, bce)


