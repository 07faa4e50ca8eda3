"""Shared by tests/golden/make_golden_decoder_train.py, test_decoder_train_cpu.py, test_gpu_decoder_train.py and
tools/bench_decoder_train.py: the cases of the decoder_train.npz fixture (inputs, weights, dropout masks and
upstream gradients regenerated from seeds, never stored), the index sample the large tensors are stored at, a
float64 numpy restatement of the forward and the backward of the reference's teacher-forced Decoder
(layers/tacotron2.py:97-247 with the attention of layers/common_layers.py:107-256), a torch restatement with
explicit masks (``TorchDecoder``: the bench's baseline and the source of ``layers.use_device_decoder``), and the
bound.

Bound.  The project's form, per tensor:  max |got - ref64| <= tol * max(1, max |ref64|)  with tol = 4e-6 (the
model-half tolerance of lstm_train_util.py), or four times the reference's own float32-against-float64 figure for
that case and tensor where that is larger (read from the fixture, never from a device run; four times is the margin
by which the existing bounds sit over the reference's float32 run: 5x for the LSTM, 4x for the conv-BN block).  The
gradient of v's bias under softmax is mathematically zero (softmax ignores a shift of the energies); it is judged
against S = max_t sum_{b,l} |de64| in place of its own magnitude, as the conv bias gradient is under batch norm.
"""
import functools

import numpy as np

TOL = 4e-6
MARGIN = 4.0
KC = 512      # DT_KC of csrc/decoder_train.hip: rows per reduction chunk of the weight gradients
SAMPLE = 400  # elements a tensor larger than this is stored at
MIN_Z = 1e-5  # every kept prenet pre-activation is at least this far from the ReLU kink in float64

REF = dict(E=512, PN=256, R=1024, A=128, mel=80)
SMALL = dict(E=32, PN=16, R=48, A=16, mel=8)

# the reference's parameter names (state-dict keys) in the order of tts_dectrain_weights
PARAMS = (
    "prenet.layers.0.linear_layer.weight", "prenet.layers.1.linear_layer.weight",
    "attention_rnn.weight_ih", "attention_rnn.weight_hh", "attention_rnn.bias_ih", "attention_rnn.bias_hh",
    "attention_layer.query_layer.linear_layer.weight", "attention_layer.inputs_layer.linear_layer.weight",
    "attention_layer.v.linear_layer.weight", "attention_layer.v.linear_layer.bias",
    "decoder_rnn.weight_ih", "decoder_rnn.weight_hh", "decoder_rnn.bias_ih", "decoder_rnn.bias_hh",
    "linear_projection.linear_layer.weight", "linear_projection.linear_layer.bias",
    "stopnet.1.linear_layer.weight", "stopnet.1.linear_layer.bias",
    "attention_rnn_init.weight", "go_frame_init.weight", "decoder_rnn_inits.weight")
V_BIAS = "grad_attention_layer.v.linear_layer.bias"


def _perm(seed, n):
    return [int(v) for v in np.random.Generator(np.random.PCG64(seed)).permutation(np.arange(1, n + 1))]


def _ints(seed, lo, hi, n):
    return [int(v) for v in np.random.Generator(np.random.PCG64(seed)).integers(lo, hi, n)]


def _case(seed, lens, T, r=1, norm="sigmoid", fwd=True, sep=True, pdrop=True, training=True, dims=REF):
    return dict(seed=seed, lens=lens, T=T, r=r, norm=norm, fwd=fwd, sep=sep, pdrop=pdrop, training=training, dims=dims)


CASES = {
    "one": _case(501, [1], 1),
    "t6": _case(502, [9, 6, 4], 6),
    "softmax_r2": _case(503, [9, 6, 4], 6, r=2, norm="softmax", fwd=False, sep=False),
    "r2_fwd": _case(504, [33, 20, 7, 1], 12, r=2, sep=False),
    "t24": _case(505, [17, 5], 24),                       # a long chain
    "b17": _case(506, _perm(511, 17), 3),                 # past one 16-row tile
    "l70": _case(507, [70, 33, 1], 4),                    # past one wave of positions
    "chunks": _case(508, _ints(512, 2, 10, 24), 24),      # B * T past one reduction chunk, not a multiple of it
    "nodrop": _case(509, [9, 6, 4], 6, pdrop=False),
    "eval": _case(510, [9, 6, 4], 6, training=False),     # forward only
    "small": _case(520, [5, 3], 4, r=3, sep=False, dims=SMALL),  # against the restatement only
}
assert KC < len(CASES["chunks"]["lens"]) * CASES["chunks"]["T"] < 2 * KC
assert (len(CASES["chunks"]["lens"]) * CASES["chunks"]["T"]) % KC
FIXTURE_CASES = [c for c in CASES if c != "small"]
BENCH = _case(530, _ints(421, 40, 151, 32), 400)  # the LSTM bench's text lengths


def case_of(case):
    return CASES[case] if isinstance(case, str) else case


def param_shapes(dims, r):
    E, PN, R, A, MR = dims["E"], dims["PN"], dims["R"], dims["A"], dims["mel"] * r
    return dict(zip(PARAMS, ((PN, MR), (PN, PN), (4 * R, PN + E), (4 * R, R), (4 * R,), (4 * R,), (A, R), (A, E), (1, A),
                             (1,), (4 * R, R + E), (4 * R, R), (4 * R,), (4 * R,), (MR, R + E), (MR,), (1, R + MR), (1,),
                             (1, R), (1, MR), (1, R))))


def mask_shapes(dims, r, B, T):
    R, PN, MR = dims["R"], dims["PN"], dims["mel"] * r
    return dict(prenet=(2, T, B, PN), att=(2, T, B, R), dec=(2, T, B, R), stop=(T, B, R + MR))


P_DROP = dict(prenet=0.5, att=0.1, dec=0.1, stop=0.1)


def tensor_names(case):
    c = case_of(case)
    names = ["outputs", "stop_tokens", "alignments"]
    if c["training"]:
        names += ["grad_inputs", "grad_memories"] + ["grad_" + n for n in PARAMS]
    return names


def _draw(c, attempt):
    g = np.random.Generator(np.random.PCG64([c["seed"], attempt]))
    d, r, lens, T = c["dims"], c["r"], c["lens"], c["T"]
    B, L, mel = len(lens), max(lens), d["mel"]
    weights = {}
    for name, shape in param_shapes(d, r).items():
        if "rnn.weight" in name or "rnn.bias" in name:
            k = 1.0 / np.sqrt(d["R"])
        elif name.endswith("bias"):
            k = 0.1
        elif "init" in name:
            k = 1.0
        else:
            k = np.sqrt(6.0 / (shape[0] + shape[1]))
        weights[name] = g.uniform(-k, k, shape).astype(np.float32)
    inputs_ = g.standard_normal((B, L, d["E"])).astype(np.float32)  # the masked rows too
    memories = g.standard_normal((B, T * r, mel)).astype(np.float32)
    mask = (np.arange(L)[None, :] < np.asarray(lens)[:, None]).astype(np.uint8)
    masks = None
    if c["training"]:
        masks = {k: (g.random(s) >= P_DROP[k]).astype(np.uint8) for k, s in mask_shapes(d, r, B, T).items()}
    up = dict(outputs=g.standard_normal((B, mel, T * r)).astype(np.float32),
              stop_tokens=g.standard_normal((B, T)).astype(np.float32))
    return dict(inputs=inputs_, memories=memories, mask=mask, masks=masks, weights=weights, up=up, lens=list(lens),
                case=c)


def _frames(inp, go):
    c = inp["case"]
    B, T = len(c["lens"]), c["T"]
    fr = inp["memories"].astype(np.float64).reshape(B, T, -1).transpose(1, 0, 2)
    return np.concatenate([np.broadcast_to(go, (1, B, go.shape[-1])), fr], 0)[:T]


def _prenet(inp, mutant=None):
    """(frames, z1, h1, z2, h2, m1, m2) in float64, [T, B, .]."""
    c, w = inp["case"], inp["weights"]
    go = w["go_frame_init.weight"].astype(np.float64)
    fr = _frames(inp, go * 0 if mutant == "zero_go" else go)
    drop = c["training"] and c["pdrop"]
    m1 = inp["masks"]["prenet"][0] * 2.0 if drop else 1.0
    m2 = inp["masks"]["prenet"][1] * 2.0 if drop else 1.0
    z1 = fr @ w[PARAMS[0]].astype(np.float64).T
    h1 = np.maximum(z1, 0) * m1
    z2 = h1 @ w[PARAMS[1]].astype(np.float64).T
    h2 = np.maximum(z2, 0) * m2
    return fr, z1, h1, z2, h2, m1, m2


def min_kept_preactivation(inp):
    _, z1, _, z2, _, m1, m2 = _prenet(inp)
    k1 = np.abs(z1[np.broadcast_to(m1, z1.shape) != 0]) if not np.isscalar(m1) else np.abs(z1)
    k2 = np.abs(z2[np.broadcast_to(m2, z2.shape) != 0]) if not np.isscalar(m2) else np.abs(z2)
    return float(min(k1.min(), k2.min()))


@functools.lru_cache(maxsize=None)
def _inputs_cached(name):
    return inputs(CASES[name])


def inputs(case):
    """dict(inputs [B, L, E], memories [B, T * r, mel], mask uint8 [B, L], masks {group: uint8} or None, weights
    {name: array}, up {outputs, stop_tokens}: the upstream gradients, lens, case), float32.  Re-seeded until every kept
    prenet pre-activation is at least MIN_Z from the ReLU kink in float64."""
    if isinstance(case, str):
        return _inputs_cached(case)
    for attempt in range(2000):
        inp = _draw(case, attempt)
        if min_kept_preactivation(inp) >= MIN_Z:
            inp["attempt"] = attempt
            return inp
    raise AssertionError("no seed keeps the prenet off the ReLU kink")


def sample_indices(case, name, size):
    if size <= SAMPLE:
        return np.arange(size)
    seed = CASES[case]["seed"] * 1000 + sum(ord(ch) for ch in name)
    return np.sort(np.random.Generator(np.random.PCG64(seed)).choice(size, SAMPLE, replace=False))


def stored(case, name, t):
    flat = np.asarray(t).reshape(-1)
    return flat[sample_indices(case, name, flat.size)]


def key(case, name, bits):
    return f"{case}__{name}__{bits}"


# ------------------------------------------------------------------ the decoder, restated in float64
def _sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


def _cell(x, h, c, w_ih, w_hh, b):
    pre = x @ w_ih.T + h @ w_hh.T + b
    H = h.shape[1]
    i, f, g, o = _sigmoid(pre[:, :H]), _sigmoid(pre[:, H:2 * H]), np.tanh(pre[:, 2 * H:3 * H]), _sigmoid(pre[:, 3 * H:])
    cn = f * c + i * g
    tc = np.tanh(cn)
    return o * tc, cn, (i, f, g, o, tc, c)


def _cell_back(dh_d, dc_d, mh, mc, saved):
    i, f, g, o, tc, c_prev = saved
    dh = dh_d * mh
    dc = dc_d * mc + dh * o * (1 - tc * tc)
    dpre = np.concatenate([dc * g * i * (1 - i), dc * c_prev * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)], 1)
    return dpre, dc * f


def restate(inp, up=None, mutant=None):
    """Forward and backward in float64 from the float32 operands of ``inputs()``: every tensor of ``tensor_names()``
    plus "S_de" (max_t sum_{b,l} |de|, the scale v's bias gradient is judged against).  ``up`` overrides the upstream
    gradients.  ``mutant`` breaks it on purpose (test_decoder_train_cpu.py): "cell_not_carried" carries the cell
    state before its dropout, "no_shift" leaves the shift out of forward attention, "mask_joins" lets masked
    positions into the normalisation, "att_ctx_t" pairs the attention LSTM's context input with ctx_t where ctx_{t-1}
    went in (its weight gradient), "stop_attached" lets the stopnet's input gradient through under separate_stopnet,
    "zero_go" puts zeros in place of the go frame, "dec_ctx_prev" feeds the decoder cell ctx_{t-1} in the forward (the
    context one step late: the forward's pairing of context and cell, which "att_ctx_t" cannot reach, since ctx_t does
    not exist yet when the attention cell of step t runs)."""
    c = inp["case"]
    d, r, T, lens = c["dims"], c["r"], c["T"], inp["lens"]
    E, PN, R, A, mel = d["E"], d["PN"], d["R"], d["A"], d["mel"]
    MR, B = mel * r, len(lens)
    W = {k: v.astype(np.float64) for k, v in inp["weights"].items()}
    (w1, w2, a_ih, a_hh, a_bi, a_bh, wq, wi, wv, bv, d_ih, d_hh, d_bi, d_bh, wpj, bpj, ws, bs, ia, go, idc) = (
        W[n] for n in PARAMS)
    train = c["training"]
    valid = inp["mask"].astype(bool)
    x_in = np.where(valid[:, :, None], inp["inputs"].astype(np.float64), 0.0)
    L = x_in.shape[1]
    nvalid = np.ones_like(valid) if mutant == "mask_joins" else valid
    fr, z1, h1, z2, h2, m1, m2 = _prenet(inp, mutant)
    ones = lambda n: np.ones((T, B, n))
    s_rnn, s_st = 1 / 0.9, 1 / 0.9
    if train:
        mk = inp["masks"]
        mah, mac, mdh, mdc, mst = (mk["att"][0] * s_rnn, mk["att"][1] * s_rnn, mk["dec"][0] * s_rnn, mk["dec"][1] * s_rnn,
                                   mk["stop"] * s_st)
    else:
        mah, mac, mdh, mdc, mst = ones(R), ones(R), ones(R), ones(R), ones(R + MR)
    Pm = x_in @ wi.T
    h_a, c_a = np.broadcast_to(ia, (B, R)).copy(), np.zeros((B, R))
    h_d, c_d = np.broadcast_to(idc, (B, R)).copy(), np.zeros((B, R))
    ctx = np.zeros((B, E))
    alpha = np.concatenate([np.ones((B, 1)), np.full((B, L - 1), 1e-7)], 1)
    sv = []
    dec_out, stops, aligns = np.zeros((T, B, MR)), np.zeros((T, B)), np.zeros((T, B, L))
    for t in range(T):
        s = dict(ctx_prev=ctx, ha_prev=h_a, hd_prev=h_d)
        h, cn, s["cell_a"] = _cell(np.concatenate([h2[t], ctx], 1), h_a, c_a, a_ih, a_hh, a_bi + a_bh)
        h_a, c_a = h * mah[t], (cn if mutant == "cell_not_carried" else cn * mac[t])
        q = h_a @ wq.T
        th = np.tanh(q[:, None, :] + Pm)
        e = th @ wv[0] + bv[0]
        if c["norm"] == "softmax":
            sg = np.where(nvalid, np.exp(e - np.where(nvalid, e, -np.inf).max(1, keepdims=True)), 0.0)
        else:
            sg = np.where(nvalid, _sigmoid(e), 0.0)
        S = sg.sum(1, keepdims=True)
        al = sg / S
        if c["fwd"]:
            shifted = alpha if mutant == "no_shift" else np.concatenate([np.zeros((B, 1)), alpha[:, :-1]], 1)
            w = 0.5 * alpha + 0.5 * shifted + 1e-8
            u = w * al
            S2 = u.sum(1, keepdims=True)
            s.update(w=w, S2=S2)
            alpha = u / S2
        else:
            alpha = al
        ctx = np.einsum("bl,ble->be", alpha, x_in)
        s.update(ha=h_a, th=th, sg=sg, S=S, al=al, alpha=alpha, ctx=ctx)
        ctx_dec = s["ctx_prev"] if mutant == "dec_ctx_prev" else ctx
        h, cn, s["cell_d"] = _cell(np.concatenate([h_a, ctx_dec], 1), h_d, c_d, d_ih, d_hh, d_bi + d_bh)
        h_d, c_d = h * mdh[t], (cn if mutant == "cell_not_carried" else cn * mdc[t])
        s["hd"] = h_d
        dec_out[t] = np.concatenate([h_d, ctx], 1) @ wpj.T + bpj
        s["xs"] = np.concatenate([h_d, dec_out[t]], 1) * mst[t]
        stops[t] = s["xs"] @ ws[0] + bs[0]
        aligns[t] = alpha
        sv.append(s)
    res = {"outputs": dec_out.transpose(1, 0, 2).reshape(B, T * r, mel).transpose(0, 2, 1),
           "stop_tokens": stops.T.copy(), "alignments": aligns.transpose(1, 0, 2).copy()}
    if not train:
        return res
    up = inp["up"] if up is None else up
    d_out = np.asarray(up["outputs"], np.float64).transpose(0, 2, 1).reshape(B, T, MR).transpose(1, 0, 2).copy()
    d_stop = np.asarray(up["stop_tokens"], np.float64).T
    G = {n: np.zeros_like(W[n]) for n in PARAMS}
    g_in, dP = np.zeros_like(x_in), np.zeros_like(Pm)
    dx = np.zeros((T, B, PN))
    dha, dca, dhd, dcd, dctx_c, dal_c = (np.zeros((B, R)), np.zeros((B, R)), np.zeros((B, R)), np.zeros((B, R)),
                                         np.zeros((B, E)), np.zeros((B, L)))
    attached = (not c["sep"]) or mutant == "stop_attached"
    S_de = 0.0
    for t in range(T - 1, -1, -1):
        s = sv[t]
        G[PARAMS[16]] += (d_stop[t] @ s["xs"])[None]
        G[PARAMS[17]] += d_stop[t].sum()
        do = d_out[t].copy()
        dh_dec = dhd.copy()
        if attached:
            dxs = d_stop[t][:, None] * ws * mst[t]
            dh_dec += dxs[:, :R]
            do += dxs[:, R:]
        hc = np.concatenate([s["hd"], s["ctx"]], 1)
        G[PARAMS[14]] += do.T @ hc
        G[PARAMS[15]] += do.sum(0)
        dhc = do @ wpj
        dh_dec += dhc[:, :R]
        dpre, dcd = _cell_back(dh_dec, dcd, mdh[t], mdc[t], s["cell_d"])
        G[PARAMS[10]] += dpre.T @ np.concatenate([s["ha"], s["ctx"]], 1)
        G[PARAMS[11]] += dpre.T @ s["hd_prev"]
        G[PARAMS[12]] += dpre.sum(0)
        G[PARAMS[13]] += dpre.sum(0)
        dxin = dpre @ d_ih
        dhd = dpre @ d_hh
        dh_att = dxin[:, :R] + dha
        dctx = dxin[:, R:] + dhc[:, R:] + dctx_c
        dalpha = dal_c + np.einsum("be,ble->bl", dctx, x_in)
        g_in += s["alpha"][:, :, None] * dctx[:, None, :]
        if c["fwd"]:
            du = (dalpha - (dalpha * s["alpha"]).sum(1, keepdims=True)) / s["S2"]
            da, dw = du * s["w"], du * s["al"]
            if mutant == "no_shift":
                dal_c = dw
            else:
                dal_c = 0.5 * dw + 0.5 * np.concatenate([dw[:, 1:], np.zeros((B, 1))], 1)
        else:
            da = dalpha
        inner = (da * s["al"]).sum(1, keepdims=True)
        if c["norm"] == "softmax":
            de = s["al"] * (da - inner)
        else:
            de = (da - inner) / s["S"] * s["sg"] * (1 - s["sg"])
        de = np.where(nvalid, de, 0.0)
        S_de = max(S_de, float(np.abs(de).sum()))
        dth = de[:, :, None] * wv[0] * (1 - s["th"] ** 2)
        dq = dth.sum(1)
        dP += dth
        G[PARAMS[8]] += np.einsum("bl,bla->a", de, s["th"])[None]
        G[PARAMS[9]] += de.sum()
        G[PARAMS[6]] += dq.T @ s["ha"]
        dh_att += dq @ wq
        dpre, dca = _cell_back(dh_att, dca, mah[t], mac[t], s["cell_a"])
        ctx_in = s["ctx"] if mutant == "att_ctx_t" else s["ctx_prev"]
        G[PARAMS[2]] += dpre.T @ np.concatenate([h2[t], ctx_in], 1)
        G[PARAMS[3]] += dpre.T @ s["ha_prev"]
        G[PARAMS[4]] += dpre.sum(0)
        G[PARAMS[5]] += dpre.sum(0)
        dxin = dpre @ a_ih
        dx[t], dctx_c, dha = dxin[:, :PN], dxin[:, PN:], dpre @ a_hh
    G[PARAMS[18]] += dha.sum(0)[None]
    G[PARAMS[20]] += dhd.sum(0)[None]
    dz2 = dx * (z2 > 0) * m2
    G[PARAMS[1]] += np.einsum("tbo,tbi->oi", dz2, h1)
    dz1 = (dz2 @ w2) * (z1 > 0) * m1
    G[PARAMS[0]] += np.einsum("tbo,tbi->oi", dz1, fr)
    dfr = dz1 @ w1
    if mutant != "zero_go":
        G[PARAMS[19]] += dfr[0].sum(0)[None]
    g_mem = np.zeros((B, T, MR))
    g_mem[:, :T - 1] = dfr[1:].transpose(1, 0, 2)
    G[PARAMS[7]] += np.einsum("bla,ble->ae", dP, x_in)
    g_in += dP @ wi
    res["grad_inputs"] = np.where(valid[:, :, None], g_in, 0.0)
    res["grad_memories"] = g_mem.reshape(B, T * r, mel)
    for n in PARAMS:
        res["grad_" + n] = G[n]
    res["S_de"] = S_de
    return res


@functools.lru_cache(maxsize=None)
def restated(case):
    """``restate(inputs(case))`` for a named case, computed once and shared; do not modify."""
    return restate(inputs(case))


# ------------------------------------------------------------------ the bound
def ratio(got, ref64, scale=None):
    """max |got - ref64| / max(1, max |ref64|) (``scale`` in place of max |ref64|): within the bound when <= tol."""
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    s = float(np.abs(ref64).max()) if scale is None else float(scale)
    return float(np.abs(got - ref64).max() / max(1.0, s))


def scale_of(case, name, restated_):
    """The magnitude a tensor is judged against when it is not its own: v's bias gradient under softmax."""
    if name == V_BIAS and case_of(case)["norm"] == "softmax":
        return restated_["S_de"]
    return None


def tolerance(reference_fp32, case, name):
    """4e-6, or 4x the reference's own float32 figure for this case and tensor (the fixture's / profile's) if larger."""
    own = 0.0 if reference_fp32 is None else float(reference_fp32.get(case, {}).get(name, 0.0))
    return max(TOL, MARGIN * own)


def check(got, ref64, what, tol=TOL, scale=None):
    """Prints the figure, then asserts the bound.  Returns the ratio."""
    v = ratio(got, ref64, scale)
    print(f"{what}: max|got - ref64| / max(1, scale) = {v:.3e} (bound {tol:.1e})")
    assert np.isfinite(np.asarray(got)).all(), f"{what}: non-finite values"
    assert v <= tol, f"{what}: {v:.3e} above {tol:.1e}"
    return v


# ------------------------------------------------------------------ the decoder, restated in torch
def torch_decoder(case_or_cfg, weights=None, dtype=None):
    """A ``TorchDecoder`` for a case (or a dict with dims, r, norm, fwd, sep, pdrop), optionally with weights."""
    import torch
    c = case_of(case_or_cfg)
    d = c["dims"]
    m = torch_decoder_class()(d["E"], d["mel"], c["r"], False, c["norm"], "original", c["pdrop"], c["fwd"], False, False, False,
                     c["sep"], prenet_dim=d["PN"], rnn_dim=d["R"], attention_dim=d["A"])
    if weights is not None:
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in weights.items()})
    return m if dtype is None else m.to(dtype)


def _torch_classes():
    import torch
    from torch import nn

    class Linear(nn.Module):
        def __init__(self, i, o, bias=True, init_gain="linear"):
            super().__init__()
            self.linear_layer = nn.Linear(i, o, bias=bias)
            nn.init.xavier_uniform_(self.linear_layer.weight, gain=nn.init.calculate_gain(init_gain))

        def forward(self, x):
            return self.linear_layer(x)

    class TorchDecoder(nn.Module):
        """The teacher-forced decoder in plain torch ops, one step at a time, with explicit dropout masks
        (``masks``: the four groups as uint8 tensors, 1 = keep; drawn from torch's generator when None and
        training).  Submodule names and shapes are the reference Decoder's, so state dicts load both ways."""

        def __init__(self, in_features, inputs_dim, r, attn_win, attn_norm, prenet_type, prenet_dropout, forward_attn,
                     trans_agent, forward_attn_mask, location_attn, separate_stopnet, prenet_dim=256, rnn_dim=1024,
                     attention_dim=128):
            super().__init__()
            assert prenet_type == "original" and not trans_agent and not location_attn
            self.mel_channels, self.r, self.encoder_embedding_dim = inputs_dim, r, in_features
            self.separate_stopnet, self.prenet_dim = separate_stopnet, prenet_dim
            self.attention_rnn_dim = self.decoder_rnn_dim = rnn_dim
            self.p_attention_dropout = self.p_decoder_dropout = 0.1
            MR = inputs_dim * r
            self.prenet = nn.Module()
            self.prenet.prenet_type, self.prenet.prenet_dropout = prenet_type, prenet_dropout
            self.prenet.layers = nn.ModuleList([Linear(MR, prenet_dim, bias=False),
                                                Linear(prenet_dim, prenet_dim, bias=False)])
            self.attention_rnn = nn.LSTMCell(prenet_dim + in_features, rnn_dim)
            att = nn.Module()
            att.query_layer = Linear(rnn_dim, attention_dim, bias=False, init_gain="tanh")
            att.inputs_layer = Linear(in_features, attention_dim, bias=False, init_gain="tanh")
            att.v = Linear(attention_dim, 1, bias=True)
            att.windowing, att.norm, att.forward_attn, att.trans_agent = attn_win, attn_norm, forward_attn, trans_agent
            att.forward_attn_mask, att.location_attention = forward_attn_mask, location_attn
            self.attention_layer = att
            self.decoder_rnn = nn.LSTMCell(rnn_dim + in_features, rnn_dim, 1)
            self.linear_projection = Linear(rnn_dim + in_features, MR)
            self.stopnet = nn.Sequential(nn.Dropout(0.1), Linear(rnn_dim + MR, 1, bias=True, init_gain="sigmoid"))
            self.attention_rnn_init = nn.Embedding(1, rnn_dim)
            self.go_frame_init = nn.Embedding(1, MR)
            self.decoder_rnn_inits = nn.Embedding(1, rnn_dim)
            self.last_masks = None

        def draw_masks(self, B, T, device):
            R, MR = self.attention_rnn_dim, self.mel_channels * self.r
            shapes = dict(prenet=(2, T, B, self.prenet_dim), att=(2, T, B, R), dec=(2, T, B, R), stop=(T, B, R + MR))
            return {k: (torch.rand(s, device=device) >= P_DROP[k]).to(torch.uint8) for k, s in shapes.items()}

        def forward(self, inputs, memories, mask, masks=None):
            B, L, _ = inputs.shape
            T, R = memories.shape[1] // self.r, self.attention_rnn_dim
            dt, dev = inputs.dtype, inputs.device
            train = self.training
            if train and masks is None:
                masks = self.draw_masks(B, T, dev)
            self.last_masks = masks if train else None
            keep = (lambda k, i=None: (masks[k] if i is None else masks[k][i]).to(dt) / (1.0 - P_DROP[k])) if train else None
            valid = torch.ones(B, L, dtype=torch.bool, device=dev) if mask is None else mask.to(torch.bool)
            x_in = torch.where(valid[:, :, None], inputs, torch.zeros((), dtype=dt, device=dev))
            zero = torch.zeros(B, dtype=torch.long, device=dev)
            frames = torch.cat([self.go_frame_init(zero)[None], memories.reshape(B, T, -1).transpose(0, 1)], 0)[:T]
            x = frames
            for i, lin in enumerate(self.prenet.layers):
                x = torch.relu(lin(x))
                if train and self.prenet.prenet_dropout:
                    x = x * keep("prenet", i)
            h_a, c_a = self.attention_rnn_init(zero), torch.zeros(B, R, dtype=dt, device=dev)
            h_d, c_d = self.decoder_rnn_inits(zero), torch.zeros(B, R, dtype=dt, device=dev)
            ctx = torch.zeros(B, self.encoder_embedding_dim, dtype=dt, device=dev)
            alpha = torch.cat([torch.ones(B, 1, dtype=dt, device=dev), torch.full((B, L - 1), 1e-7, dtype=dt, device=dev)], 1)
            Pm = self.attention_layer.inputs_layer(x_in)
            ninf = torch.full((), -float("inf"), dtype=dt, device=dev)
            outs, stops, aligns = [], [], []
            for t in range(T):
                h_a, c_a = self.attention_rnn(torch.cat([x[t], ctx], 1), (h_a, c_a))
                if train:
                    h_a, c_a = h_a * keep("att", 0)[t], c_a * keep("att", 1)[t]
                q = self.attention_layer.query_layer(h_a)
                e = self.attention_layer.v(torch.tanh(q[:, None, :] + Pm)).squeeze(-1)
                e = torch.where(valid, e, ninf)
                if self.attention_layer.norm == "softmax":
                    al = torch.softmax(e, -1)
                else:
                    sg = torch.sigmoid(e)
                    al = sg / sg.sum(1, keepdim=True)
                if self.attention_layer.forward_attn:
                    shifted = torch.nn.functional.pad(alpha[:, :-1], (1, 0))
                    u = ((0.5 * alpha + 0.5 * shifted) + 1e-8) * al
                    alpha = u / u.sum(1, keepdim=True)
                else:
                    alpha = al
                ctx = torch.bmm(alpha[:, None, :], x_in).squeeze(1)
                h_d, c_d = self.decoder_rnn(torch.cat([h_a, ctx], 1), (h_d, c_d))
                if train:
                    h_d, c_d = h_d * keep("dec", 0)[t], c_d * keep("dec", 1)[t]
                out = self.linear_projection(torch.cat([h_d, ctx], 1))
                xs = torch.cat([h_d, out], 1)
                if self.separate_stopnet:
                    xs = xs.detach()
                if train:
                    xs = xs * keep("stop")[t]
                stops.append(self.stopnet[1](xs).squeeze(1))
                outs.append(out)
                aligns.append(alpha)
            outputs = torch.stack(outs).transpose(0, 1).contiguous().view(B, -1, self.mel_channels).transpose(1, 2)
            return outputs, torch.stack(stops).transpose(0, 1).contiguous(), torch.stack(aligns).transpose(0, 1)

    return TorchDecoder


@functools.lru_cache(maxsize=None)
def torch_decoder_class():
    return _torch_classes()


def __getattr__(name):  # TorchDecoder is built on first use, so that importing this module needs no torch
    if name == "TorchDecoder":
        return torch_decoder_class()
    raise AttributeError(name)


# ------------------------------------------------------------------ a small reference-shaped model for train_batch
MODEL = dict(E=32, PN=16, R=48, A=16, mel=16)
MODEL_TEXT_LENGTHS, MODEL_MEL_LENGTHS, MODEL_R = [6, 5, 3], [10, 7, 4], 2


def model_batch(device="cpu"):
    """A batch as datasets.collate_fn returns it (train_util.batch with 16 mel channels): L = 6, T = 5 steps at r = 2."""
    import torch
    g = np.random.Generator(np.random.PCG64(541))
    B, T, D = 3, 10, MODEL["mel"]
    mel = g.uniform(0.0, 1.0, (B, T, D)).astype(np.float32)
    stop = np.zeros((B, T), np.float32)
    for b, n in enumerate(MODEL_MEL_LENGTHS):
        mel[b, n:] = 0.0
        stop[b, n - 1:] = 1.0
    text = g.integers(1, 100, (B, 6))
    for b, n in enumerate(MODEL_TEXT_LENGTHS):
        text[b, n:] = 0
    return (torch.from_numpy(text), torch.LongTensor(MODEL_TEXT_LENGTHS), [f"spk{b}" for b in range(B)],
            torch.from_numpy(mel.copy()).to(device), torch.from_numpy(mel).to(device), torch.LongTensor(MODEL_MEL_LENGTHS),
            torch.from_numpy(stop).to(device), [f"item{b}.wav" for b in range(B)])


def small_model(separate_stopnet):
    """Embedding -> three conv-BN blocks -> BiLSTM -> TorchDecoder -> a Postnet of three conv-BN blocks, wired as the
    reference's Tacotron2.forward wires them (models/tacotron2.py:44-60), at MODEL's small dimensions."""
    import torch
    from torch import nn
    d = MODEL

    class Block(nn.Module):
        def __init__(self, cin, cout, act):
            super().__init__()
            mods = [nn.Conv1d(cin, cout, 5, padding=2), nn.BatchNorm1d(cout)] + ([act()] if act else []) + [nn.Dropout(0.5)]
            self.net = nn.Sequential(*mods)

        def forward(self, x):
            return self.net(x)

    class Encoder(nn.Module):
        def __init__(self):
            super().__init__()
            self.convolutions = nn.Sequential(*[Block(d["E"], d["E"], nn.ReLU) for _ in range(3)])
            self.lstm = nn.LSTM(d["E"], d["E"] // 2, num_layers=1, batch_first=True, bidirectional=True)

        def forward(self, x, input_lengths):
            x = self.convolutions(x).transpose(1, 2)
            x = nn.utils.rnn.pack_padded_sequence(x, input_lengths.cpu().numpy(), batch_first=True)
            self.lstm.flatten_parameters()
            outputs, _ = self.lstm(x)
            return nn.utils.rnn.pad_packed_sequence(outputs, batch_first=True)[0]

    class Postnet(nn.Module):
        def __init__(self):
            super().__init__()
            self.convolutions = nn.ModuleList([Block(d["mel"], 32, nn.Tanh), Block(32, 32, nn.Tanh), Block(32, d["mel"], None)])

        def forward(self, x):
            for layer in self.convolutions:
                x = layer(x)
            return x

    class Model(nn.Module):
        def __init__(self):
            super().__init__()
            self.embedding = nn.Embedding(100, d["E"])
            self.encoder, self.postnet = Encoder(), Postnet()
            self.decoder = torch_decoder(dict(dims=d, r=MODEL_R, norm="sigmoid", fwd=True, sep=separate_stopnet, pdrop=True))

        def forward(self, text, text_lengths, mel, speaker_ids=None):
            mask = torch.arange(text.shape[1], device=text.device)[None, :] < text_lengths.to(text.device)[:, None]
            enc = self.encoder(self.embedding(text).transpose(1, 2), text_lengths)
            dec, stop, align = self.decoder(enc, mel, mask)
            post = dec + self.postnet(dec)
            return dec.transpose(1, 2), post.transpose(1, 2), align, stop

    torch.manual_seed(540)
    return Model()
