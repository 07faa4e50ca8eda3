"""The cases of tests/tacotron_resident_util.py are not vacuous and its comparator can fail (no GPU: the
float64 / float32 numpy oracle alone).

Every reference a device test compares with keeps its stop decisions MARGIN = 1e-3 (250 x the tolerance) away
from 0.6, leaves at most 3 % of its steps out of the argmax comparison, moves its attention past the slice
boundary it is there for, and is reproduced by the float32 oracle far inside the device bound; every tail case
ends by the alignment-tail rule below its step cap.  The faults the device tests are there to catch are restated
in numpy over the kernel's own cuts (slices of 32 positions, mel rows from 256 on, the sentences of a group) and
check_sentence has to reject each on the case that targets it.
"""
import numpy as np
import pytest

import tacotron_resident_util as u
from oracle.tacotron_oracle import TacotronOracle, _sig

REFS = u.references()
REF_IDS = [f"L{s.L}_c{s.c:g}_r{r}m{m}_cap{cap}" for (s, r, m, cap) in REFS]


def _live(ref, L):
    return 4 * np.arange(1, ref["steps"] + 1) > L


# ------------------------------------------------------------------ the cases
@pytest.mark.parametrize("key", list(REFS), ids=REF_IDS)
def test_reference_is_decisive_and_float32_reproduces_it(key):
    sent, r, m, cap = key
    L = sent.L
    ref = u.reference(sent, r, m, cap)
    live = _live(ref, L)
    assert live.any()
    assert np.abs(ref["stop"][live] - 0.6).min() >= u.MARGIN
    assert np.abs(ref["align"][live, L - 1] - 0.6).min() >= u.MARGIN
    assert u.tie_steps(ref["align"]).mean() <= u.SKIP_CAP
    k, reach = REFS[key]
    if k:  # at least half of the attention mass past position 32 k at some step
        assert ref["align"][:, u.PPC * k:].sum(1).max() > 0.5, f"never crosses position {u.PPC * k}"
    if reach:
        assert ref["align"].argmax(1).max() >= u.PPC * reach, f"the argmax never reaches slice {reach}"
    # float32 numpy against float64 numpy: a device miss at 4e-6 is the kernel's, not the number format's
    fig = u.check_sentence(u.reference(sent, r, m, cap, f32=True), ref, L)
    assert fig["align_err"] <= 1e-6 and fig["stop_err"] <= 1e-6 and fig["mel_rel_rms"] <= 1e-6, fig


# (case, sentence) -> the step the float64 oracle stops at
TAIL_STEPS = {("tail", 0): 70, ("tail", 1): 74, ("tail", 3): 145, ("tail", 4): 143, ("tail129", 0): 259}


@pytest.mark.parametrize("name,i", list(TAIL_STEPS))
def test_tail_cases_stop_by_the_tail_rule(name, i):
    c = u.CASES[name]
    sent = c["sents"][i]
    assert sent.c == u.TAIL_FACTOR[sent.L] != 1.0
    ref = u.case_reference(name, i)
    n = ref["steps"]
    assert n == TAIL_STEPS[name, i] and n <= c["cap"], "the cap, not the rule, ended the sentence"
    assert ref["align"][-1, sent.L - 1] > 0.6 and not ref["stop"][-1] > 0.6
    assert not (ref["stop"][:-1] > 0.6)[_live(ref, sent.L)[:-1]].any()
    # the unmodified slot-mates run to the cap: every tail sentence finishes while they go on
    for j, s in enumerate(c["sents"]):
        if s.c == 1.0:
            assert u.case_reference(name, j)["steps"] == c["cap"] + 1


def test_case_table_covers_the_cuts():
    a = u.CASES["slice_edges"]
    assert [s.L for s in a["sents"]] == [1, 2, 31, 32, 33, 63, 64, 65, 96, 97] and len(a["sents"]) % 4 == 2
    assert all(u.case_reference("long", i)["steps"] == 501 for i in (0, 1))
    assert set(u.EDGE_LENS) <= set(u.GROUP_LENS) and len(u.GROUP_LENS) == 32
    assert sorted({i % 4 for i in u.CASES["groups"]["oracle"]}) == [0, 1, 2, 3]
    assert len({i // 4 for i in u.CASES["groups"]["oracle"]}) == 4 and 31 in u.CASES["groups"]["oracle"]
    for name, c in u.CASES.items():
        queue, B, Lmax = 80 * c["m"], len(c["sents"]), max(s.L for s in c["sents"])
        assert c["resident"] is (B <= 32 and Lmax <= 256 and queue <= 512), name
        assert set(c["crossing"]) | set(c["reach"]) <= set(c["oracle"]), name
    assert u.case_reference("mel_r4m4", 0)["align"][:, 32:].sum(1).max() > 0.99


# ------------------------------------------------------------------ seeded faults
class Faulty(TacotronOracle):
    """The oracle's forward-attention step and decoder loop for config_tacotron_gst.json's attention (sigmoid
    norm, forward attention, u = 0.5, nothing else), with one of the kernel's possible slips:
      "prev":  alpha[j-1] taken as 0 at j % 32 == 0 (the boundary hand-off lost)
      "tail":  the stop rule's alpha[L-1] read at local index 31 of the last occupied slice
      "norm":  the normaliser without the last occupied slice's partial sum
      "mel":   rows m >= 256 of a step's mel output zero (the m1 < nmel cut misplaced)."""
    fault = None

    def _attention(self, st, h_att, inputs, P):
        w = self.w
        L = inputs.shape[0]
        pq = w["decoder.attention_layer.query_layer.linear_layer.weight"] @ h_att
        e = np.tanh(pq[None, :] + P) @ w["decoder.attention_layer.v.linear_layer.weight"][0] + \
            w["decoder.attention_layer.v.linear_layer.bias"][0]
        s = _sig(e)
        align = s / s.sum()
        alpha, uu = st["alpha"], st["u"]
        prev = np.concatenate([[0.0], alpha[:-1]]).astype(self.dt)
        if self.fault == "prev":
            prev[::u.PPC] = 0.0
        a = ((1 - uu) * alpha + uu * prev + 1e-8) * align
        last = (L - 1) // u.PPC
        total = a[:u.PPC * last].sum() if self.fault == "norm" and last > 0 else a.sum()
        st["alpha"] = a / total
        st["att_w"] = st["alpha"]
        jt = u.PPC * last + u.PPC - 1
        st["tail"] = (st["alpha"][jt] if jt < L else 0.0) if self.fault == "tail" else st["alpha"][-1]
        return st["alpha"] @ inputs

    def decoder(self, memory_in):
        w, dt = self.w, self.dt
        inputs = memory_in.astype(dt)
        L = inputs.shape[0]
        P = inputs @ w["decoder.attention_layer.inputs_layer.linear_layer.weight"].T
        memory = w["decoder.memory_init.weight"][0].copy()
        h_att = w["decoder.attention_rnn_init.weight"][0].copy()
        h_dec = [w["decoder.decoder_rnn_inits.weight"][i].copy() for i in range(2)]
        ctx = np.zeros(inputs.shape[1], dt)
        alpha = np.concatenate([[1.0], np.zeros(L - 1) + 1e-7]).astype(np.float32).astype(dt)
        st = dict(alpha=alpha, u=0.5)
        outs, stops, aligns = [], [], []
        gru = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")
        t = 0
        while True:
            x = self._prenet("decoder.prenet", memory)
            h_att = self._gru_cell(np.concatenate([x, ctx]), h_att, *[w[f"decoder.attention_rnn.{n}"] for n in gru])
            ctx = self._attention(st, h_att, inputs, P)
            d = w["decoder.project_to_decoder_in.weight"] @ np.concatenate([h_att, ctx]) + \
                w["decoder.project_to_decoder_in.bias"]
            for i in range(2):
                h_dec[i] = self._gru_cell(d, h_dec[i], *[w[f"decoder.decoder_rnns.{i}.{n}"] for n in gru])
                d = h_dec[i] + d
            out = _sig(w["decoder.proj_to_mel.weight"] @ d + w["decoder.proj_to_mel.bias"])
            if self.fault == "mel":
                out[256:] = 0.0
            stop = _sig(w["decoder.stopnet.linear.weight"][0] @ np.concatenate([d, out]) +
                        w["decoder.stopnet.linear.bias"][0])
            outs.append(out)
            stops.append(stop)
            aligns.append(st["att_w"].copy())
            t += 1
            if (t > L / 4 and (stop > 0.6 or st["tail"] > 0.6)) or t > self.max_decoder_steps:
                break
            memory = np.concatenate([memory[self.r * 80:], out])
        return np.stack(outs).reshape(-1, 80), np.array(stops), np.stack(aligns)


def _faulty(fault, sent, r=5, m=5, cap=200, L_used=None):
    o = Faulty(u._weights(r, m), dtype=np.float64, **u.flags(r, m, cap))
    o.fault = fault
    rows = np.array(u.enc_rows(sent))
    if L_used is not None:  # the sentence's zero-padded rows decoded at another sentence's length
        rows = np.concatenate([rows, np.zeros((max(L_used - sent.L, 0), 256), np.float32)])[:L_used]
    got = u.as_result(*o.decoder(rows))
    if got["align"].shape[1] < sent.L:
        got["align"] = np.pad(got["align"], ((0, 0), (0, sent.L - got["align"].shape[1])))
    return got


def _rejected(got, ref, L):
    try:
        u.check_sentence(got, ref, L)
    except AssertionError:
        return True
    return False


def test_restated_decoder_is_the_oracle():
    """The restated loop without a fault is the oracle's own, bit for bit: a rejection below is the fault's."""
    for name, i in (("slice_edges", 4), ("tail", 1), ("mel_r1m5", 1)):
        c = u.CASES[name]
        got = _faulty(None, c["sents"][i], c["r"], c["m"], c["cap"])
        ref = u.case_reference(name, i)
        for k in ("mel", "stop", "align"):
            np.testing.assert_array_equal(got[k], ref[k])
        assert not _rejected(got, ref, c["sents"][i].L)


# fault -> the (case, sentence) that target it
FAULT_TARGETS = [("prev", "slice_edges", 4), ("prev", "slice_edges", 7), ("prev", "long", 1), ("prev", "mel_r4m4", 0),
                 ("tail", "tail", 1), ("tail", "tail", 4), ("tail", "tail129", 0),
                 ("norm", "slice_edges", 4), ("norm", "slice_edges", 9), ("norm", "small_handle", 1),
                 ("mel", "mel_r4m4", 0), ("mel", "mel_r4m5", 0), ("mel", "mel_r6m6", 0)]


@pytest.mark.parametrize("fault,name,i", FAULT_TARGETS)
def test_comparator_rejects_seeded_fault(fault, name, i):
    c = u.CASES[name]
    sent = c["sents"][i]
    assert _rejected(_faulty(fault, sent, c["r"], c["m"], c["cap"]), u.case_reference(name, i), sent.L)


def test_mel_fault_is_invisible_below_256_rows():
    """r = 1 has no row 256: the fault (d) is the r = 4 / r = 6 cases' to catch, and they do (above)."""
    c = u.CASES["mel_r1m5"]
    assert not _rejected(_faulty("mel", c["sents"][0], 1, 5, c["cap"]), u.case_reference("mel_r1m5", 0), 40)


@pytest.mark.parametrize("i,j", [(4, 5), (5, 4), (8, 9), (0, 1)])
def test_comparator_rejects_swapped_lengths(i, j):
    """(e) two sentences of a group swap encoder lengths: sentence i decoded at sentence j's length."""
    c = u.CASES["slice_edges"]
    si, sj = c["sents"][i], c["sents"][j]
    assert i // 4 == j // 4
    got = _faulty(None, si, L_used=sj.L)
    assert _rejected(got, u.case_reference("slice_edges", i), si.L)
