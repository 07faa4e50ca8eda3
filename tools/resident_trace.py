#!/usr/bin/env python3
"""Per-CU event trace of the resident batch-1 decoder at configs[1] (measurement only).

Re-runs the last sentence with timers (tts_decoder_resident_phases) and reads the event trace:
for each event, its spread across the 256 CUs relative to the step's first P1, and which CUs
are last to publish h_att / h_dec.

    python tools/resident_trace.py [--L 100]
"""
import argparse
import collections
import importlib
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
gu = importlib.import_module("your-voice-tts_amd.generic_utils")
weights = importlib.import_module("your-voice-tts_amd.weights")

# events 8-11: the synthesis form (partials published, partials gathered, A2, none) | the general form
# (query row published, none, none, context published)
# events 12, 13 (both forms): the loop-top work done on wave 0 / wave 3, ahead of the pre1 poll
EV_TOP = ("looptop_w0", "looptop_w3", "unused", "unused")
# event 14 (synthesis form): the next step's attention operand loads issued (wave 6, end of the step)
# event 11 (synthesis form): on a stop CU the previous step's continue flag published (wave 5, behind
# its prenet-2 row, after that step's stop row and rule); on every other CU the pre1 rows
# gathered, by wave 0 on the CUs of even rank and wave 1 on the odd
# event 15 (synthesis form): the previous step's continue flag gathered (wave 2, with the energy
# partials, ahead of A2)
# --rule-in-step11: a library from before the rule moved (flag published at the end of its own step,
# gathered behind the next step's prenet-2 row)
EV_SYN = ("P1", "B1", "hatt_pub", "B3", "B4", "hdec_pub", "B6", "pre1_pub", "part_pub", "part_gathered", "att_A2",
          "rows_gathered|flag_pub") + EV_TOP[:2] + ("operands_issued", "flag_gathered")
EV_GEN = EV_SYN[:8] + ("q_pub", "unused", "unused", "ctx_pub") + EV_TOP
STOP_CUS = 8  # workgroups 0-7 are rank 0 of their XCD (the stop CUs) under round-robin placement

ap = argparse.ArgumentParser()
ap.add_argument("--L", type=int, default=100)
ap.add_argument("--nomask", action="store_true", help="Synthesizer.tts()'s configuration (general form)")
ap.add_argument("--rule-in-step11", action="store_true", help="the flag's sites of the earlier synthesis form")
args = ap.parse_args()
EV = EV_GEN if args.nomask else EV_SYN
cfg = gu.default_config("config_tacotron2.json")
cfg.forward_attn_mask = not args.nomask
m = gu.setup_model(130, cfg, max_batch=1, max_len=256)
m.load_state_dict({k: torch.from_numpy(v) for k, v in weights.tacotron2_weights(0).items()})
m.cuda().eval()
ids = weights.synthetic_ids(args.L, 1)
for _ in range(3):
    out = m.inference_batch([ids])
torch.cuda.synchronize()
ph = m.profile_resident_phases()
tr = m.profile_resident_trace().astype(np.float64) / 100.0  # wall clock 100 MHz -> us
steps = range(8, 60)
rel = {k: [] for k in EV}
last = {"hatt_pub": collections.Counter(), "hdec_pub": collections.Counter(), "pre1_pub": collections.Counter()}
period, edge_p1 = [], []
# the loop top of step t: from this CU's pre1 publish of step t-1 (wave 0) to the stamps ahead of
# the pre1 poll; P1, B1 and B3 after the step's first P1; the stop CUs against the rest, and B3 of the
# CUs that write a mel row against those that do not (stop CUs left out of both)
# the continue flag against the pre1 rows (synthesis form), us: at the publishers, the flag's
# publish after the XCD's last row (wave 0's rows: the one stamped) and after the stop CU's own;
# at the consumers (the CUs that are no stop CU), the flag's gather after the rows' gather on the
# same CU, and both against P1.  XCD = workgroup % 8, rank = workgroup // 8 (round-robin placement)
flag = {k: [] for k in ("last_row_pub_to_flag_pub", "stop_cu_row_pub_to_flag_pub", "rows_w0_gathered_to_flag_gathered",
                        "rows_w1_gathered_to_flag_gathered", "rows_gathered_to_P1", "flag_gathered_to_P1")}
flag_later = []
xcd, rk = np.arange(256) % 8, np.arange(256) // 8
top = {k: [] for k in ("looptop_w0_rest", "looptop_w0_stop", "looptop_w3_rest", "looptop_w3_stop", "P1_rest", "P1_stop",
                        "B1_rest", "B1_stop", "B3_rest", "B3_stop", "B3_mel_row_cus", "B3_no_mel_row_cus")}
# the flag behind the prenet-2 row (synthesis form): at the stop CUs, its publish after their own P1
# and ahead of their B1; at every CU, its gather after the publish (how long it had been visible)
# and after the partials' gather of wave 0
late = {k: [] for k in ("stop_cu_P1_to_flag_pub", "stop_cu_flag_pub_to_B1", "flag_pub_to_flag_gathered",
                        "part_gathered_to_flag_gathered")}
NMEL = 80  # workgroups 0-79 own a mel row (written by wave 4 inside the h_att wait)
mmm = lambda v: (v.min(), np.median(v), v.max())
for t in steps:
    t0 = tr[:, t, 0].min()
    period.append(tr[:, t + 1, 0].min() - t0)
    edge_p1.append(np.median(tr[:, t + 1, 0]) - np.median(tr[:, t, 7]))
    for w, k in (("w0", 12), ("w3", 13)):
        d = tr[:, t, k] - tr[:, t - 1, 7]
        top[f"looptop_{w}_rest"].append(mmm(d[STOP_CUS:]))
        top[f"looptop_{w}_stop"].append(mmm(d[:STOP_CUS]))
    top["P1_rest"].append(mmm(tr[STOP_CUS:, t, 0] - t0))
    top["P1_stop"].append(mmm(tr[:STOP_CUS, t, 0] - t0))
    top["B1_rest"].append(mmm(tr[STOP_CUS:, t, 1] - t0))
    top["B1_stop"].append(mmm(tr[:STOP_CUS, t, 1] - t0))
    top["B3_rest"].append(mmm(tr[STOP_CUS:, t, 3] - t0))
    top["B3_stop"].append(mmm(tr[:STOP_CUS, t, 3] - t0))
    top["B3_mel_row_cus"].append(mmm(tr[STOP_CUS:NMEL, t, 3] - t0))
    top["B3_no_mel_row_cus"].append(mmm(tr[NMEL:, t, 3] - t0))
    if not args.nomask and not args.rule_in_step11:
        fp = tr[:STOP_CUS, t, 11]  # step t-1's flag, published inside step t
        late["stop_cu_P1_to_flag_pub"].append(mmm(fp - tr[:STOP_CUS, t, 0]))
        late["stop_cu_flag_pub_to_B1"].append(mmm(tr[:STOP_CUS, t, 1] - fp))
        late["flag_pub_to_flag_gathered"].append(mmm(tr[:, t, 15] - fp[xcd]))
        late["part_gathered_to_flag_gathered"].append(mmm(tr[:, t, 15] - tr[:, t, 9]))
        flag["rows_gathered_to_P1"].append(mmm((tr[:, t, 0] - tr[:, t, 11])[STOP_CUS:]))
    if not args.nomask and args.rule_in_step11:
        fp = tr[:STOP_CUS, t - 1, 11]  # step t-1's flag: step t's P1 (parent) or B1 waits for it
        flag["last_row_pub_to_flag_pub"].append(mmm(np.array([fp[x] - tr[xcd == x, t - 1, 7].max() for x in range(8)])))
        flag["stop_cu_row_pub_to_flag_pub"].append(mmm(fp - tr[:STOP_CUS, t - 1, 7]))
        d = tr[:, t, 15] - tr[:, t, 11]
        flag["rows_w0_gathered_to_flag_gathered"].append(mmm(d[(rk > 0) & (rk % 2 == 0)]))
        flag["rows_w1_gathered_to_flag_gathered"].append(mmm(d[rk % 2 == 1]))
        flag["rows_gathered_to_P1"].append(mmm((tr[:, t, 0] - tr[:, t, 11])[STOP_CUS:]))
        flag["flag_gathered_to_P1"].append(mmm((tr[:, t, 0] - tr[:, t, 15])[STOP_CUS:]))
        flag_later.append(float((d[STOP_CUS:] > 0).mean()))
    for k, name in enumerate(EV):
        if name == "rows_gathered|flag_pub":  # (two meanings: reported above)
            continue
        v = tr[:, t, k]
        v = v[v > 0]
        if v.size == 0:  # (an event this form does not record)
            continue
        r = v - t0
        rel[name].append((r.min(), np.median(r), r.max()))
        if name in last:
            last[name][int(np.argmax(tr[:, t, k]))] += 1
rec = {"us_per_step_trace": float(np.median(period)),
       "pre1_pub_to_P1_us(median CU to median CU)": round(float(np.median(edge_p1)), 2),
       "loop_top_us(min,median,max)": {k: [round(float(x), 2) for x in np.median(np.array(v), 0)] for k, v in top.items()},
       "events_rel_step_start_us(min,median,max)": {k: [round(float(x), 2) for x in np.median(np.array(v), 0)]
                                                    for k, v in rel.items() if v},
       "flag_vs_rows_us(min,median,max)": {k: [round(float(x), 2) for x in np.median(np.array(v), 0)]
                                           for k, v in flag.items() if v},
       "flag_behind_prenet2_row_us(min,median,max)": {k: [round(float(x), 2) for x in np.median(np.array(v), 0)]
                                                for k, v in late.items() if v},
       "flag_gathered_after_rows_share_of_cus": round(float(np.mean(flag_later)), 3) if flag_later else None,
       "last_cu": {k: v.most_common(6) for k, v in last.items()},
       "phases": ph}
print(json.dumps(rec, indent=1))
