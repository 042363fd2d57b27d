#!/usr/bin/env python3
"""Greedy decode with bf16-stored weights against the fp32 decode, measured in one process (GPU box) at config 2 (--cfg5: also
config 5).  Every engine is a captured graph; the engines are timed in alternating rounds (median of the rounds), so clock and cache
drift fall on all alike.  Two fp32 engines are alternated as well: their ratio is the noise the bf16 / fp32 ratio is read against.
Also: per-launch times of both modes (run_timed(): eager, HIP events, steps >= 1), the weight bytes each mode streams per step
(from shapes), the cache plan each engine chose, the bf16 rate under the alternative cache plans, and how many captions of the bf16
decode equal the fp32 decode's on the UNROUNDED synthetic checkpoint (random weights with small margins, not a trained model).
Prints one JSON line.

  python tools/bench_decode_bf16.py [--steps 20] [--rounds 5] [--cfg5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "cyclical-visual-captioning_amd"))

LAUNCHES = ("att_lstm", "h2attn", "attn_scores", "attn_wsum", "lang_lstm", "logits", "word_select")
HBM_BYTES_PER_S = 8e12


def rate(eng, steps, units):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.run()
    torch.cuda.synchronize()
    return units * steps / (time.perf_counter() - t0)


def alternate(engines, steps, rounds, units):
    for e in engines:                       # warm-up
        for _ in range(3):
            e.run()
    res = [[] for _ in engines]
    for _ in range(rounds):
        for i, e in enumerate(engines):
            res[i].append(rate(e, steps, units))
    return [float(np.median(r)) for r in res]


def launch_bytes(d, bpw, qsplit=8):
    """algorithmic bytes of every launch of a step: weights at bpw bytes each, every fp32 operand and result once"""
    B, N, F, R, A, V = d.B, d.N, d.F, d.R, d.A, d.V
    f = 4 * B
    return {"att_lstm": bpw * 8 * R * R + f * (2 * R + 4 * R + 4 * R + 3 * R),          # x, gate_fc, table rows, c / c' / h'
            "h2attn": bpw * A * R + f * (R + qsplit * A),
            "attn_scores": 4 * B * (N + F) * A + f * (qsplit * A + N + F),
            "attn_wsum": 4 * B * (N + F) * R + f * (2 * (N + F) + R),
            "lang_lstm": bpw * 12 * R * R + f * (3 * R + 3 * R),
            "logits": bpw * V * R + f * R + ((V + 31) // 32) * 64 * 6 * 4,
            "word_select": ((V + 31) // 32) * 64 * 6 * 4}


def per_launch(eng, d, bpw):
    eng.run_timed()
    t = eng.run_timed()
    nbytes = launch_bytes(d, bpw)
    out = {}
    for name in LAUNCHES:
        us = float(np.median(t[name][1:])) * 1e3 if len(t[name]) > 1 else float(t[name][0]) * 1e3      # (step 0 multiplies a short K)
        out[name] = dict(us=round(us, 2), bytes=nbytes[name], frac_of_8TBps=round(nbytes[name] / (us * 1e-6) / HBM_BYTES_PER_S, 3))
    out["sum_us"] = round(sum(v["us"] for v in out.values()), 1)
    return out


def plan_of(eng):
    return {k: bool(v) for k, v in eng.cache_keep.items()}


def config(name, dev, steps, rounds, seed, alternatives):
    from cvc import synth
    from cvc.decode import DecodeEngine, DecodeWeights, weights as Wt
    d = synth.CONFIGS[name]
    W = DecodeWeights({k: torch.from_numpy(v).to(dev) for k, v in synth.hot_path_state_dict(d, seed).items()})
    feats = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in synth.clip_features(d, seed).items()}
    mk = lambda **kw: DecodeEngine(W, feats, d.T, synth.UNK_IDX, **kw).capture()
    e32, e32b, e16 = mk(), mk(), mk(weights_dtype="bf16")
    units = d.B * d.T
    r32, r32b, r16 = alternate([e32, e32b, e16], steps, rounds, units)
    R, A, V = d.R, d.A, d.V
    out = dict(fp32=round(r32, 1), fp32_again=round(r32b, 1), bf16=round(r16, 1), ratio_bf16_over_fp32=round(r16 / r32, 4),
               fp32_vs_fp32_spread=round(abs(r32b / r32 - 1.0), 4),
               weight_bytes_per_step=dict(fp32=4 * (20 * R * R + A * R + V * R), bf16=2 * (20 * R * R + A * R + V * R)),
               cache_plan=dict(fp32=plan_of(e32), bf16=plan_of(e16)),
               per_launch=dict(fp32=per_launch(e32, d, 4), bf16=per_launch(e16, d, 2)))
    # caption agreement on the unrounded checkpoint
    s32, s16 = e32.run()[0].clone(), e16.run()[0].clone()
    out["agreement_bf16_vs_fp32_unrounded_synthetic_checkpoint"] = dict(
        clips=round(float((s32 == s16).all(1).float().mean()), 4), words=round(float((s32 == s16).float().mean()), 4),
        note="random synthetic weights with small deciding margins, not a trained checkpoint")
    if alternatives:
        # the bf16 rate under other cache plans, each against the fp32 engine in the same alternation
        alt = {}
        saved = (Wt.CACHE_GATE_WEIGHTS, Wt.CACHE_LANG_GATE_WEIGHTS)
        try:
            for label, att, lang in (("att_w_only", True, False), ("features_instead", False, False)):
                Wt.CACHE_GATE_WEIGHTS, Wt.CACHE_LANG_GATE_WEIGHTS = att, lang
                e = mk(weights_dtype="bf16")
                ra, rb, rc = alternate([e32, e16, e], steps, rounds, units)
                alt[label] = dict(bf16=round(rc, 1), bf16_default_plan=round(rb, 1), fp32=round(ra, 1), cache_plan=plan_of(e))
                del e
        finally:
            Wt.CACHE_GATE_WEIGHTS, Wt.CACHE_LANG_GATE_WEIGHTS = saved
        out["bf16_cache_plan_alternatives"] = alt
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1236)
    ap.add_argument("--cfg5", action="store_true")
    ap.add_argument("--no_alternatives", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.rounds < 5:
        ap.error("--rounds: the rates are medians of at least 5 rounds")
    from cvc import hip
    dev = torch.device("cuda:0")
    out = {"metric": "greedy decode-steps/s, bf16-stored weights vs fp32, graph replay", "unit": "decode-steps/s", "lib": hip.version(),
           "steps": args.steps, "rounds": args.rounds}
    out["cfg2"] = config("cfg2", dev, args.steps, args.rounds, args.seed, not args.no_alternatives)
    if args.cfg5:
        out["cfg5"] = config("cfg5", dev, args.steps, args.rounds, args.seed, False)
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
