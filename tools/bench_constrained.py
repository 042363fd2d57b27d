#!/usr/bin/env python3
"""Constrained decoding next to the decodes it sits between, measured in one process at config 2 (GPU box): the greedy engine on
the C driver, the unconstrained sampling engine, and the constrained engine in both of its modes (arg-max and sampled) with
no_repeat_ngram = 3, a minimum length and a bad-endings list set.  Every engine is a captured graph; the four are timed in
alternating rounds (median of the rounds), so clock and cache drift fall on all alike.  Rates are decode-steps/s in clip steps
(B x T per decode, as bench.py counts).  The per-launch time of the selection block comes from DecodeEngine.run_timed() (HIP
events around every launch of an eager decode, median over the T steps of --timed_runs decodes), next to the plain sampling
block's and the step's `logits` launch on the same shape.  Prints one JSON line.

  python tools/bench_constrained.py [--steps 20] [--rounds 5] [--timed_runs 5]
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


def rate(eng, steps, units):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.run()
    torch.cuda.synchronize()
    return units * steps / (time.perf_counter() - t0)


def launch_us(eng, runs):
    """median microseconds per launch of word_select and logits over `runs` eager decodes (the first decode is not counted)"""
    eng.run_timed()
    acc = {"word_select": [], "logits": []}
    for _ in range(runs):
        t = eng.run_timed()
        for k in acc:
            acc[k] += t[k]
    return {k: round(1e3 * float(np.median(v)), 2) for k, v in acc.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--timed_runs", type=int, default=5, help="eager decodes behind the per-launch times")
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    from cvc import synth, hip
    from cvc.decode import DecodeEngine, DecodeWeights
    dev = torch.device("cuda:0")
    d = synth.CONFIGS["cfg2"]
    W = DecodeWeights({k: torch.from_numpy(v).to(dev) for k, v in synth.hot_path_state_dict(d, args.seed).items()})
    feats = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in synth.clip_features(d, args.seed).items()}
    greedy = DecodeEngine(W, feats, d.T, synth.UNK_IDX)
    seq = greedy.run()[0]
    # the lists: the words the greedy decode of this checkpoint puts most often (ids; a synthetic vocabulary has no articles)
    ids, counts = torch.unique(seq, return_counts=True)
    common = [int(v) for v in ids[torch.argsort(counts, descending=True)][:8].tolist() if v != 0]
    rules = dict(no_repeat_ngram=3, min_len=8, bad_endings=common)
    sample = dict(temperature=1.0, seed=1)
    kws = dict(greedy=dict(), sampling=sample, constrained_argmax=rules, constrained_sampled=dict(sample, **rules))
    engines = {name: DecodeEngine(W, feats, d.T, synth.UNK_IDX, **kw).capture() for name, kw in kws.items()}
    assert engines["greedy"]._plan is not None and engines["constrained_argmax"]._plan is None
    for e in engines.values():
        for _ in range(3):
            e.run()
    res = {name: [] for name in engines}
    for _ in range(args.rounds):
        for name, e in engines.items():
            res[name].append(rate(e, args.steps, d.B * d.T))
    rates = {name: round(float(np.median(r)), 1) for name, r in res.items()}
    us = {name: launch_us(engines[name], args.timed_runs) for name in ("sampling", "constrained_argmax", "constrained_sampled")}
    nb = {name: engines[name].nbanned.float() for name in ("constrained_argmax", "constrained_sampled")}
    e = engines["constrained_argmax"]
    out = {"metric": "decode-steps/s (clip steps) at config 2, constrained decoding next to greedy and sampling", "unit": "decode-steps/s",
           "lib": hip.version(), "rows": e.rows, "T": d.T, "V": d.V, "path": "packed" if e.packed else ("tile" if e.tile else "ring"),
           "rules": dict(no_repeat_ngram=3, min_len=8, bad_endings=len(common)), "rates": rates,
           "ratio_constrained_argmax_vs_greedy": round(rates["constrained_argmax"] / rates["greedy"], 3),
           "ratio_constrained_sampled_vs_sampling": round(rates["constrained_sampled"] / rates["sampling"], 3),
           "word_select_us": {name: v["word_select"] for name, v in us.items()}, "logits_us": {name: v["logits"] for name, v in us.items()},
           "nbanned_mean": {name: round(float(v.mean()), 2) for name, v in nb.items()},
           "nbanned_max": {name: int(v.max()) for name, v in nb.items()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
