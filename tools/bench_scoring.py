#!/usr/bin/env python3
"""Teacher-forced decoding against the decodes it sits next to, measured in one process (GPU box) at config 2: the forced engine
with one caption per clip vs the greedy engine (packed path), and with 5 captions per clip vs the sampling engine with n = 5 (tile
path).  Every engine is a captured graph; the two engines of a pair are timed in alternating rounds (median of the rounds), so clock
and cache drift fall on both alike.  Rates are decode-steps/s in clip steps (B x T per decode, as bench.py counts them).  Next to the
rates: the word_select time per launch of both engines of a pair from DecodeEngine.run_timed() (HIP events around every launch of
an eager decode, median over the T steps of --timed_runs decodes), and the step's `logits` launch.  Prints one JSON line.

  python tools/bench_scoring.py [--steps 20] [--rounds 5] [--timed_runs 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "cyclical-visual-captioning_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_sampling import rate, launch_us          # noqa: E402  (the same timing loops)


def pair(W, feats, d, words, a_kw, n, steps, rounds, timed_runs):
    """engine a (a_kw) against the forced engine with n captions per clip -> dict of rates, ratio and per-launch times"""
    from cvc import synth
    from cvc.decode import DecodeEngine
    ea = DecodeEngine(W, feats, d.T, synth.UNK_IDX, **a_kw).capture()
    ef = DecodeEngine(W, feats, d.T, synth.UNK_IDX, forced_n=n).load_captions(words.repeat_interleave(n, 0).contiguous()).capture()
    for e in (ea, ef):
        for _ in range(3):
            e.run()
    res = [[], []]
    for _ in range(rounds):
        for i, e in enumerate((ea, ef)):
            res[i].append(rate(e, steps, d.B * d.T))
    ra, rf = (float(np.median(r)) for r in res)
    ua, uf = launch_us(ea, timed_runs), launch_us(ef, timed_runs)
    return dict(path="packed" if ef.packed else ("tile" if ef.tile else "ring"), rows=ef.rows, other=round(ra, 1), forced=round(rf, 1),
                ratio=round(rf / ra, 3), word_select_us_other=ua["word_select"], word_select_us_forced=uf["word_select"],
                logits_us_other=ua["logits"], logits_us_forced=uf["logits"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--timed_runs", type=int, default=5, help="eager decodes behind the per-launch times")
    args = ap.parse_args()
    from cvc import synth, hip
    from cvc.decode import DecodeWeights
    dev = torch.device("cuda:0")
    d = synth.CONFIGS["cfg2"]
    W = DecodeWeights({k: torch.from_numpy(v).to(dev) for k, v in synth.hot_path_state_dict(d, 1).items()})
    feats = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in synth.clip_features(d, 1).items()}
    words = torch.from_numpy(synth.captions(d, 1).astype(np.int64)).to(dev)
    out = {"metric": "decode-steps/s (clip steps), teacher-forced vs greedy / sampled decodes at config 2", "unit": "decode-steps/s",
           "lib": hip.version()}
    out["forced_n1_vs_greedy"] = pair(W, feats, d, words, dict(), 1, args.steps, args.rounds, args.timed_runs)
    out["forced_n5_vs_sample_n5"] = pair(W, feats, d, words, dict(temperature=1.0, sample_n=5, seed=1), 5, args.steps, args.rounds,
                                         args.timed_runs)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
