#!/usr/bin/env python3
"""Sampled decoding against the arg-max decodes it sits next to, measured in one process (GPU box): greedy vs sampling with n = 1
at config 2, beam 5 vs sampling with n = 5 at config 3.  Every engine is a captured graph; the two engines of a pair are timed in
alternating rounds (median of the rounds), so clock and cache drift fall on both alike.  Rates are decode-steps/s in clip steps
(B x T per decode, as bench.py counts beam search): a sampled decode with n = 5 gives 5 captions per clip.  Prints one JSON line.

  python tools/bench_sampling.py [--steps 20] [--rounds 5]
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


def pair(d, dev, a_kw, b_kw, steps, rounds, seed=1):
    from cvc import synth
    from cvc.decode import DecodeEngine, DecodeWeights
    W = DecodeWeights({k: torch.from_numpy(v).to(dev) for k, v in synth.hot_path_state_dict(d, seed).items()})
    feats = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in synth.clip_features(d, seed).items()}
    engines = [DecodeEngine(W, feats, d.T, synth.UNK_IDX, **kw).capture() for kw in (a_kw, b_kw)]
    for e in engines:                       # warm-up
        for _ in range(3):
            e.run()
    res = [[], []]
    for _ in range(rounds):
        for i, e in enumerate(engines):
            res[i].append(rate(e, steps, d.B * d.T))
    return [float(np.median(r)) for r in res], engines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    from cvc import synth, hip
    dev = torch.device("cuda:0")
    out = {"metric": "decode-steps/s (clip steps), sampling vs arg-max decodes", "unit": "decode-steps/s", "lib": hip.version()}
    d2, d3 = synth.CONFIGS["cfg2"], synth.CONFIGS["cfg3"]
    (g, s1), (eg, es) = pair(d2, dev, dict(), dict(temperature=1.0, seed=1), args.steps, args.rounds)
    out["cfg2"] = dict(greedy=round(g, 1), sample_n1=round(s1, 1), ratio=round(s1 / g, 3), target=0.9,
                       sample_path="packed" if es.packed else ("tile" if es.tile else "ring"))
    del eg, es
    (b5, s5), (eb, es) = pair(d3, dev, dict(beam=5), dict(temperature=1.0, sample_n=5, seed=1), args.steps, args.rounds)
    out["cfg3"] = dict(beam5=round(b5, 1), sample_n5=round(s5, 1), ratio=round(s5 / b5, 3), target=1.0,
                       sample_path="packed" if es.packed else ("tile" if es.tile else "ring"))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
