#!/usr/bin/env python3
"""Sampled decoding against the arg-max decodes it sits next to, measured in one process (GPU box): greedy vs sampling with n = 1
at config 2, beam 5 vs sampling with n = 5 at config 3.  Every engine is a captured graph; the two engines of a pair are timed in
alternating rounds (median of the rounds), so clock and cache drift fall on both alike.  Rates are decode-steps/s in clip steps
(B x T per decode, as bench.py counts beam search): a sampled decode with n = 5 gives 5 captions per clip.  Prints one JSON line.

  python tools/bench_sampling.py [--steps 20] [--rounds 5]

With --top_k / --top_p (one value each per setting, several settings allowed: --top_k 0 40 40 --top_p 0.9 1.0 0.9) the tool also
measures top-k / nucleus truncation at config 2, on the packed path (n = 1) and on the tile path (n = 5): decode-steps/s of the
temperature-only engine against the truncating one (captured graphs, alternating rounds), and the word_select time per launch of
both from DecodeEngine.run_timed() (HIP events around every launch of an eager decode, median over the T steps of --timed_runs
decodes), next to the step's `logits` launch.  --trunc_only skips the greedy / beam pairs.
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


_bound = {}


def pair(d, dev, a_kw, b_kw, steps, rounds, seed=1):
    from cvc import synth
    from cvc.decode import DecodeEngine, DecodeWeights
    key = (repr(d), seed)
    if key not in _bound:                 # one binding of the checkpoint per shape, shared by the pairs of a run
        _bound.clear()
        _bound[key] = (DecodeWeights({k: torch.from_numpy(v).to(dev) for k, v in synth.hot_path_state_dict(d, seed).items()}),
                       {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in synth.clip_features(d, seed).items()})
    W, feats = _bound[key]
    engines = [DecodeEngine(W, feats, d.T, synth.UNK_IDX, **kw).capture() for kw in (a_kw, b_kw)]
    for e in engines:                       # warm-up
        for _ in range(3):
            e.run()
    res = [[], []]
    for _ in range(rounds):
        for i, e in enumerate(engines):
            res[i].append(rate(e, steps, d.B * d.T))
    return [float(np.median(r)) for r in res], engines


def launch_us(eng, runs):
    """median microseconds per launch of word_select and logits over `runs` eager decodes (the first decode is not counted)"""
    eng.run_timed()
    acc = {"word_select": [], "logits": []}
    for _ in range(runs):
        t = eng.run_timed()
        for k in acc:
            acc[k] += t[k]
    return {k: round(1e3 * float(np.median(v)), 2) for k, v in acc.items()}


def truncation(d, dev, n, settings, steps, rounds, timed_runs, seed=1):
    """temperature-only against truncating engines of one shape: rates (graph replay) and per-launch times (eager)"""
    from cvc import synth
    from cvc.decode import DecodeEngine, DecodeWeights
    base = dict(temperature=1.0, sample_n=n, seed=1)
    out = []
    for k, p in settings:
        (r0, r1), (e0, e1) = pair(d, dev, base, dict(base, top_k=k, top_p=p), steps, rounds, seed)
        u0, u1 = launch_us(e0, timed_runs), launch_us(e1, timed_runs)
        out.append(dict(top_k=k, top_p=p, path="packed" if e1.packed else ("tile" if e1.tile else "ring"), rows=e1.rows,
                        plain=round(r0, 1), trunc=round(r1, 1), ratio=round(r1 / r0, 3), word_select_us_plain=u0["word_select"],
                        word_select_us_trunc=u1["word_select"], logits_us=u1["logits"],
                        kept_median=float(e1.kept.float().median())))
        del e0, e1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--top_k", type=int, nargs="+", default=None, help="truncation settings to measure (paired with --top_p)")
    ap.add_argument("--top_p", type=float, nargs="+", default=None)
    ap.add_argument("--timed_runs", type=int, default=5, help="eager decodes behind the per-launch times")
    ap.add_argument("--trunc_only", action="store_true", help="skip the greedy / beam pairs")
    args = ap.parse_args()
    settings = []
    if args.top_k is not None or args.top_p is not None:
        ks, ps = args.top_k or [0], args.top_p or [1.0]
        if len(ks) != len(ps) and 1 not in (len(ks), len(ps)):
            ap.error("--top_k and --top_p take one value each per setting")
        m = max(len(ks), len(ps))
        settings = list(zip(ks * (m // len(ks)), ps * (m // len(ps))))
    from cvc import synth, hip
    dev = torch.device("cuda:0")
    out = {"metric": "decode-steps/s (clip steps), sampling vs arg-max decodes", "unit": "decode-steps/s", "lib": hip.version()}
    d2, d3 = synth.CONFIGS["cfg2"], synth.CONFIGS["cfg3"]
    if settings:
        out["truncation_cfg2"] = (truncation(d2, dev, 1, settings, args.steps, args.rounds, args.timed_runs) +
                                  truncation(d2, dev, 5, settings, args.steps, args.rounds, args.timed_runs))
    if args.trunc_only:
        print(json.dumps(out))
        return
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
