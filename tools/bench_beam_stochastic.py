#!/usr/bin/env python3
"""Stochastic beam search next to what it sits between, measured in one process (GPU box; default config 3, beam 5, tile path):
  * the step: cvc_beam_select_stoch_parts next to cvc_beam_select_hist_parts, back-to-back launches of each on random inputs of the
    engine's shape (64 clips x beam rows, V = 5000, 6 slabs + bias, t = 19) between two events, and the per-launch time of
    word_select inside an eager decode (DecodeEngine.run_timed(), HIP events around every launch);
  * the decode: the stochastic engine next to the plain history beam of the same width and next to the sampling engine at
    sample_n = beam, all captured graphs timed in alternating rounds (median with min and max), in clip steps per second
    (B x T per decode, as bench.py counts);
  * what the feature is for: the share of clips whose `beam` independent samples are NOT all distinct (and the mean number of distinct
    captions among them), next to the stochastic beam's, which is 0 by construction, over --draws decodes of the batch.
Prints one JSON line.

  python tools/bench_beam_stochastic.py [--steps 20] [--rounds 5] [--timed_runs 5] [--beam 5] [--tau 1.0] [--draws 8] [--config cfg3]
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

from bench_beam_diverse import rate, launch_us           # noqa: E402  (the same clocks as the other beam tools)


def launch_probe(rounds, beam, tau, n=300):
    from cvc import hip
    L = hip.lib()
    dev = torch.device("cuda:0")
    B, V, NP, t = 64, 5000, 6, 19
    rows = B * beam
    g = torch.Generator().manual_seed(1)
    parts = (torch.randn(NP, rows, V, generator=g) / NP ** 0.5).to(dev)
    bias, score = torch.randn(V, generator=g).to(dev), torch.randn(rows, generator=g).to(dev)
    logq = -torch.rand(rows, generator=g) * 20
    G = (logq - torch.log(-torch.log(torch.rand(rows, generator=g).clamp(1e-6, 1 - 1e-6)))).to(dev)
    logq = logq.to(dev)
    done = torch.zeros(rows, dtype=torch.uint8, device=dev)
    parent = torch.zeros(rows, dtype=torch.int64, device=dev)
    word, score_out, done_out = torch.zeros_like(parent), torch.zeros(rows, device=dev), torch.zeros_like(done)
    logq_out, G_out = torch.zeros(rows, device=dev), torch.zeros(rows, device=dev)
    ws, nb = torch.zeros(26 * rows, device=dev), torch.zeros(rows, dtype=torch.int32, device=dev)
    state = torch.tensor([1, 0, 1, 0], dtype=torch.int32, device=dev)
    hin = torch.randint(0, V, (65, rows), generator=g).to(dev)
    hout = torch.zeros_like(hin)
    st = lambda: torch.cuda.current_stream().cuda_stream
    head = (parts.data_ptr(), NP, rows * V, bias.data_ptr(), score.data_ptr(), done.data_ptr(), B, beam, V, 1, t, hin.data_ptr(),
            hout.data_ptr(), rows, None)
    tail = (parent.data_ptr(), word.data_ptr(), score_out.data_ptr(), done_out.data_ptr())
    cases = {"hist": lambda: L.cvc_beam_select_hist_parts(*head, *tail, nb.data_ptr(), ws.data_ptr(), st()),
             "stoch": lambda: L.cvc_beam_select_stoch_parts(*head, 1.0 / tau, state.data_ptr(), logq.data_ptr(), G.data_ptr(), *tail,
                                                            logq_out.data_ptr(), G_out.data_ptr(), nb.data_ptr(), ws.data_ptr(), st())}

    def us(fn):
        for _ in range(20):
            assert fn() == 0
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / n

    res = {k: [] for k in cases}
    for _ in range(rounds):
        for k, fn in cases.items():
            res[k].append(us(fn))
    return ({k: round(float(np.median(v)), 2) for k, v in res.items()}, {k: [round(min(v), 2), round(max(v), 2)] for k, v in res.items()})


def distinct_counts(rows_per_clip):
    """[B, n, T] captions (words after the first 0 do not count) -> distinct captions per clip"""
    out = []
    for clip in rows_per_clip.tolist():
        cut = lambda h: tuple(h[:h.index(0) + 1]) if 0 in h else tuple(h)
        out.append(len({cut(h) for h in clip}))
    return np.array(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--timed_runs", type=int, default=5, help="eager decodes behind the per-launch times")
    ap.add_argument("--beam", type=int, default=5)
    ap.add_argument("--tau", type=float, default=1.0)
    ap.add_argument("--draws", type=int, default=8, help="decodes of the batch behind the distinctness figures")
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    from cvc import synth, hip
    from cvc.decode import DecodeEngine, DecodeWeights
    dev = torch.device("cuda:0")
    d = synth.CONFIGS[args.config]
    n = args.beam
    W = DecodeWeights({k: torch.from_numpy(v).to(dev) for k, v in synth.hot_path_state_dict(d, args.seed).items()})
    feats = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in synth.clip_features(d, args.seed).items()}
    engines = {"beam_history": DecodeEngine(W, feats, d.T, synth.UNK_IDX, beam=n, beam_history=True),
               "stochastic": DecodeEngine(W, feats, d.T, synth.UNK_IDX, beam=n, beam_history=True, stochastic=True,
                                          stochastic_tau=args.tau, seed=args.seed),
               "samples": DecodeEngine(W, feats, d.T, synth.UNK_IDX, sample_n=n, temperature=args.tau, seed=args.seed)}
    assert all(e._plan is None for e in engines.values())
    for e in engines.values():
        e.capture()
        for _ in range(3):
            e.run()
    res = {name: [] for name in engines}
    for _ in range(args.rounds):
        for name, e in engines.items():
            res[name].append(rate(e, args.steps, d.B * d.T))
    rates = {name: round(float(np.median(r)), 1) for name, r in res.items()}
    spread = {name: [round(min(r), 1), round(max(r), 1)] for name, r in res.items()}
    # distinct captions among a clip's n candidates
    ds, dd = [], []
    for _ in range(args.draws):
        seq = engines["samples"].run()[0].cpu().view(d.B, n, d.T)
        ds.append(distinct_counts(seq))
        engines["stochastic"].run()
        hyp, score, G, logq = engines["stochastic"].hypotheses()
        assert bool(torch.isfinite(G).all())
        dd.append(distinct_counts(hyp.cpu()))
    ds, dd = np.concatenate(ds), np.concatenate(dd)
    us = {name: launch_us(e, args.timed_runs) for name, e in engines.items()}
    probe, probe_mm = launch_probe(args.rounds, n, args.tau)
    out = {"metric": f"decode-steps/s (clip steps) at {args.config}, {n} candidates per clip, tau {args.tau}: stochastic beam search next "
                     f"to the history beam and to {n} independent samples",
           "unit": "decode-steps/s", "lib": hip.version(), "rows": engines["stochastic"].rows, "T": d.T, "V": d.V,
           "path": "tile" if engines["stochastic"].tile else "ring", "rates": rates, "rates_min_max": spread,
           "ratio_stochastic_vs_history": round(rates["stochastic"] / rates["beam_history"], 4),
           "ratio_stochastic_vs_samples": round(rates["stochastic"] / rates["samples"], 4),
           "word_select_us": {name: v["word_select"] for name, v in us.items()},
           "step_probe_us": probe, "step_probe_us_min_max": probe_mm, "ratio_step_stoch_vs_hist": round(probe["stoch"] / probe["hist"], 4),
           "clips": int(len(ds)),
           "samples_not_all_distinct": round(float((ds < n).mean()), 4), "samples_mean_distinct": round(float(ds.mean()), 3),
           "stochastic_not_all_distinct": round(float((dd < n).mean()), 4), "stochastic_mean_distinct": round(float(dd.mean()), 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
