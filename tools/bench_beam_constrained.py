#!/usr/bin/env python3
"""Constrained beam search next to the beam decodes it extends, measured in one process at config 3 with beam 5 (GPU box): the
plain beam engine on the C driver, the plain beam engine on its Python launch list, the engine with beam_history alone (the
selection block that carries the hypotheses' histories, nothing banned but UNK), and the constrained engine with
no_repeat_ngram = 3, a minimum length of 8 and eight bad endings.  Every engine is a captured graph; the four are timed in
alternating rounds (median of the rounds), so clock and cache drift fall on all alike.  Rates are decode-steps/s in clip steps
(B x T per decode, as bench.py counts).  The per-launch time of word_select comes from DecodeEngine.run_timed() (HIP events around
every launch of an eager decode, median over the T steps of --timed_runs decodes): the plain cvc_beam_select_parts launch on the
same shape in the same process is the yardstick of the new block; the step's `logits` launch is printed next to it.  Prints one
JSON line.  --launch_probe instead times the two blocks alone: 300 back-to-back launches of each on random inputs of the engine's
shape (64 clips x beam 5, V = 5000, 6 slabs + bias) between two events, at t = 0 / 1 / 19 / 64 and with the rules, median of five
alternating rounds -- where the history block's time goes (throughput, not the latency run_timed() sees).

  python tools/bench_beam_constrained.py [--steps 20] [--rounds 5] [--timed_runs 5] [--beam 5] [--config cfg3] [--launch_probe]
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


def launch_probe(rounds, n=300):
    from cvc import hip
    L = hip.lib()
    dev = torch.device("cuda:0")
    B, beam, V, NP = 64, 5, 5000, 6
    rows = B * beam
    g = torch.Generator().manual_seed(1)
    parts = (torch.randn(NP, rows, V, generator=g) / NP ** 0.5).to(dev)
    bias, score = torch.randn(V, generator=g).to(dev), torch.randn(rows, generator=g).to(dev)
    done = torch.zeros(rows, dtype=torch.uint8, device=dev)
    parent = torch.zeros(rows, dtype=torch.int64, device=dev)
    word, score_out, done_out = torch.zeros_like(parent), torch.zeros(rows, device=dev), torch.zeros_like(done)
    ws, nb = torch.zeros(17 * rows, device=dev), torch.zeros(rows, dtype=torch.int32, device=dev)
    hin = torch.randint(0, V, (65, rows), generator=g).to(dev)
    hout = torch.zeros_like(hin)
    bad = torch.arange(10, 18, dtype=torch.int32, device=dev)
    rules = hip.Constraint(3, 0, 8, 0, bad.data_ptr(), bad.data_ptr(), 8)
    st = lambda: torch.cuda.current_stream().cuda_stream
    head = (parts.data_ptr(), NP, rows * V, bias.data_ptr(), score.data_ptr(), done.data_ptr(), B, beam, V, 1)
    tail = (parent.data_ptr(), word.data_ptr(), score_out.data_ptr(), done_out.data_ptr())
    plain = lambda: L.cvc_beam_select_parts(*head, 0, *tail, ws.data_ptr(), st())
    hist = lambda t, c: lambda: L.cvc_beam_select_hist_parts(*head, t, hin.data_ptr(), hout.data_ptr(), rows, c, *tail, nb.data_ptr(),
                                                             ws.data_ptr(), st())

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

    cases = {"plain": plain, "hist_t0": hist(0, None), "hist_t1": hist(1, None), "hist_t19": hist(19, None), "hist_t64": hist(64, None),
             "hist_t19_rules": hist(19, rules)}
    res = {k: [] for k in cases}
    for _ in range(rounds):
        for k, fn in cases.items():
            res[k].append(us(fn))
    print(json.dumps({"metric": "us per launch, back-to-back launches of the beam selection blocks (64 x 5 rows, V = 5000, 6 slabs + bias)",
                      "lib": hip.version(), "us": {k: round(float(np.median(v)), 2) for k, v in res.items()}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--timed_runs", type=int, default=5, help="eager decodes behind the per-launch times")
    ap.add_argument("--beam", type=int, default=5)
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--launch_probe", action="store_true", help="time the plain and the history block alone (see above)")
    args = ap.parse_args()
    if args.launch_probe:
        return launch_probe(args.rounds)
    from cvc import synth, hip
    from cvc.decode import DecodeEngine, DecodeWeights
    dev = torch.device("cuda:0")
    d = synth.CONFIGS[args.config]
    W = DecodeWeights({k: torch.from_numpy(v).to(dev) for k, v in synth.hot_path_state_dict(d, args.seed).items()})
    feats = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in synth.clip_features(d, args.seed).items()}
    mk = lambda **kw: DecodeEngine(W, feats, d.T, synth.UNK_IDX, beam=args.beam, **kw)
    hist = mk(beam_history=True)
    hist.run()
    # the lists: the words the free beam decode of this checkpoint puts most often (ids; a synthetic vocabulary has no articles)
    ids, counts = torch.unique(hist.hypotheses()[0], return_counts=True)
    common = [int(v) for v in ids[torch.argsort(counts, descending=True)][:9].tolist() if v != 0][:8]
    rules = dict(no_repeat_ngram=3, min_len=8, bad_endings=common)
    engines = {"beam_driver": mk(), "beam_python": mk(driver=False), "beam_history": hist, "constrained": mk(beam_history=True, **rules)}
    assert engines["beam_driver"]._plan is not None and all(engines[k]._plan is None for k in ("beam_python", "beam_history", "constrained"))
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
    us = {name: launch_us(engines[name], args.timed_runs) for name in ("beam_python", "beam_history", "constrained")}
    nb = engines["constrained"].nbanned.float()
    seq = engines["constrained"].hypotheses()[0].reshape(-1, d.T).tolist()
    cut = lambda h: h[:h.index(0)] if 0 in h else h
    rep3 = lambda h: len({tuple(h[i:i + 3]) for i in range(len(h) - 2)}) < max(len(h) - 2, 0)
    free = engines["beam_history"].hypotheses()[0].reshape(-1, d.T).tolist()
    e = engines["constrained"]
    out = {"metric": f"decode-steps/s (clip steps) at {args.config}, beam {args.beam}: constrained beam search next to the plain beam engines",
           "unit": "decode-steps/s", "lib": hip.version(), "rows": e.rows, "T": d.T, "V": d.V, "path": "tile" if e.tile else "ring",
           "rules": dict(no_repeat_ngram=3, min_len=8, bad_endings=len(common)), "rates": rates, "rates_min_max": spread,
           "ratio_history_vs_python": round(rates["beam_history"] / rates["beam_python"], 4),
           "ratio_constrained_vs_python": round(rates["constrained"] / rates["beam_python"], 4),
           "ratio_python_vs_driver": round(rates["beam_python"] / rates["beam_driver"], 4),
           "word_select_us": {name: v["word_select"] for name, v in us.items()}, "logits_us": {name: v["logits"] for name, v in us.items()},
           "nbanned_mean": round(float(nb.mean()), 2), "nbanned_max": int(nb.max()),
           "hypotheses_repeating_a_trigram": {"free": sum(rep3(cut(h)) for h in free), "constrained": sum(rep3(cut(h)) for h in seq),
                                              "of": len(seq)}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
