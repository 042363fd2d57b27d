#!/usr/bin/env python3
"""Diverse (group) beam search next to the beam decodes it extends, measured in one process (GPU box; default config 3, beam 6 in
3 groups, lambda 0.5): the plain beam engine on its Python launch list, the engine with beam_history alone
(cvc_beam_select_hist_parts) and the engine with beam_groups / diversity / length_penalty (cvc_beam_select_groups_parts, then
cvc_beam_rank and cvc_beam_backtrack_from).  Every engine is a captured graph; the three are timed in alternating rounds (median of
the rounds), so clock and cache drift fall on all alike.  Rates are decode-steps/s in clip steps (B x T per decode, as bench.py
counts).  The per-launch time of word_select comes from DecodeEngine.run_timed() (HIP events around every launch of an eager decode,
median over the T steps of --timed_runs decodes).  distinct = the share of distinct hypotheses per clip, mean over the clips;
distinct_first_words = the mean number of different first words among a clip's hypotheses.  Prints one JSON line.  --launch_probe
instead times the history block and the groups block alone: 300 back-to-back launches of each on random inputs of the engine's
shape (64 clips, V = 5000, 6 slabs + bias, t = 19) between two events, median of the alternating rounds.

  python tools/bench_beam_diverse.py [--steps 20] [--rounds 5] [--timed_runs 5] [--beam 6] [--groups 3] [--diversity 0.5]
                                     [--length_penalty 0.7] [--config cfg3] [--launch_probe]
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


def launch_probe(rounds, beam, groups, lam, n=300):
    from cvc import hip
    L = hip.lib()
    dev = torch.device("cuda:0")
    B, V, NP, t = 64, 5000, 6, 19
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
    st = lambda: torch.cuda.current_stream().cuda_stream
    head = (parts.data_ptr(), NP, rows * V, bias.data_ptr(), score.data_ptr(), done.data_ptr(), B, beam, V, 1, t, hin.data_ptr(),
            hout.data_ptr(), rows, None)
    tail = (parent.data_ptr(), word.data_ptr(), score_out.data_ptr(), done_out.data_ptr(), nb.data_ptr(), ws.data_ptr())
    cases = {"hist": lambda: L.cvc_beam_select_hist_parts(*head, *tail, st()),
             "groups_1": lambda: L.cvc_beam_select_groups_parts(*head, 1, 0.0, *tail, st()),
             f"groups_{groups}": lambda: L.cvc_beam_select_groups_parts(*head, groups, lam, *tail, st()),
             f"groups_{beam}": lambda: L.cvc_beam_select_groups_parts(*head, beam, lam, *tail, st())}

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
    print(json.dumps({"metric": f"us per launch, back-to-back launches of the history and the groups block (64 x {beam} rows, V = 5000, "
                                f"6 slabs + bias, t = {t})", "lib": hip.version(),
                      "us": {k: round(float(np.median(v)), 2) for k, v in res.items()},
                      "us_min_max": {k: [round(min(v), 2), round(max(v), 2)] for k, v in res.items()}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--timed_runs", type=int, default=5, help="eager decodes behind the per-launch times")
    ap.add_argument("--beam", type=int, default=6)
    ap.add_argument("--groups", type=int, default=3)
    ap.add_argument("--diversity", type=float, default=0.5)
    ap.add_argument("--length_penalty", type=float, default=0.7)
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--launch_probe", action="store_true", help="time the history and the groups block alone (see above)")
    args = ap.parse_args()
    if args.launch_probe:
        return launch_probe(args.rounds, args.beam, args.groups, args.diversity)
    from cvc import synth, hip
    from cvc.decode import DecodeEngine, DecodeWeights
    dev = torch.device("cuda:0")
    d = synth.CONFIGS[args.config]
    W = DecodeWeights({k: torch.from_numpy(v).to(dev) for k, v in synth.hot_path_state_dict(d, args.seed).items()})
    feats = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in synth.clip_features(d, args.seed).items()}
    mk = lambda **kw: DecodeEngine(W, feats, d.T, synth.UNK_IDX, beam=args.beam, **kw)
    engines = {"beam_python": mk(driver=False), "beam_history": mk(beam_history=True),
               "diverse": mk(beam_history=True, beam_groups=args.groups, diversity=args.diversity, length_penalty=args.length_penalty)}
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
    us = {name: launch_us(e, args.timed_runs) for name, e in engines.items()}

    def variety(e):
        seq = e.hypotheses()[0].cpu().tolist()
        return (round(float(np.mean([len({tuple(h) for h in clip}) / len(clip) for clip in seq])), 4),
                round(float(np.mean([len({h[0] for h in clip}) for clip in seq])), 2))
    var = {name: variety(engines[name]) for name in ("beam_history", "diverse")}
    e = engines["diverse"]
    out = {"metric": f"decode-steps/s (clip steps) at {args.config}, beam {args.beam}: diverse beam search ({args.groups} groups, lambda "
                     f"{args.diversity}, length penalty {args.length_penalty}) next to the plain and the history beam engines",
           "unit": "decode-steps/s", "lib": hip.version(), "rows": e.rows, "T": d.T, "V": d.V, "path": "tile" if e.tile else "ring",
           "rates": rates, "rates_min_max": spread, "ratio_diverse_vs_history": round(rates["diverse"] / rates["beam_history"], 4),
           "ratio_history_vs_python": round(rates["beam_history"] / rates["beam_python"], 4),
           "word_select_us": {name: v["word_select"] for name, v in us.items()}, "logits_us": {name: v["logits"] for name, v in us.items()},
           "distinct": {name: v[0] for name, v in var.items()}, "distinct_first_words": {name: v[1] for name, v in var.items()},
           "best_is_not_slot_0": int((e.order[:, 0] != 0).sum())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
