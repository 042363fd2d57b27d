#!/usr/bin/env python3
"""Lexically constrained beam search (forced words per clip) next to the history beam engine it extends, measured in one process
(GPU box; default config 3, beam 6, C = 2 forced words per clip, tile path): the engine with beam_history alone
(cvc_beam_select_hist_parts) and the engine with force_n = C (cvc_beam_select_force_parts, then cvc_beam_rank_force and
cvc_beam_backtrack_from).  Both are captured graphs, timed in alternating rounds (median of the rounds with min and max), so clock
and cache drift fall on both alike.  Rates are decode-steps/s in clip steps (B x T per decode, as bench.py counts).  The per-launch
time of word_select comes from DecodeEngine.run_timed() (HIP events around every launch of an eager decode, median over the T steps
of --timed_runs decodes).  The forced words are C distinct words per clip drawn from the vocabulary without UNK and word 0;
met_all = the share of clips whose returned caption holds all of them.  Prints one JSON line.  --launch_probe instead times the
history block and the forced block alone: 300 back-to-back launches of each on random inputs of the engine's shape (64 clips,
V = 5000, 6 slabs + bias, t = 19) between two events, median of the alternating rounds.

  python tools/bench_beam_forced.py [--steps 20] [--rounds 5] [--timed_runs 5] [--beam 6] [--force_n 2] [--length_penalty 0.0]
                                    [--config cfg3] [--launch_probe]
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

from bench_beam_diverse import rate, launch_us           # noqa: E402  (the same clocks as the diverse-beam tool)


def draw_force_words(B, C, V, unk, seed):
    rng = np.random.default_rng(seed)
    pool = np.array([w for w in range(1, V) if w != unk])
    return np.stack([rng.choice(pool, size=C, replace=False) for _ in range(B)]).astype(np.int32)


def launch_probe(rounds, beam, C, n=300):
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
    ws, nb, nm = torch.zeros(21 * rows, device=dev), torch.zeros(rows, dtype=torch.int32, device=dev), torch.zeros(rows, dtype=torch.int32, device=dev)
    hin = torch.randint(0, V, (65, rows), generator=g).to(dev)
    hout = torch.zeros_like(hin)
    force = torch.from_numpy(draw_force_words(B, C, V, 1, 1)).to(dev)
    st = lambda: torch.cuda.current_stream().cuda_stream
    head = (parts.data_ptr(), NP, rows * V, bias.data_ptr(), score.data_ptr(), done.data_ptr(), B, beam, V, 1, t, hin.data_ptr(),
            hout.data_ptr(), rows, None)
    tail = (parent.data_ptr(), word.data_ptr(), score_out.data_ptr(), done_out.data_ptr(), nb.data_ptr())
    cases = {"hist": lambda: L.cvc_beam_select_hist_parts(*head, *tail, ws.data_ptr(), st()),
             f"force_{C}": lambda: L.cvc_beam_select_force_parts(*head, force.data_ptr(), C, *tail, nm.data_ptr(), ws.data_ptr(), st())}

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
    print(json.dumps({"metric": f"us per launch, back-to-back launches of the history and the forced block (64 x {beam} rows, V = 5000, "
                                f"6 slabs + bias, t = {t})", "lib": hip.version(),
                      "us": {k: round(float(np.median(v)), 2) for k, v in res.items()},
                      "us_min_max": {k: [round(min(v), 2), round(max(v), 2)] for k, v in res.items()}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--timed_runs", type=int, default=5, help="eager decodes behind the per-launch times")
    ap.add_argument("--beam", type=int, default=6)
    ap.add_argument("--force_n", type=int, default=2)
    ap.add_argument("--length_penalty", type=float, default=0.0)
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--launch_probe", action="store_true", help="time the history and the forced block alone (see above)")
    args = ap.parse_args()
    if args.launch_probe:
        return launch_probe(args.rounds, args.beam, args.force_n)
    from cvc import synth, hip
    from cvc.decode import DecodeEngine, DecodeWeights
    dev = torch.device("cuda:0")
    d = synth.CONFIGS[args.config]
    W = DecodeWeights({k: torch.from_numpy(v).to(dev) for k, v in synth.hot_path_state_dict(d, args.seed).items()})
    feats = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in synth.clip_features(d, args.seed).items()}
    mk = lambda **kw: DecodeEngine(W, feats, d.T, synth.UNK_IDX, beam=args.beam, beam_history=True, **kw)
    engines = {"beam_history": mk(), "forced": mk(force_n=args.force_n, length_penalty=args.length_penalty)}
    assert all(e._plan is None for e in engines.values())
    force = draw_force_words(d.B, args.force_n, d.V, synth.UNK_IDX, args.seed)
    engines["forced"].load_force_words(force)
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
    e = engines["forced"]
    seq = e.run()[0].cpu().tolist()
    met_all = float(np.mean([set(int(w) for w in force[b]) <= set(seq[b]) for b in range(d.B)]))
    out = {"metric": f"decode-steps/s (clip steps) at {args.config}, beam {args.beam}: {args.force_n} forced words per clip (length "
                     f"penalty {args.length_penalty}) next to the history beam engine",
           "unit": "decode-steps/s", "lib": hip.version(), "rows": e.rows, "T": d.T, "V": d.V, "path": "tile" if e.tile else "ring",
           "rates": rates, "rates_min_max": spread, "ratio_forced_vs_history": round(rates["forced"] / rates["beam_history"], 4),
           "word_select_us": {name: v["word_select"] for name, v in us.items()}, "logits_us": {name: v["logits"] for name, v in us.items()},
           "met_all": round(met_all, 4), "top_bank_reached": round(float((e.final_nmet.max(1).values == args.force_n).float().mean()), 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
