#!/usr/bin/env python3
"""Ensemble decoding next to the single engine, measured in one process (GPU box; default config 3, seeded random checkpoints):
  * the decode: the single DecodeEngine in its ordinary mode (greedy: fused tail through the C driver; beam 5: the C driver), the
    M = 1 ensemble (the cost of the members' `given` form plus the combine launch) and M = 2, 3, each for greedy and for beam 5, all
    captured graphs timed in alternating rounds (median with min and max), in clip steps per second (B x T per decode, as bench.py
    counts) and in ms per decode;
  * the combine launch on its own: cvc_ensemble_logprobs back to back between two events at 64 rows (finished logits, as the packed
    members leave them) and at 320 rows (6 K-slice slabs + bias per member, as the tile members leave them), M = 1, 2, 3, both forms.
Prints one JSON line.

  python tools/bench_ensemble.py [--steps 20] [--rounds 5] [--beam 5] [--config cfg3] [--members 3]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "cyclical-visual-captioning_amd"))


def ms_per_decode(eng, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.run()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def combine_probe(rounds, V=5000, n=300):
    from cvc import hip
    L, dev = hip.lib(), torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    cases = {}
    for rows, nparts, with_bias in ((64, 1, False), (320, 6, True)):
        out = torch.zeros(rows, V, device=dev)
        members = [((torch.randn(nparts, rows, V, generator=g) / nparts ** 0.5).to(dev), torch.randn(V, generator=g).to(dev) if with_bias else None)
                   for _ in range(3)]
        for M in (1, 2, 3):
            src = (hip.EnsembleSrc * M)(*(hip.EnsembleSrc(p.data_ptr(), nparts, rows * V, None if b is None else b.data_ptr())
                                          for p, b in members[:M]))
            logw = (C.c_float * M)(*hip.ensemble_log_weights(None, M))
            for geometric in (0, 1):
                cases[f"rows{rows}_M{M}_{'logprob' if geometric else 'prob'}"] = (
                    lambda src=src, M=M, logw=logw, geometric=geometric, rows=rows, out=out, keep=members:
                    L.cvc_ensemble_logprobs(src, M, logw, geometric, rows, V, out.data_ptr(), V, torch.cuda.current_stream().cuda_stream))

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="decodes per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--beam", type=int, default=5)
    ap.add_argument("--members", type=int, default=3)
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    from cvc import synth, hip
    from cvc.decode import DecodeEngine, DecodeWeights, EnsembleEngine
    dev = torch.device("cuda:0")
    d = synth.CONFIGS[args.config]
    members = []
    for m in range(args.members):
        W = DecodeWeights({k: torch.from_numpy(v).to(dev) for k, v in synth.hot_path_state_dict(d, args.seed + m).items()})
        f = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in synth.clip_features(d, args.seed + m).items()}
        f["pnt_mask"] = members[0][1]["pnt_mask"] if members else f["pnt_mask"]
        members.append((W, f))
    engines, launches = {}, {}
    for mode, kw in (("greedy", {}), (f"beam{args.beam}", dict(beam=args.beam))):
        engines[f"{mode}_single"] = DecodeEngine(members[0][0], members[0][1], d.T, synth.UNK_IDX, **kw)
        launches[f"{mode}_single"] = len(engines[f"{mode}_single"]._python_launches())
        for M in range(1, args.members + 1):
            e = engines[f"{mode}_M{M}"] = EnsembleEngine(members[:M], d.T, synth.UNK_IDX, **kw)
            launches[f"{mode}_M{M}"] = len(e._launches)
    for e in engines.values():
        e.capture()
        for _ in range(3):
            e.run()
    res = {name: [] for name in engines}
    for _ in range(args.rounds):
        for name, e in engines.items():
            res[name].append(ms_per_decode(e, args.steps))
    ms = {k: round(float(np.median(v)), 3) for k, v in res.items()}
    ms_mm = {k: [round(min(v), 3), round(max(v), 3)] for k, v in res.items()}
    rates = {k: round(d.B * d.T / (1e-3 * v), 1) for k, v in ms.items()}
    probe, probe_mm = combine_probe(args.rounds)
    ratio = {k: round(ms[k] / ms[k.split("_")[0] + "_single"], 3) for k in ms if not k.endswith("_single")}
    print(json.dumps({
        "metric": f"ms per decode and decode-steps/s (clip steps) at {args.config}: the single engine next to ensembles of 1 .. "
                  f"{args.members} seeded random checkpoints, greedy and beam {args.beam}, captured graphs, alternating rounds",
        "unit": "ms/decode", "lib": hip.version(), "B": d.B, "T": d.T, "V": d.V, "steps": args.steps, "rounds": args.rounds,
        "ms_per_decode": ms, "ms_per_decode_min_max": ms_mm, "decode_steps_per_s": rates, "ratio_vs_single": ratio,
        "launches_per_decode": launches, "combine_launch_us": probe, "combine_launch_us_min_max": probe_mm}))


if __name__ == "__main__":
    main()
