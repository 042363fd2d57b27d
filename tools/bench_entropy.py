#!/usr/bin/env python3
"""What the entropy regulariser costs: config 3's captured cross-entropy step (cyclical pass, backward, clip, Adam; train-mode dropout;
one rank, no gradient exchange) with confidence_penalty off, = 0.05 and a SECOND trainer with it off, the three alternated in one
process -- the median of the rounds per trainer -- and the eager self-critical step (--scst_samples rollouts per clip) with
scst_entropy off, = 0.05 and off again under the same scheme.  A step with the term is judged against the first trainer without it;
the margin is the spread between the two trainers without it, which run identical launches.  The fused head launch
(cvc_vocab_head_nll_ls_fwd against cvc_vocab_head_nll_ent_fwd at config 3's head size, with the row sums behind it) is timed alone
by HIP events, median of --head_calls.
Writes profiles/entropy.md and profiles/bench_entropy_cfg3.json and prints the JSON line.

  python tools/bench_entropy.py [--steps 30] [--rounds 5] [--warmup 5] [--config cfg3] [--scst_samples 5] [--out profiles]
"""
import argparse
import dataclasses
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "cyclical-visual-captioning_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_label_smoothing import make_batch          # noqa: E402  (the same batch as the label-smoothing measurement)

BETA = 0.05


def build_trainer(d, dev, seed, capturable, **extra):
    """bench_train.run_train's model and options at the dims d, one rank; extra: confidence_penalty / scst_entropy / scst_* options"""
    from cvc import synth, opts as cvc_opts
    from cvc.model.captioner import DecodeAndGroundCaptionerGVDROI, PrecomputedRegionFeatures
    from cvc.trainer import Trainer, build_optimizer
    o = cvc_opts.parse_opt([])
    o.vocab_size, o.itow, o.wtoi = d.V, {str(i): "w%d" % i for i in range(d.V)}, {"UNK": synth.UNK_IDX}
    o.seq_length, o.rnn_size, o.input_encoding_size, o.att_hid_size = d.T, d.R, d.E, d.A
    o.detect_size, o.vis_encoding_size, o.train_decoder_only = d.DET, d.G, False
    o.xe_loss_weight, o.caption_consistency_loss_weight, o.learning_rate, o.batch_size = 0.5, 0.5, 1e-4, d.B
    for k, v in extra.items():
        setattr(o, k, v)
    model = DecodeAndGroundCaptionerGVDROI(o, roi_extractor=PrecomputedRegionFeatures(d.DET, d.G))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.hot_path_state_dict(d, seed).items()}, strict=False)
    model = model.to(dev).train()
    return Trainer(o, None, model, build_optimizer(model, o, capturable=capturable), None, None)


def timed_ms(step, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def alternate(kinds, steppers, rounds, steps):
    out = {name: [] for name in kinds}
    for _ in range(rounds):
        for name in kinds:
            out[name].append(round(timed_ms(steppers[name], steps), 4))
    return out, {name: statistics.median(v) for name, v in out.items()}


def head_launch_us(d, dev, calls):
    """the fused head launch alone (kernel + the row-sum launch(es) behind it), HIP events around every call: median us per form"""
    from cvc import hip
    M, K, V = d.B * d.T, d.R, d.V
    g = torch.Generator().manual_seed(1)
    x, W, b = torch.randn(M, K, generator=g).to(dev), (torch.randn(V, K, generator=g) * 0.02).to(dev), torch.randn(V, generator=g).to(dev)
    target, w = torch.randint(0, V, (M,), generator=g).to(dev), (torch.rand(M, generator=g) < 0.7).float().to(dev)
    master = hip.tile_mm(x, hip.weight_operand(W), parts_only=True).clone()
    parts = master.clone()
    forms = {"unsmoothed_entry": lambda: hip.vocab_head_nll_fwd(parts, b, target, w),
             "ls_entry_eps_0": lambda: hip.vocab_head_nll_ls_fwd(parts, b, target, w, 0.0),
             "ent_entry_beta_0": lambda: hip.vocab_head_nll_ent_fwd(parts, b, target, w, w, 0.0, 0.0),
             "ent_entry_beta_0.05": lambda: hip.vocab_head_nll_ent_fwd(parts, b, target, w, w, 0.0, BETA)}
    out = {}
    for name, fn in forms.items():
        times = []
        for i in range(calls + 5):
            parts.copy_(master)                       # (pre aliases slab 0: every call reads the head's real partial sums)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= 5:
                times.append(1e3 * e0.elapsed_time(e1))
        out[name] = round(statistics.median(times), 2)
    out["slabs"], out["rows"], out["V"] = int(master.shape[0]), M, V
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--head_calls", type=int, default=50)
    ap.add_argument("--scst_samples", type=int, default=5)
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    from cvc import synth, hip
    from cvc.cider import CiderD
    dev = torch.device("cuda:0")
    d = synth.CONFIGS[args.config]
    batch = make_batch(d, dev, args.seed)
    kinds = ["off", "beta_0.05", "off_second"]
    betas = {"off": None, "beta_0.05": BETA, "off_second": None}
    # ---- the captured cross-entropy step
    xe = {name: build_trainer(d, dev, args.seed, True, **({} if b is None else dict(confidence_penalty=b))) for name, b in betas.items()}
    last = {}
    for name, tr in xe.items():                             # capture (3 warm-up steps inside) + warm replays
        for _ in range(args.warmup):
            last[name] = tr.train_step_graphed(batch).tolist()
    xe_rounds, xe_med = alternate(kinds, {n: (lambda tr=tr: tr.train_step_graphed(batch)) for n, tr in xe.items()}, args.rounds, args.steps)
    del xe
    # ---- the eager self-critical step
    corpus = list(synth.captions(d, args.seed)) + list(synth.captions(dataclasses.replace(d, B=60), args.seed + 1))
    sc = {}
    for name, b in betas.items():
        tr = build_trainer(d, dev, args.seed, False, scst_samples=args.scst_samples, scst_temperature=1.0, scst_seed=1, scst_dropout=False,
                           **({} if b is None else dict(scst_entropy=b)))
        tr._cider = CiderD.from_captions(corpus, dev)
        for _ in range(args.warmup):
            tr.scst_step(batch)
        sc[name] = tr
    sc_rounds, sc_med = alternate(kinds, {n: (lambda tr=tr: tr.scst_step(batch)) for n, tr in sc.items()}, args.rounds, args.steps)
    entropy = float(sc["beta_0.05"].last_scst["entropy"])
    del sc
    head = head_launch_us(d, dev, args.head_calls)
    head_diff_ms = (head["ent_entry_beta_0.05"] - head["unsmoothed_entry"]) / 1e3

    def verdict(med, heads):
        cost, spread = med["beta_0.05"] - med["off"], abs(med["off"] - med["off_second"])
        return dict(cost_ms=round(cost, 4), spread_between_off_trainers_ms=round(spread, 4), head_launch_difference_ms=round(heads * head_diff_ms, 4),
                    within_spread_plus_head=bool(cost <= spread + heads * head_diff_ms))
    line = {"tool": "bench_entropy", "config": args.config, "lib": hip.version(), "steps_per_round": args.steps, "rounds": args.rounds, "beta": BETA,
            "xe_ms_per_step_median": {k: round(v, 4) for k, v in xe_med.items()}, "xe_ms_per_step_rounds": xe_rounds,
            "xe": verdict(xe_med, 2), "scst_samples": args.scst_samples,
            "scst_ms_per_step_median": {k: round(v, 4) for k, v in sc_med.items()}, "scst_ms_per_step_rounds": sc_rounds,
            "scst": verdict(sc_med, 1), "scst_entropy_last_step": round(entropy, 5), "head_launch_us_median": head,
            "last_xe_step": {k: [round(x, 5) for x in v] for k, v in last.items()},
            "note": "one rank, no gradient exchange; captured cross-entropy step (Trainer.train_step_graphed, two heads per step), eager "
                    "self-critical step (Trainer.scst_step, one head); the steps with the term carry the mean entropy as a last element"}
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench_entropy_%s.json" % args.config), "w") as f:
        json.dump(line, f, indent=1)
        f.write("\n")
    with open(os.path.join(args.out, "entropy.md"), "w") as f:
        f.write("# Entropy regulariser: cost at %s (tools/bench_entropy.py)\n\n" % args.config)
        for title, rounds, med, key in (("Captured cross-entropy step (confidence_penalty)", xe_rounds, xe_med, "xe"),
                                        ("Eager self-critical step, %d rollouts per clip (scst_entropy)" % args.scst_samples, sc_rounds, sc_med, "scst")):
            f.write("%s, %d rounds of %d steps per trainer, alternated in one process; median of the rounds.\n\n" % (title, args.rounds, args.steps))
            f.write("| trainer | ms / step (median) | rounds |\n|---|---|---|\n")
            for name in kinds:
                f.write("| %s | %.4f | %s |\n" % (name, med[name], ", ".join("%.4f" % x for x in rounds[name])))
            v = line[key]
            f.write("\nbeta = %g against the first trainer without it: %+.4f ms / step; spread between the two trainers without it: %.4f ms; "
                    "the head launches' own difference: %.4f ms -- %s.\n\n"
                    % (BETA, v["cost_ms"], v["spread_between_off_trainers_ms"], v["head_launch_difference_ms"],
                       "within spread + head" if v["within_spread_plus_head"] else "MORE than spread + head"))
        f.write("Fused head launch alone (%d rows x %d words, %d slabs; HIP events, median of %d calls, the row-sum launches included):\n\n"
                % (head["rows"], head["V"], head["slabs"], args.head_calls))
        f.write("| entry | us |\n|---|---|\n")
        for k in ("unsmoothed_entry", "ls_entry_eps_0", "ent_entry_beta_0", "ent_entry_beta_0.05"):
            f.write("| %s | %.2f |\n" % (k, head[k]))
    print(json.dumps(line))


if __name__ == "__main__":
    main()
