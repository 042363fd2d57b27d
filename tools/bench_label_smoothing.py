#!/usr/bin/env python3
"""What label smoothing costs: config 3's captured cross-entropy step (cyclical pass, backward, clip, Adam; train-mode dropout; one
rank, no gradient exchange) with label_smoothing = 0, = 0.1 and a SECOND trainer at 0, the three alternated in one process -- the
median of the rounds per trainer.  The 0.1 step is judged against the first 0 step of the same alternation; the margin is the spread
between the two 0 trainers, which run identical launches.  The fused head launch (cvc_vocab_head_nll_fwd / cvc_vocab_head_nll_ls_fwd
at config 3's head size, 1280 rows x 5000 words, with the row sums behind it) is timed alone by HIP events, median of --head_calls.
Writes profiles/label_smoothing.md and profiles/bench_label_smoothing_cfg3.json and prints the JSON line.

  python tools/bench_label_smoothing.py [--steps 30] [--rounds 5] [--warmup 5] [--config cfg3] [--out profiles]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "cyclical-visual-captioning_amd"))

EPS = 0.1


def build_trainer(d, dev, eps, seed):
    """bench_train.run_train's model and options at the dims d, one rank, a capturable optimizer, label_smoothing = eps"""
    from cvc import synth, opts as cvc_opts
    from cvc.model.captioner import DecodeAndGroundCaptionerGVDROI, PrecomputedRegionFeatures
    from cvc.trainer import Trainer, build_optimizer
    o = cvc_opts.parse_opt([])
    o.vocab_size, o.itow, o.wtoi = d.V, {str(i): "w%d" % i for i in range(d.V)}, {"UNK": synth.UNK_IDX}
    o.seq_length, o.rnn_size, o.input_encoding_size, o.att_hid_size = d.T, d.R, d.E, d.A
    o.detect_size, o.vis_encoding_size, o.train_decoder_only = d.DET, d.G, False
    o.xe_loss_weight, o.caption_consistency_loss_weight, o.learning_rate, o.batch_size = 0.5, 0.5, 1e-4, d.B
    o.label_smoothing = eps
    model = DecodeAndGroundCaptionerGVDROI(o, roi_extractor=PrecomputedRegionFeatures(d.DET, d.G))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.hot_path_state_dict(d, seed).items()}, strict=False)
    model = model.to(dev).train()
    return Trainer(o, None, model, build_optimizer(model, o, capturable=True), None, None)


def make_batch(d, dev, seed):
    from cvc import synth
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    feats = {k: t(v) for k, v in synth.clip_features(d, seed).items()}
    b = {k: t(v) for k, v in synth.label_glue_batch(d, seed).items()}
    return (feats, b["input_seq"], b["gt_seq"], b["num"].cpu(), b["proposals"], b["gt_bboxs"], b["box_mask"],
            ["v_x_segment_%02d" % i for i in range(d.B)], torch.zeros(d.B, d.N, 1), b["frm_mask"], b["sample_idx"], feats["pnt_mask"][:, 1:])


def step_ms(tr, batch, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.train_step_graphed(batch)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def head_launch_us(d, dev, calls):
    """the fused head launch alone (kernel + the row-sum launches behind it), HIP events around every call: median us per form"""
    from cvc import hip
    M, K, V = d.B * d.T, d.R, d.V
    g = torch.Generator().manual_seed(1)
    x, W, b = torch.randn(M, K, generator=g).to(dev), (torch.randn(V, K, generator=g) * 0.02).to(dev), torch.randn(V, generator=g).to(dev)
    target, w = torch.randint(0, V, (M,), generator=g).to(dev), (torch.rand(M, generator=g) < 0.7).float().to(dev)
    master = hip.tile_mm(x, hip.weight_operand(W), parts_only=True).clone()
    parts = master.clone()
    forms = {"unsmoothed_entry": lambda: hip.vocab_head_nll_fwd(parts, b, target, w),
             "ls_entry_eps_0": lambda: hip.vocab_head_nll_ls_fwd(parts, b, target, w, 0.0),
             "ls_entry_eps_0.1": lambda: hip.vocab_head_nll_ls_fwd(parts, b, target, w, EPS)}
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
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    from cvc import synth, hip
    dev = torch.device("cuda:0")
    d = synth.CONFIGS[args.config]
    batch = make_batch(d, dev, args.seed)
    kinds = [("eps_0", 0.0), ("eps_0.1", EPS), ("eps_0_second", 0.0)]
    trainers = {name: build_trainer(d, dev, eps, args.seed) for name, eps in kinds}
    last = {}
    for name, tr in trainers.items():                       # capture (3 warm-up steps inside) + warm replays
        for _ in range(args.warmup):
            last[name] = tr.train_step_graphed(batch).tolist()
    rounds = {name: [] for name, _ in kinds}
    for _ in range(args.rounds):
        for name, _eps in kinds:
            rounds[name].append(round(step_ms(trainers[name], batch, args.steps), 4))
    med = {name: statistics.median(v) for name, v in rounds.items()}
    spread = abs(med["eps_0"] - med["eps_0_second"])
    cost = med["eps_0.1"] - med["eps_0"]
    head = head_launch_us(d, dev, args.head_calls)
    line = {"tool": "bench_label_smoothing", "config": args.config, "lib": hip.version(), "steps_per_round": args.steps, "rounds": args.rounds,
            "ms_per_step_median": {k: round(v, 4) for k, v in med.items()}, "ms_per_step_rounds": rounds,
            "smoothing_cost_ms": round(cost, 4), "spread_between_eps_0_trainers_ms": round(spread, 4),
            "smoothing_cost_within_spread": bool(cost <= spread), "head_launch_us_median": head,
            "last_step": {k: [round(x, 5) for x in v] for k, v in last.items()},
            "note": "one rank, no gradient exchange; captured step (Trainer.train_step_graphed), train-mode dropout; the 0.1 step's "
                    "result carries a sixth element, loop A's unsmoothed NLL"}
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench_label_smoothing_%s.json" % args.config), "w") as f:
        json.dump(line, f, indent=1)
        f.write("\n")
    with open(os.path.join(args.out, "label_smoothing.md"), "w") as f:
        f.write("# Label smoothing: cost at %s (tools/bench_label_smoothing.py)\n\n" % args.config)
        f.write("Captured cross-entropy step, %d rounds of %d steps per trainer, alternated in one process; median of the rounds.\n\n"
                % (args.rounds, args.steps))
        f.write("| trainer | ms / step (median) | rounds |\n|---|---|---|\n")
        for name, _eps in kinds:
            f.write("| %s | %.4f | %s |\n" % (name, med[name], ", ".join("%.4f" % x for x in rounds[name])))
        f.write("\nSmoothing (0.1 against the first 0 trainer): %+.4f ms / step; spread between the two 0 trainers: %.4f ms -- %s.\n\n"
                % (cost, spread, "within the spread" if cost <= spread else "MORE than the spread"))
        f.write("Fused head launch alone (%d rows x %d words, %d slabs; HIP events, median of %d calls, the row-sum launches included):\n\n"
                % (head["rows"], head["V"], head["slabs"], args.head_calls))
        f.write("| entry | us |\n|---|---|\n")
        for k in ("unsmoothed_entry", "ls_entry_eps_0", "ls_entry_eps_0.1"):
            f.write("| %s | %.2f |\n" % (k, head[k]))
    print(json.dumps(line))


if __name__ == "__main__":
    main()
