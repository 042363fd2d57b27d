#!/usr/bin/env python3
"""What word-level distillation costs at config 3, in one process (one rank, no gradient exchange, train-mode dropout):

  * the eager distilled step (teacher pass, cyclical pass, backward, clip, Adam: Trainer.train_step_prepared with model.distill set)
    against the eager cross-entropy step of the SAME trainer (model.distill = None), with a second, identical trainer's
    cross-entropy step beside them: the spread between the two identical trainers is the margin of any difference;
  * the teacher pass alone (CaptionEnsemble.soft_targets: every member's encoder and the forced ensemble engine with kept rows) for
    M = 1, 2 and 3 members;
  * the KD head launch alone (cvc_vocab_head_nll_kd_fwd) against cvc_vocab_head_nll_ls_fwd at the same rows, HIP events around every
    call, median; with the bytes each launch must move (computed from the shapes) the achieved bytes per second of both.

The forms are alternated round by round; the figure per form is the median of the rounds.
Writes profiles/distill.md and profiles/bench_distill_<config>.json and prints the JSON line.

  python tools/bench_distill.py [--steps 20] [--rounds 5] [--warmup 5] [--config cfg3] [--members 2] [--out profiles]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "cyclical-visual-captioning_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_label_smoothing import make_batch          # noqa: E402  (the same batch as the label-smoothing measurement)
from bench_entropy import build_trainer, timed_ms, alternate          # noqa: E402

ALPHA, TAU = 0.5, 2.0


def teacher_of(d, dev, members, seed):
    """a CaptionEnsemble of `members` frozen models of the dims d, seeds seed + 101, + 102, ..."""
    from cvc import synth, opts as cvc_opts
    from cvc.model.captioner import DecodeAndGroundCaptionerGVDROI, PrecomputedRegionFeatures
    from cvc.model.ensemble import CaptionEnsemble
    models = []
    for m in range(members):
        o = cvc_opts.parse_opt([])
        o.vocab_size, o.itow, o.wtoi = d.V, {str(i): "w%d" % i for i in range(d.V)}, {"UNK": synth.UNK_IDX}
        o.seq_length, o.rnn_size, o.input_encoding_size, o.att_hid_size = d.T, d.R, d.E, d.A
        o.detect_size, o.vis_encoding_size, o.train_decoder_only = d.DET, d.G, False
        model = DecodeAndGroundCaptionerGVDROI(o, roi_extractor=PrecomputedRegionFeatures(d.DET, d.G))
        model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.hot_path_state_dict(d, seed + 101 + m).items()}, strict=False)
        models.append(model.to(dev).eval().requires_grad_(False))
    return CaptionEnsemble(models)


def eleven(b):
    return (b["segs_feat"], b["input_seqs"], b["gt_seqs"], b["num"], b["ppls"], b["gt_bboxs"], b["mask_bboxs"], b["ppls_feat"], b["mask_frms"],
            b["sample_idx"], b["pnt_mask"])


def head_launch(d, dev, calls):
    """the fused head launch alone (kernel + the row-sum launch behind it), HIP events around every call -> median us per form, the
    bytes each must move and the achieved bytes per second"""
    from cvc import hip
    M, K, V = d.B * d.T, d.R, d.V
    g = torch.Generator().manual_seed(1)
    x, W, b = torch.randn(M, K, generator=g).to(dev), (torch.randn(V, K, generator=g) * 0.02).to(dev), torch.randn(V, generator=g).to(dev)
    target, w = torch.randint(0, V, (M,), generator=g).to(dev), (torch.rand(M, generator=g) < 0.7).float().to(dev)
    teacher = torch.log_softmax(torch.randn(M, V, generator=g) * 2.0, 1).to(dev)
    master = hip.tile_mm(x, hip.weight_operand(W), parts_only=True).clone()
    parts = master.clone()
    slabs = int(master.shape[0])
    forms = {"ls_entry_eps_0.1": lambda: hip.vocab_head_nll_ls_fwd(parts, b, target, w, 0.1),
             "kd_entry_tau_1": lambda: hip.vocab_head_nll_kd_fwd(parts, b, target, w, teacher, ALPHA, 1.0),
             "kd_entry_tau_2": lambda: hip.vocab_head_nll_kd_fwd(parts, b, target, w, teacher, ALPHA, TAU)}
    base = 4 * (slabs * M * V + V + M * V + 4 * M)              # the slabs and the bias in, pre out, target / weight / rows
    need = {"ls_entry_eps_0.1": base, "kd_entry_tau_1": base + 4 * M * V, "kd_entry_tau_2": base + 4 * M * V}
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
        us = statistics.median(times)
        out[name] = dict(us=round(us, 2), bytes=need[name], gb_per_s=round(need[name] / (us * 1e-6) / 1e9, 1))
    out["slabs"], out["rows"], out["V"] = slabs, M, V
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--head_calls", type=int, default=50)
    ap.add_argument("--members", type=int, default=2, help="members of the distilled step's teacher")
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    from cvc import synth, hip
    dev = torch.device("cuda:0")
    d = synth.CONFIGS[args.config]
    batch = make_batch(d, dev, args.seed)
    # ---- the eager steps: one trainer with and without model.distill, a second identical trainer without
    tr, tr2 = build_trainer(d, dev, args.seed, False), build_trainer(d, dev, args.seed, False)
    b = tr._prepare(batch, True)
    teachers = {m: teacher_of(d, dev, m, args.seed) for m in (1, 2, 3)}
    kd = dict(teacher=teachers[args.members], alpha=ALPHA, tau=TAU)
    last = {}

    def step(trainer, distill, name):
        def run():
            trainer.model.distill = distill
            last[name] = trainer.train_step_prepared(b)
        return run
    steppers = {"xe": step(tr, None, "xe"), "distilled": step(tr, kd, "distilled"), "xe_second": step(tr2, None, "xe_second")}
    kinds = list(steppers)
    for name in kinds:
        for _ in range(args.warmup):
            steppers[name]()
    step_rounds, step_med = alternate(kinds, steppers, args.rounds, args.steps)
    last = {k: [round(float(x), 5) for x in v] for k, v in last.items()}
    tr.model.distill = None
    # ---- the teacher pass alone
    t_kinds = ["M1", "M2", "M3"]
    t_steppers = {"M%d" % m: (lambda t=teachers[m]: t.soft_targets(*eleven(b))) for m in (1, 2, 3)}
    for name in t_kinds:
        for _ in range(args.warmup):
            t_steppers[name]()
    t_rounds, t_med = alternate(t_kinds, t_steppers, args.rounds, args.steps)
    head = head_launch(d, dev, args.head_calls)
    cost, spread = step_med["distilled"] - step_med["xe"], abs(step_med["xe"] - step_med["xe_second"])
    line = {"tool": "bench_distill", "config": args.config, "lib": hip.version(), "steps_per_round": args.steps, "rounds": args.rounds,
            "alpha": ALPHA, "tau": TAU, "teacher_members_of_the_step": args.members,
            "step_ms_median": {k: round(v, 4) for k, v in step_med.items()}, "step_ms_rounds": step_rounds,
            "distilled_minus_xe_ms": round(cost, 4), "spread_between_xe_trainers_ms": round(spread, 4),
            "teacher_pass_ms_median": {k: round(v, 4) for k, v in t_med.items()}, "teacher_pass_ms_rounds": t_rounds,
            "head_launch": head, "last_step": last,
            "note": "one rank, no gradient exchange, eager steps (Trainer.train_step_prepared); the distilled step carries the unmixed NLL "
                    "and the KD as its last two elements; the teacher's forced engine is captured when the options ask for HIP graphs"}
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench_distill_%s.json" % args.config), "w") as f:
        json.dump(line, f, indent=1)
        f.write("\n")
    with open(os.path.join(args.out, "distill.md"), "w") as f:
        f.write("# Word-level distillation: cost at %s (tools/bench_distill.py)\n\n" % args.config)
        f.write("Eager steps, alpha = %g, tau = %g, a teacher of %d checkpoints; %d rounds of %d steps per form, alternated in one process; "
                "median of the rounds.\n\n" % (ALPHA, TAU, args.members, args.rounds, args.steps))
        f.write("| step | ms / step (median) | rounds |\n|---|---|---|\n")
        for name in kinds:
            f.write("| %s | %.4f | %s |\n" % (name, step_med[name], ", ".join("%.4f" % x for x in step_rounds[name])))
        f.write("\nThe distilled step against the cross-entropy step of the same trainer: %+.4f ms / step; spread between the two identical "
                "trainers' cross-entropy steps: %.4f ms.\n\n" % (cost, spread))
        f.write("The teacher pass alone (every member's encoder, the forced ensemble engine with kept rows):\n\n")
        f.write("| members | ms / pass (median) | rounds |\n|---|---|---|\n")
        for name in t_kinds:
            f.write("| %s | %.4f | %s |\n" % (name[1:], t_med[name], ", ".join("%.4f" % x for x in t_rounds[name])))
        f.write("\nFused head launch alone (%d rows x %d words, %d slabs; HIP events, median of %d calls, the row-sum launch included; bytes: "
                "what the launch must move, from the shapes -- the KD launch reads one more [rows, V] fp32 tensor):\n\n"
                % (head["rows"], head["V"], head["slabs"], args.head_calls))
        f.write("| entry | us | MB | GB / s |\n|---|---|---|---|\n")
        for k in ("ls_entry_eps_0.1", "kd_entry_tau_1", "kd_entry_tau_2"):
            f.write("| %s | %.2f | %.1f | %.1f |\n" % (k, head[k]["us"], head[k]["bytes"] / 1e6, head[k]["gb_per_s"]))
    print(json.dumps(line))


if __name__ == "__main__":
    main()
