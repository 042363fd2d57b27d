#!/usr/bin/env python3
"""The three optimizer rules behind the clip (cvc.optim.ClipAdam / ClipSGD / ClipAdamax, csrc/optim.hip) against
nn.utils.clip_grad_norm_ + the torch optimizer's step(), at config 3's parameter set (every parameter that gets a gradient in a
training step, with its shape), both sides in ONE process, eager and captured into a graph, alternated round by round -- the median
of the rounds, ms per clip + step.  The native side's achieved GB/s is taken against the bytes the three launches move,
4 n (1 + loads + stores): the norm pass reads g; the update reads p, g and the rule's state and writes p, the state and the clipped
gradient.  Then config 3's training step (cyclical pass, backward, clip, step; train-mode dropout, one rank) with --optim sgd and
--optim adamax, eager against captured, which the library optimizers could not do.
Writes <out>/optim_rules.md and <out>/bench_optim_<config>.json and prints the JSON line.

  python tools/bench_optim.py [--calls 50] [--rounds 5] [--steps 20] [--warmup 5] [--config cfg3] [--out profiles]
"""
import argparse
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

from bench_entropy import build_trainer                # noqa: E402  (bench_train's model and options, one rank)
from bench_label_smoothing import make_batch           # noqa: E402

GRAD_CLIP = 0.1                                          # opts.grad_clip's default
# (loads, stores) of the update launch per element, the clipped gradient's write-back included
TRAFFIC = {"adam": (4, 4), "sgd": (3, 3), "adamax": (4, 4)}


def compiler_report(kernels=r"optim_\w+?_kernel"):
    """csrc/optim.hip compiled as the library's build compiles it, with hipcc's resource remarks -> {kernel: {VGPRs, SGPRs, LDS,
    scratch, sgpr_spills, vgpr_spills, occupancy}} of the source this run measures (None where hipcc is not at hand)"""
    import re
    import subprocess
    import tempfile
    import build_hip
    src = os.path.join(build_hip.CSRC, "optim.hip")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [build_hip.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-Wno-comment", "-c", src,
               "-o", os.path.join(tmp, "optim.o"), "-Rpass-analysis=kernel-resource-usage"] + build_hip.extra_flags().split()
        try:
            err = subprocess.run(cmd, stderr=subprocess.PIPE, text=True, check=True).stderr
        except (OSError, subprocess.CalledProcessError):
            return None
    fields = {"VGPRs": "VGPRs", "SGPRs": "TotalSGPRs", "LDS": r"LDS Size \[bytes/block\]", "scratch": r"ScratchSize \[bytes/lane\]",
              "sgpr_spills": "SGPRs Spill", "vgpr_spills": "VGPRs Spill", "occupancy": r"Occupancy \[waves/SIMD\]"}
    out = {}
    for block in err.split("remark: Function Name: ")[1:]:
        name = re.search(kernels, block.split()[0])
        if name:
            out[name.group(0)] = {k: int(re.search(r"remark:\s+%s: (\d+)" % pat, block).group(1)) for k, pat in fields.items()}
    return out


def timed_ms(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / calls


def alternate(steppers, rounds, calls):
    out = {name: [] for name in steppers}
    for _ in range(rounds):
        for name, fn in steppers.items():
            out[name].append(round(timed_ms(fn, calls), 4))
    return out, {name: statistics.median(v) for name, v in out.items()}


def parameter_set(d, dev, seed, batch):
    """shapes, learning rates and weight decay of the parameters of config 3's model that get a gradient in a training step"""
    tr = build_trainer(d, dev, seed, False)
    tr.train_step(batch)
    torch.cuda.synchronize()
    return [(tuple(g["params"][0].shape), g["lr"], g["weight_decay"]) for g in tr.optimizer.param_groups if g["params"][0].grad is not None]


def make_side(rule, native, pset, dev):
    """parameters with gradients at the set's shapes and one optimizer over them -> (params, optimizer)"""
    from cvc.optim import ClipAdam, ClipAdamax, ClipSGD
    g = torch.Generator().manual_seed(3)
    ps = []
    for shape, _lr, _wd in pset:
        p = torch.nn.Parameter((torch.randn(*shape, generator=g) * 0.05).to(dev))
        p.grad = (torch.randn(*shape, generator=g) * 0.01).to(dev)
        ps.append(p)
    groups = [{"params": [p], "lr": lr, "weight_decay": wd} for p, (_s, lr, wd) in zip(ps, pset)]
    if rule == "adam":
        opt = ClipAdam(groups) if native else torch.optim.Adam(groups, capturable=True, fused=True)
    elif rule == "sgd":
        opt = ClipSGD(groups, lr=1e-4, momentum=0.9) if native else torch.optim.SGD(groups, lr=1e-4, momentum=0.9)
    else:
        opt = ClipAdamax(groups) if native else torch.optim.Adamax(groups, capturable=True)
    return ps, opt


def rule_steppers(rule, pset, dev, warmup):
    """native / torch x eager / captured: four callables, each one clip + step"""
    out, keep = {}, []
    for native in (True, False):
        for captured in (False, True):
            ps, opt = make_side(rule, native, pset, dev)
            if native:
                one = lambda opt=opt: opt.clip_and_step(GRAD_CLIP, 1.0)
            else:
                def one(ps=ps, opt=opt):
                    torch.nn.utils.clip_grad_norm_(ps, GRAD_CLIP)
                    opt.step()
            name = ("native" if native else "torch") + ("_captured" if captured else "_eager")
            if captured:
                s = torch.cuda.Stream()
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):
                    for _ in range(3):
                        one()
                torch.cuda.current_stream().wait_stream(s)
                graph = torch.cuda.CUDAGraph()
                try:
                    with torch.cuda.graph(graph, stream=s):
                        one()
                except RuntimeError as e:                # (a library step that cannot be captured is reported, not timed)
                    if native:
                        raise
                    print("bench_optim: torch's %s step was not captured: %s" % (rule, str(e).splitlines()[0]), flush=True)
                    continue
                keep.append((ps, opt, graph))
                out[name] = graph.replay
            else:
                keep.append((ps, opt))
                out[name] = one
            for _ in range(warmup):
                out[name]()
    torch.cuda.synchronize()
    return out, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    from cvc import synth, hip
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim: needs the GPU (no timing is taken anywhere else)")
    dev = torch.device("cuda:0")
    d = synth.CONFIGS[args.config]
    batch = make_batch(d, dev, args.seed)
    pset = parameter_set(d, dev, args.seed, batch)
    n = sum(int(torch.Size(s).numel()) for s, _lr, _wd in pset)
    report = compiler_report()
    rules = {}
    for rule in ("adam", "sgd", "adamax"):
        steppers, keep = rule_steppers(rule, pset, dev, args.warmup)
        rounds, med = alternate(steppers, args.rounds, args.calls)
        loads, stores = TRAFFIC[rule]
        nbytes = 4 * n * (1 + loads + stores)
        captured = "torch_captured" in med                        # (a library step that was not captured has no figure: null)
        rules[rule] = dict(ms_median=dict({k: round(v, 4) for k, v in med.items()}, **({} if captured else {"torch_captured": None})),
                           ms_rounds=rounds, bytes=nbytes,
                           native_gb_per_s={k: round(nbytes / (med[k] * 1e-3) / 1e9, 1) for k in ("native_eager", "native_captured")},
                           speedup_eager=round(med["torch_eager"] / med["native_eager"], 3),
                           speedup_captured=round(med["torch_captured"] / med["native_captured"], 3) if captured else None)
        del steppers, keep
    # ---- config 3's training step under the two rules, eager against captured
    train = {}
    for optim in ("sgd", "adamax"):
        trs = {mode: build_trainer(d, dev, args.seed, True, optim=optim, hip_graph=1) for mode in ("eager", "captured")}
        assert all(tr.graph_capable() and tr._can_defer() for tr in trs.values()), optim
        steppers = {"eager": lambda tr=trs["eager"]: tr.train_step(batch), "captured": lambda tr=trs["captured"]: tr.train_step_graphed(batch)}
        last = {}
        for name, fn in steppers.items():
            for _ in range(args.warmup):
                last[name] = float(fn()[0])
        rounds, med = alternate(steppers, args.rounds, args.steps)
        train[optim] = dict(optimizer=type(trs["eager"].optimizer).__name__, ms_median={k: round(v, 4) for k, v in med.items()}, ms_rounds=rounds,
                            last_warmup_loss=last)
        del trs, steppers
    import build_hip
    line = {"tool": "bench_optim", "config": args.config, "lib": hip.version(), "source_hash": build_hip.source_hash(), "parameters_with_gradient": len(pset), "elements": n,
            "calls_per_round": args.calls, "steps_per_round": args.steps, "rounds": args.rounds, "grad_clip": GRAD_CLIP, "rules": rules,
            "train_step": train, "compiler_report": report,
            "note": "one rank; clip + step alone on config 3's parameter shapes (native: three launches; torch: clip_grad_norm_ + "
                    "Adam(fused, capturable) / SGD(momentum 0.9) / Adamax(capturable)), then the whole training step; host clock around "
                    "calls that end in a device synchronise, rounds alternated in one process, medians"}
    os.makedirs(args.out, exist_ok=True)
    ms = lambda x: "not captured" if x is None else "%.4f" % x
    ratio = lambda x: "not captured" if x is None else "%.2f" % x
    with open(os.path.join(args.out, "bench_optim_%s.json" % args.config), "w") as f:
        json.dump(line, f, indent=1)
        f.write("\n")
    with open(os.path.join(args.out, "optim_rules.md"), "w") as f:
        f.write("# SGD-momentum and Adamax steps behind the clip: cost at %s (tools/bench_optim.py)\n\n" % args.config)
        f.write("%d parameters with a gradient, %d elements (%.1f MB of fp32).  Clip + step alone, %d rounds of %d calls per form, "
                "alternated in one process on an MI355X; median of the rounds.  torch = `nn.utils.clip_grad_norm_` + the torch "
                "optimizer's `step()` (Adam fused and capturable, SGD momentum 0.9, Adamax capturable).  Kernel sources %s "
                "(`build_hip.source_hash()`).\n\n" % (len(pset), n, 4 * n / 1e6, args.rounds, args.calls, line["source_hash"]))
        f.write("| rule | native eager ms | torch eager ms | eager: torch / native | native captured ms | torch captured ms | captured: torch / native "
                "| bytes moved | native GB/s (eager / captured) |\n|---|---|---|---|---|---|---|---|---|\n")
        for rule, r in rules.items():
            m = r["ms_median"]
            f.write("| %s | %s | %s | %s | %s | %s | %s | %.1f MB | %.0f / %.0f |\n"
                    % (rule, ms(m["native_eager"]), ms(m["torch_eager"]), ratio(r["speedup_eager"]), ms(m["native_captured"]),
                       ms(m["torch_captured"]), ratio(r["speedup_captured"]), r["bytes"] / 1e6, r["native_gb_per_s"]["native_eager"],
                       r["native_gb_per_s"]["native_captured"]))
        slower = [(rule, k) for rule, r in rules.items() for k in ("eager", "captured") if r["speedup_" + k] is not None and r["speedup_" + k] < 1.0]
        missing = [rule for rule, r in rules.items() if r["speedup_captured"] is None]
        f.write("\n" + ("NOT faster than the torch baseline: %s.\n" % ", ".join("%s (%s)" % s_ for s_ in slower) if slower
                        else "Every rule is faster than its torch baseline in every form that was measured.\n"))
        if missing:
            f.write("torch's step could not be captured, so there is no captured baseline, for: %s.\n" % ", ".join(missing))
        f.write("\nBytes moved = 4 n (1 + loads + stores): the norm pass reads g, the update reads p, g and the state and writes p, the state "
                "and the clipped gradient (Adam and Adamax 4 + 4, SGD 3 + 3).  GB/s is that over the median time of the three launches "
                "together, launch gaps included -- an end-to-end figure, not a kernel's share of the memory roof.\n\n")
        f.write("## %s's training step, eager against captured\n\n" % args.config)
        f.write("Cyclical pass, backward, clip, step; train-mode dropout, one rank, no exchange; %d rounds of %d steps.  The library "
                "optimizers these two rules ran on before could not be captured (`Trainer.graph_capable()` was false), so there was no "
                "captured column.\n\n" % (args.rounds, args.steps))
        f.write("| --optim | optimizer | eager ms / step | captured ms / step | rounds eager | rounds captured |\n|---|---|---|---|---|---|\n")
        for optim, r in train.items():
            f.write("| %s | %s | %.3f | %.3f | %s | %s |\n" % (optim, r["optimizer"], r["ms_median"]["eager"], r["ms_median"]["captured"],
                                                             ", ".join("%.3f" % x for x in r["ms_rounds"]["eager"]),
                                                             ", ".join("%.3f" % x for x in r["ms_rounds"]["captured"])))
        f.write("\n## Compiler report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, of the source this run measured)\n\n")
        if report is None:
            f.write("Not taken: hipcc was not at hand where the tool ran.\n")
        else:
            f.write("| kernel | threads | VGPRs | SGPRs | LDS bytes | scratch | spills | occupancy |\n|---|---|---|---|---|---|---|---|\n")
            for k, r in report.items():
                f.write("| `%s` | 256 | %d | %d | %d | %d | %d | %d |\n" % (k, r["VGPRs"], r["SGPRs"], r["LDS"], r["scratch"],
                                                                        r["sgpr_spills"] + r["vgpr_spills"], r["occupancy"]))
            f.write("\nThe build refuses scratch and spills for the three update kernels (`build_hip.NO_SCRATCH_KERNELS`).\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
