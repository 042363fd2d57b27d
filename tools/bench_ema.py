#!/usr/bin/env python3
"""What the weight average inside the optimizer step costs (cvc.optim._ClipStep.attach_ema, the _ema entries of csrc/optim.hip), by
tools/bench_optim.py's method: config 3's parameter set, every form in ONE process, alternated round by round, the median of the
rounds, ms per call.  For each of the three rules, eager and captured into a graph:
    plain        clip + step
    fused        clip + step with the average kept in the update launch
    plain+lerp   clip + step, then torch._foreach_lerp_(shadows, parameters, 1 - d) over the same tensors
Then the exchange (swap_ema), and config 3's captured training step without the average (two identical trainers: their difference
is the spread) and with it.  Achieved GB/s is taken against the bytes the launches move, 4 n x streams: the plain step's
1 + loads + stores of tools/bench_optim.py, + 2 for the fused average (e read, e written), + 3 for a separate lerp (p and e read, e
written), 4 for the swap.
Writes <out>/ema.md and <out>/bench_ema_<config>.json and prints the JSON line.

  python tools/bench_ema.py [--calls 50] [--rounds 5] [--steps 20] [--warmup 5] [--config cfg3] [--out profiles]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "cyclical-visual-captioning_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_optim as BO                               # noqa: E402
from bench_entropy import build_trainer                # noqa: E402
from bench_label_smoothing import make_batch           # noqa: E402

DECAY = 0.999
FORMS = ("plain", "fused", "plain+lerp")
EXTRA_STREAMS = {"plain": 0, "fused": 2, "plain+lerp": 3}


def steppers_of(rule, pset, dev, warmup):
    out, keep = {}, []
    for form in FORMS:
        for captured in (False, True):
            ps, opt = BO.make_side(rule, True, pset, dev)
            if form == "fused":
                opt.attach_ema(DECAY)
                one = lambda opt=opt: opt.clip_and_step(BO.GRAD_CLIP, 1.0)
            elif form == "plain+lerp":
                shadows = [p.detach().clone() for p in ps]
                datas = [p.data for p in ps]

                def one(opt=opt, shadows=shadows, datas=datas):
                    opt.clip_and_step(BO.GRAD_CLIP, 1.0)
                    torch._foreach_lerp_(shadows, datas, 1.0 - DECAY)
                keep.append(shadows)
            else:
                one = lambda opt=opt: opt.clip_and_step(BO.GRAD_CLIP, 1.0)
            name = form + ("_captured" if captured else "_eager")
            if captured:
                s = torch.cuda.Stream()
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):
                    for _ in range(3):
                        one()
                torch.cuda.current_stream().wait_stream(s)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=s):
                    one()
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
        raise SystemExit("bench_ema: needs the GPU (no timing is taken anywhere else)")
    dev = torch.device("cuda:0")
    d = synth.CONFIGS[args.config]
    batch = make_batch(d, dev, args.seed)
    pset = BO.parameter_set(d, dev, args.seed, batch)
    n = sum(int(torch.Size(s).numel()) for s, _lr, _wd in pset)
    report = BO.compiler_report(r"(optim_\w+?|ema_swap)_kernel")         # (the exchange kernel too)
    rules = {}
    for rule in ("adam", "sgd", "adamax"):
        steppers, keep = steppers_of(rule, pset, dev, args.warmup)
        rounds, med = BO.alternate(steppers, args.rounds, args.calls)
        loads, stores = BO.TRAFFIC[rule]
        base = 1 + loads + stores
        rules[rule] = dict(ms_median={k: round(v, 4) for k, v in med.items()}, ms_rounds=rounds,
                           streams={f: base + EXTRA_STREAMS[f] for f in FORMS},
                           gb_per_s={k: round(4 * n * (base + EXTRA_STREAMS[k.rsplit("_", 1)[0]]) / (v * 1e-3) / 1e9, 1) for k, v in med.items()},
                           fused_over_plain_ms={m: round(med["fused_" + m] - med["plain_" + m], 4) for m in ("eager", "captured")},
                           lerp_over_plain_ms={m: round(med["plain+lerp_" + m] - med["plain_" + m], 4) for m in ("eager", "captured")},
                           fused_is_faster={m: bool(med["fused_" + m] < med["plain+lerp_" + m]) for m in ("eager", "captured")})
        if rule == "adam":                                   # the exchange, on the fused optimizer's own shadows
            opt = next(k[1] for k in keep if isinstance(k, tuple) and len(k) == 2 and k[1].ema_active)
            sw_rounds, sw = BO.alternate({"swap": opt.swap_ema}, args.rounds, 2 * (args.calls // 2))       # an even count: back where it was
            shadowed = sum(e.numel() for e in opt._ema_shadow.values())
            swap = dict(ms_median=round(sw["swap"], 4), ms_rounds=sw_rounds["swap"], elements=shadowed,
                        gb_per_s=round(4 * shadowed * 4 / (sw["swap"] * 1e-3) / 1e9, 1))
        del steppers, keep
    # ---- config 3's captured training step: two identical trainers without the average (the spread), one with it
    trs = {"plain_a": build_trainer(d, dev, args.seed, True, hip_graph=1), "plain_b": build_trainer(d, dev, args.seed, True, hip_graph=1),
           "ema": build_trainer(d, dev, args.seed, True, hip_graph=1, ema_decay=DECAY)}
    assert trs["ema"].ema_active and not trs["plain_a"].ema_active
    steppers = {k: (lambda tr=tr: tr.train_step_graphed(batch)) for k, tr in trs.items()}
    last = {}
    for name, fn in steppers.items():
        for _ in range(args.warmup):
            last[name] = float(fn()[0])
    t_rounds, t_med = BO.alternate(steppers, args.rounds, args.steps)
    train = dict(ms_median={k: round(v, 4) for k, v in t_med.items()}, ms_rounds=t_rounds, last_warmup_loss=last,
                 spread_ms=round(abs(t_med["plain_a"] - t_med["plain_b"]), 4),
                 ema_over_plain_ms=round(t_med["ema"] - 0.5 * (t_med["plain_a"] + t_med["plain_b"]), 4),
                 averaged_steps=trs["ema"].optimizer.ema_updates)
    import build_hip
    line = {"tool": "bench_ema", "config": args.config, "lib": hip.version(), "source_hash": build_hip.source_hash(),
            "device": torch.cuda.get_device_name(0), "parameters_with_gradient": len(pset), "elements": n, "decay": DECAY,
            "calls_per_round": args.calls, "steps_per_round": args.steps, "rounds": args.rounds, "rules": rules, "swap": swap,
            "train_step_captured": train, "compiler_report": report,
            "note": "one rank; host clock around calls that end in a device synchronise, rounds alternated in one process, medians"}
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench_ema_%s.json" % args.config), "w") as f:
        json.dump(line, f, indent=1)
        f.write("\n")
    with open(os.path.join(args.out, "ema.md"), "w") as f:
        f.write("# Weight averaging inside the optimizer step: cost at %s (tools/bench_ema.py)\n\n" % args.config)
        f.write("%s.  %d parameters with a gradient, %d elements (%.1f MB of fp32), decay %g.  %d rounds of %d calls per form, alternated in "
                "one process; median of the rounds, ms per call.  Kernel sources %s (`build_hip.source_hash()`).\n\n"
                % (line["device"], len(pset), n, 4 * n / 1e6, DECAY, args.rounds, args.calls, line["source_hash"]))
        f.write("plain = clip + step; fused = the same with the average kept in the update launch; plain+lerp = clip + step followed by "
                "`torch._foreach_lerp_` over the same tensors.  Streams = passes of 4 n bytes: the plain step's 1 + loads + stores, + 2 "
                "fused (e read, e written), + 3 for a separate lerp.\n\n")
        f.write("| rule | form | streams | eager ms | captured ms | GB/s eager / captured | rounds captured |\n|---|---|---|---|---|---|---|\n")
        for rule, r in rules.items():
            for form in FORMS:
                f.write("| %s | %s | %d | %.4f | %.4f | %.0f / %.0f | %s |\n"
                        % (rule, form, r["streams"][form], r["ms_median"][form + "_eager"], r["ms_median"][form + "_captured"],
                           r["gb_per_s"][form + "_eager"], r["gb_per_s"][form + "_captured"],
                           ", ".join("%.4f" % x for x in r["ms_rounds"][form + "_captured"])))
        f.write("\n| rule | fused - plain, eager / captured ms | (plain+lerp) - plain, eager / captured ms | fused faster than plain+lerp (eager / captured) |\n"
                "|---|---|---|---|\n")
        for rule, r in rules.items():
            f.write("| %s | %+.4f / %+.4f | %+.4f / %+.4f | %s / %s |\n"
                    % (rule, r["fused_over_plain_ms"]["eager"], r["fused_over_plain_ms"]["captured"], r["lerp_over_plain_ms"]["eager"],
                       r["lerp_over_plain_ms"]["captured"], *("yes" if r["fused_is_faster"][m] else "NO" for m in ("eager", "captured"))))
        slower = ["%s (%s)" % (rule, m) for rule, r in rules.items() for m in ("eager", "captured") if not r["fused_is_faster"][m]]
        f.write("\n" + ("The fused average is NOT faster than plain + foreach lerp for: %s.\n" % ", ".join(slower) if slower else
                        "The fused average is faster than plain + foreach lerp for every rule, eager and captured.\n"))
        f.write("\n## The exchange (swap_ema)\n\n%d shadowed elements, 4 streams (p and e read, p and e written): %.4f ms, %.0f GB/s; rounds %s.\n"
                % (swap["elements"], swap["ms_median"], swap["gb_per_s"], ", ".join("%.4f" % x for x in swap["ms_rounds"])))
        f.write("\n## %s's captured training step\n\nCyclical pass, backward, clip, step; train-mode dropout, one rank; %d rounds of %d steps.  "
                "Two identical trainers without the average give the spread.\n\n" % (args.config, args.rounds, args.steps))
        f.write("| trainer | ms / step | rounds |\n|---|---|---|\n")
        for k in ("plain_a", "plain_b", "ema"):
            f.write("| %s | %.3f | %s |\n" % (k, train["ms_median"][k], ", ".join("%.3f" % x for x in train["ms_rounds"][k])))
        f.write("\nThe average costs %+.3f ms per captured step against the mean of the two plain trainers; the two plain trainers differ by "
                "%.3f ms.%s\n" % (train["ema_over_plain_ms"], train["spread_ms"],
                                  "  The cost is inside the spread." if abs(train["ema_over_plain_ms"]) <= train["spread_ms"] else ""))
        f.write("\n## Compiler report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, of the source this run measured)\n\n")
        if report is None:
            f.write("Not taken: hipcc was not at hand where the tool ran.\n")
        else:
            f.write("| kernel | threads | VGPRs | SGPRs | LDS bytes | scratch | spills | occupancy |\n|---|---|---|---|---|---|---|---|\n")
            for k, r in report.items():
                f.write("| `%s` | 256 | %d | %d | %d | %d | %d | %d |\n" % (k, r["VGPRs"], r["SGPRs"], r["LDS"], r["scratch"],
                                                                        r["sgpr_spills"] + r["vgpr_spills"], r["occupancy"]))
            f.write("\nThe build refuses scratch and spills for the update kernels, their averaging forms and the swap "
                    "(`build_hip.NO_SCRATCH_KERNELS`).\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
