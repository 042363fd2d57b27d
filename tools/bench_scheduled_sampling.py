#!/usr/bin/env python3
"""The scheduled-sampling training step next to the eager cross-entropy step, measured in one process (GPU box) at config 3 (B = 64,
T = 20, V = 5000): the eager cross-entropy step; the scheduled-sampling step as a whole and split into rollout (encoder in eval
mode + one decode of the mixed engine), forward + backward + update on the mixed inputs, and DecodeWeights.refresh(); and the same
step with invalidate_decode_cache() in place of refresh() -- every rollout then re-packs the weights, rebuilds the engine and
re-captures its graph.  The kinds of step are timed in alternating rounds (median of the rounds), each window behind one untimed step
of its own kind, so clock and cache drift fall on all alike and no window pays for the kind before it.
Prints one JSON line (times in ms).

  python tools/bench_scheduled_sampling.py [--steps 5] [--rounds 5] [--prob 0.25] [--config cfg3]
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


def ms(fn, steps):
    fn()                                      # untimed: the window's own kind of step came last
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--prob", type=float, default=0.25)
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--seed", type=int, default=1234)
    args = ap.parse_args()
    from cvc import synth, hip, opts as cvc_opts
    from cvc.model.captioner import DecodeAndGroundCaptionerGVDROI, PrecomputedRegionFeatures
    from cvc.trainer import Trainer, build_optimizer
    dev = torch.device("cuda:0")
    d = synth.CONFIGS[args.config]
    o = cvc_opts.parse_opt([])
    o.vocab_size, o.itow, o.wtoi = d.V, {str(i): "w%d" % i for i in range(d.V)}, {"UNK": synth.UNK_IDX}
    o.seq_length, o.rnn_size, o.input_encoding_size, o.att_hid_size = d.T, d.R, d.E, d.A
    o.detect_size, o.vis_encoding_size, o.train_decoder_only = d.DET, d.G, False
    o.xe_loss_weight, o.caption_consistency_loss_weight, o.learning_rate, o.batch_size = 0.5, 0.5, 1e-4, d.B
    o.ss_temperature, o.ss_seed = 1.0, 1
    sd = {k: torch.from_numpy(v) for k, v in synth.hot_path_state_dict(d, args.seed).items()}
    model = DecodeAndGroundCaptionerGVDROI(o, roi_extractor=PrecomputedRegionFeatures(d.DET, d.G))
    model.load_state_dict(sd, strict=False)
    model = model.to(dev).train()
    tr = Trainer(o, None, model, build_optimizer(model, o), None, None)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    feats = {k: t(v) for k, v in synth.clip_features(d, args.seed).items()}
    b = {k: t(v) for k, v in synth.label_glue_batch(d, args.seed).items()}
    batch = (feats, b["input_seq"], b["gt_seq"], b["num"].cpu(), b["proposals"], b["gt_bboxs"], b["box_mask"],
             ["v_x_segment_%02d" % i for i in range(d.B)], torch.zeros(d.B, d.N, 1), b["frm_mask"], b["sample_idx"], feats["pnt_mask"][:, 1:])
    prepared = tr._prepare(batch, True)
    enc_args = [prepared[k] for k in ("segs_feat", "ppls", "num", "mask_bboxs", "ppls_feat", "gt_bboxs", "mask_frms", "sample_idx", "pnt_mask")]
    state = {}
    refresh, invalidate = model.refresh_decode_weights, model.invalidate_decode_cache

    def xe():
        model.ss_prob = 0.0
        tr.train_step_prepared(prepared)

    def ss_step():
        model.ss_prob = args.prob
        tr.train_step_prepared(prepared)

    def ss_step_invalidate():
        model.refresh_decode_weights = invalidate              # the step as it would be without refresh()
        try:
            ss_step()
        finally:
            model.refresh_decode_weights = refresh

    def rollout():
        model.eval()
        with torch.no_grad():
            enc = model.encode_clips(*enc_args)
            state["inputs"] = model.ss_rollout(enc, prepared["gt_seqs"], args.prob, 1.0, 1)
        model.train()

    def forward_backward():
        out = tr._call(prepared, ss_inputs=state["inputs"])
        tr._backward_and_update(tr.loss_mix(out)[0])

    kinds = {"xe_eager": xe, "ss_step": ss_step, "ss_rollout": rollout, "ss_forward_backward": forward_backward, "ss_refresh": refresh,
             "ss_step_invalidate": ss_step_invalidate}
    for fn in kinds.values():                 # warm-up: allocator, lazy workspaces, Adam state, the engine and its graph
        for _ in range(2):
            fn()
    res = {k: [] for k in kinds}
    for _ in range(args.rounds):
        for k, fn in kinds.items():
            res[k].append(ms(fn, args.steps))
    med = {k: round(float(np.median(v)), 3) for k, v in res.items()}
    spread = {k + "_minmax": [round(float(min(v)), 3), round(float(max(v)), 3)] for k, v in res.items()}
    rollout()                                 # (the last kind dropped the engine: bind one to report its path)
    eng = model.ss_engine()
    out = {"metric": "scheduled-sampling step vs eager cross-entropy step, ms per step (median of alternating rounds)", "unit": "ms",
           "lib": hip.version(), "config": args.config, "B": d.B, "T": d.T, "V": d.V, "prob": args.prob, "steps": args.steps,
           "rounds": args.rounds, "engine_path": "packed" if eng.packed else "tile" if eng.tile else "ring", "engine_graph": eng.graph is not None,
           **med, **spread, "ss_over_xe": round(med["ss_step"] / med["xe_eager"], 3),
           "invalidate_over_refresh": round(med["ss_step_invalidate"] / med["ss_step"], 3),
           "sampled_share": round(float(tr.last_ss["share"]), 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
