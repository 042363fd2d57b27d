#!/usr/bin/env python3
"""The self-critical step with rollouts drawn WITHOUT replacement (opts.scst_wor: a stochastic beam of S + 1 slots, importance
weights from cvc_scst_weights_wor) next to the with-replacement step (S independent samples, leave-one-out baseline), measured in
one process (GPU box) at config 3 sizes (B = 64, T = 20, V = 5000) with S = 5.  Each kind has a model and a trainer of its own, from
the same seeded checkpoint; the kinds are timed in alternating rounds (median of the rounds), so clock and cache drift fall on both
alike.  Also reported: the weights launch alone (both blocks, on the last step's tensors), and the share of DUPLICATE captions among
the independent samples -- rows whose words up to the first 0 repeat an earlier row of their clip, the decode and gradient rows the
without-replacement step does not spend -- at the step's temperature and at lower ones (rollouts only).  The checkpoint is the seeded
random one of the benchmarks: near-uniform over the vocabulary at tau = 1, so duplicates appear only when the temperature sharpens it.
No speed is promised: beam S + 1 decodes one row more per clip than S samples do, and the stochastic step is the slowest decode form.
Prints one JSON line (times in ms).

  python tools/bench_scst_wor.py [--steps 5] [--rounds 5] [--samples 5] [--config cfg3] [--temperature 1.0]
"""
import argparse
import copy
import dataclasses
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
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def duplicate_share(seq: torch.Tensor, S: int) -> float:
    """seq [B * S, T]: the share of rows whose caption (the words up to and including the first 0) repeats an earlier row of the clip"""
    s = seq.masked_fill((seq == 0).cumsum(1) > 0, 0).view(-1, S, seq.size(1)).cpu().tolist()
    dup = sum(len(clip) - len({tuple(r) for r in clip}) for clip in s)
    return dup / float(len(s) * S)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--dup_temperatures", default="1.0,0.5,0.25,0.1")
    args = ap.parse_args()
    from cvc import synth, hip, opts as cvc_opts
    from cvc.cider import CiderD
    from cvc.model.captioner import DecodeAndGroundCaptionerGVDROI, PrecomputedRegionFeatures
    from cvc.trainer import Trainer, build_optimizer
    dev = torch.device("cuda:0")
    d, S = synth.CONFIGS[args.config], args.samples
    o = cvc_opts.parse_opt([])
    o.vocab_size, o.itow, o.wtoi = d.V, {str(i): "w%d" % i for i in range(d.V)}, {"UNK": synth.UNK_IDX}
    o.seq_length, o.rnn_size, o.input_encoding_size, o.att_hid_size = d.T, d.R, d.E, d.A
    o.detect_size, o.vis_encoding_size, o.train_decoder_only = d.DET, d.G, False
    o.xe_loss_weight, o.caption_consistency_loss_weight, o.learning_rate, o.batch_size = 0.5, 0.5, 1e-4, d.B
    o.scst_samples, o.scst_temperature, o.scst_seed, o.scst_dropout = S, args.temperature, 1, False
    sd = {k: torch.from_numpy(v) for k, v in synth.hot_path_state_dict(d, args.seed).items()}
    corpus = list(synth.captions(d, args.seed)) + list(synth.captions(dataclasses.replace(d, B=4000), args.seed + 1))
    table = CiderD.from_captions(corpus, dev)

    def fresh(wor):
        oo = copy.copy(o)
        oo.scst_wor = wor
        m = DecodeAndGroundCaptionerGVDROI(oo, roi_extractor=PrecomputedRegionFeatures(d.DET, d.G))
        m.load_state_dict(sd, strict=False)
        m = m.to(dev).train()
        tr = Trainer(oo, None, m, build_optimizer(m, oo, capturable=True), None, None)
        tr._cider = table
        return m, tr
    model_r, tr_r = fresh(False)
    model_w, tr_w = fresh(True)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    feats = {k: t(v) for k, v in synth.clip_features(d, args.seed).items()}
    b = {k: t(v) for k, v in synth.label_glue_batch(d, args.seed).items()}
    batch = (feats, b["input_seq"], b["gt_seq"], b["num"].cpu(), b["proposals"], b["gt_bboxs"], b["box_mask"],
             ["v_x_segment_%02d" % i for i in range(d.B)], torch.zeros(d.B, d.N, 1), b["frm_mask"], b["sample_idx"], feats["pnt_mask"][:, 1:])
    kinds = {"scst_step_with_replacement": lambda: tr_r.scst_step(batch), "scst_step_without_replacement": lambda: tr_w.scst_step(batch)}
    for fn in kinds.values():                 # warm-up: allocator, lazy workspaces, Adam state
        for _ in range(2):
            fn()
    res = {k: [] for k in kinds}
    dups, distinct = [], []
    for _ in range(args.rounds):
        for k, fn in kinds.items():
            res[k].append(ms(fn, args.steps))
        dups.append(duplicate_share(tr_r.last_scst["seq"], S))
        distinct.append(float(tr_w.last_scst["distinct"]))
    # the weights launch alone, on the last steps' tensors
    lr, lw = tr_r.last_scst, tr_w.last_scst
    res["weights_with_replacement"] = [ms(lambda: hip.scst_weights(lr["reward"], None, S, lr["seq"], t_major=True), 200)
                                       for _ in range(args.rounds)]
    res["weights_without_replacement"] = [ms(lambda: hip.scst_weights_wor(lw["reward"], lw["logq"], lw["G"], lw["state"], S, lw["seq"],
                                                                          t_major=True), 200) for _ in range(args.rounds)]
    # duplicates among independent samples at sharper temperatures (rollouts only, the with-replacement model's current weights)
    prepared = tr_r._prepare(batch, True)
    smp_args = [prepared[k] for k in ("segs_feat", "input_seqs", "ppls", "gt_seqs", "num", "mask_bboxs", "gt_bboxs", "ppls_feat", "mask_frms",
                                      "sample_idx", "pnt_mask")]
    model_r.eval()
    dup_at = {}
    with torch.no_grad():
        for tau in (float(x) for x in args.dup_temperatures.split(",") if x):
            seq = model_r._sample(*smp_args, sample_max=0, temperature=tau, sample_n=S, seed=7, beam_size=1, top_k=0, top_p=1.0)[0]
            dup_at[str(tau)] = round(duplicate_share(seq.contiguous(), S), 4)
    med = {k: round(float(np.median(v)), 4) for k, v in res.items()}
    wgt = lw["wgt"].view(-1, S)
    out = {"metric": "self-critical step, rollouts with vs without replacement, ms per step (median of alternating rounds)", "unit": "ms",
           "lib": hip.version(), "config": args.config, "B": d.B, "T": d.T, "V": d.V, "samples_per_clip": S, "rows": d.B * S,
           "temperature": args.temperature, "steps": args.steps, "rounds": args.rounds, **med,
           "wor_over_with_replacement": round(med["scst_step_without_replacement"] / med["scst_step_with_replacement"], 4),
           "spread_with_replacement": [round(min(res["scst_step_with_replacement"]), 3), round(max(res["scst_step_with_replacement"]), 3)],
           "spread_without_replacement": [round(min(res["scst_step_without_replacement"]), 3),
                                          round(max(res["scst_step_without_replacement"]), 3)],
           "duplicate_share_of_independent_samples": round(float(np.mean(dups)), 4), "duplicate_share_by_temperature": dup_at,
           "distinct_share_without_replacement": round(float(np.mean(distinct)), 4),
           "largest_weight_of_a_clip_mean": round(float(wgt.max(1).values.mean()), 4),
           "mean_reward_with_replacement": round(float(lr["reward"].mean()), 5),
           "mean_reward_without_replacement": round(float(lw["reward"].mean()), 5)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
