#!/usr/bin/env python3
"""The self-critical training step next to the cross-entropy step, measured in one process (GPU box) at config 3 (B = 64, T = 20,
V = 5000), S samples per clip: the cross-entropy step (eager, and replayed from its HIP graph as bench.py --mode train runs it), the
self-critical step as a whole and split into rollout / reward + weights / gradient pass (forward, backward, clip, Adam), and the
fp64 Python restatement of the reward (tests/cider_ref.py) on the host for the same samples, the device-to-host copy of the samples
included.  The kinds of step are timed in alternating rounds (median of the rounds), so clock and cache drift fall on all alike.
The checkpoint is the seeded random one of the benchmarks: its samples are near-uniform over the vocabulary, so rewards are small;
the reward kernel's work (keys, counts, one table search per distinct n-gram) does not depend on how many n-grams match.
Prints one JSON line (times in ms).

  python tools/bench_scst.py [--steps 5] [--rounds 5] [--samples 5] [--config cfg3]
"""
import argparse
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def ms(fn, steps):
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
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--seed", type=int, default=1234)
    args = ap.parse_args()
    from cvc import synth, hip, opts as cvc_opts
    from cvc.cider import CiderD
    from cvc.model.captioner import DecodeAndGroundCaptionerGVDROI, PrecomputedRegionFeatures
    from cvc.trainer import Trainer, build_optimizer
    import cider_ref as R
    dev = torch.device("cuda:0")
    d, S = synth.CONFIGS[args.config], args.samples
    o = cvc_opts.parse_opt([])
    o.vocab_size, o.itow, o.wtoi = d.V, {str(i): "w%d" % i for i in range(d.V)}, {"UNK": synth.UNK_IDX}
    o.seq_length, o.rnn_size, o.input_encoding_size, o.att_hid_size = d.T, d.R, d.E, d.A
    o.detect_size, o.vis_encoding_size, o.train_decoder_only = d.DET, d.G, False
    o.xe_loss_weight, o.caption_consistency_loss_weight, o.learning_rate, o.batch_size = 0.5, 0.5, 1e-4, d.B
    o.scst_samples, o.scst_temperature, o.scst_seed, o.scst_dropout = S, 1.0, 1, False
    sd = {k: torch.from_numpy(v) for k, v in synth.hot_path_state_dict(d, args.seed).items()}

    def fresh():
        m = DecodeAndGroundCaptionerGVDROI(o, roi_extractor=PrecomputedRegionFeatures(d.DET, d.G))
        m.load_state_dict(sd, strict=False)
        m = m.to(dev).train()
        return m, Trainer(o, None, m, build_optimizer(m, o, capturable=True), None, None)
    # the captured cross-entropy step gets a model and a trainer of its own, warmed up and captured before anything else runs: its
    # warm-up and capture run on a side stream, and a parameter whose gradient accumulator was made by an eager step on the default
    # stream cannot be captured there
    _model_g, tr_g = fresh()
    model, tr = fresh()
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    feats = {k: t(v) for k, v in synth.clip_features(d, args.seed).items()}
    b = {k: t(v) for k, v in synth.label_glue_batch(d, args.seed).items()}
    batch = (feats, b["input_seq"], b["gt_seq"], b["num"].cpu(), b["proposals"], b["gt_bboxs"], b["box_mask"],
             ["v_x_segment_%02d" % i for i in range(d.B)], torch.zeros(d.B, d.N, 1), b["frm_mask"], b["sample_idx"], feats["pnt_mask"][:, 1:])
    corpus = list(synth.captions(d, args.seed)) + list(synth.captions(dataclasses.replace(d, B=4000), args.seed + 1))
    tr._cider = CiderD.from_captions(corpus, dev)
    df, n_doc = R.doc_freq(corpus)
    prepared = tr._prepare(batch, True)
    refs, nref = prepared["gt_seqs"][:, :, :d.T].contiguous(), prepared["num"][:, 0].to(torch.int32)
    refs_h, nref_h = refs.cpu().numpy(), nref.cpu().numpy()
    enc_args = [prepared[k] for k in ("segs_feat", "ppls", "num", "mask_bboxs", "ppls_feat", "gt_bboxs", "mask_frms", "sample_idx", "pnt_mask")]
    smp_args = [prepared[k] for k in ("segs_feat", "input_seqs", "ppls", "gt_seqs", "num", "mask_bboxs", "gt_bboxs", "ppls_feat", "mask_frms",
                                      "sample_idx", "pnt_mask")]
    for _ in range(2):
        tr_g.train_step_graphed(batch)
    torch.cuda.synchronize()
    state = {}

    def rollout():
        model.eval()
        model.invalidate_decode_cache()          # as after every optimizer step: the rollout binds the new weights
        with torch.no_grad():
            state["enc"] = model.encode_clips(*enc_args)
            state["seq"] = model._sample(*smp_args, sample_max=0, temperature=1.0, sample_n=S, seed=1, beam_size=1, top_k=0, top_p=1.0,
                                         encoded=state["enc"])[0].contiguous()

    def reward():
        state["reward"] = tr.cider().score(state["seq"], refs, nref)
        state["w"] = hip.scst_weights(state["reward"], None, S, state["seq"], t_major=True)

    def gradient():
        loss, _adv = model.scst_loss(state["enc"], state["seq"], state["reward"], None, S)
        model.train()
        tr._backward_and_update(loss)
        tr._weights_changed()

    def host_reward():
        state["host"] = R.score_batch(state["seq"].cpu().numpy(), refs_h, nref_h, df, n_doc)[0]

    kinds = {"xe_eager": lambda: tr.train_step(batch), "xe_graphed": lambda: tr_g.train_step_graphed(batch),
             "scst_step": lambda: tr.scst_step(batch), "scst_rollout": rollout, "scst_reward_weights": reward, "scst_gradient_pass": gradient}
    for fn in kinds.values():                 # warm-up: allocator, lazy workspaces, Adam state, the graph's capture
        for _ in range(2):
            fn()
    res = {k: [] for k in kinds}
    res["host_reward_fp64"] = []
    for _ in range(args.rounds):
        for k, fn in kinds.items():
            res[k].append(ms(fn, args.steps if k != "scst_reward_weights" else 20 * args.steps))
        res["host_reward_fp64"].append(ms(host_reward, 1))
    med = {k: round(float(np.median(v)), 3) for k, v in res.items()}
    err = float(np.abs(state["reward"].cpu().double().numpy() - state["host"]).max())
    out = {"metric": "self-critical step vs cross-entropy step, ms per step (median of alternating rounds)", "unit": "ms", "lib": hip.version(),
           "config": args.config, "B": d.B, "T": d.T, "V": d.V, "samples_per_clip": S, "rows": d.B * S, "steps": args.steps, "rounds": args.rounds,
           "table_ngrams": len(tr.cider()), **med,
           "reward_speedup_vs_host": round(med["host_reward_fp64"] / max(med["scst_reward_weights"], 1e-9), 1),
           "scst_over_xe_graphed": round(med["scst_step"] / med["xe_graphed"], 3),
           "mean_reward": round(float(state["reward"].mean()), 5), "reward_max_abs_err_vs_fp64": err}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
