#!/usr/bin/env python3
"""The token-overlap metrics kernel (cvc_caption_overlap: BLEU statistics, sentence BLEU-1..4, ROUGE-L) next to its fp64 Python
restatement on the host (tests/overlap_ref.py, the device-to-host copy of the captions included), and the self-critical step with a
three-way reward mix next to the CIDEr-D-only step, measured in one process (GPU box) at config 3 (B = 64, T = 20, V = 5000):
the kernel at the self-critical shape (B x S sampled rows) and at a validation-sized batch (the B greedy captions).  The kinds are timed
in alternating rounds (median of the rounds), so clock and cache drift fall on all alike.  The checkpoint is the seeded random one of the
benchmarks: its captions share few n-grams with the references; the kernel's work (keys, counts, one ballot per candidate word and
reference) does not depend on how many match.  Prints one JSON line (times in ms).

  python tools/bench_metrics.py [--steps 5] [--rounds 5] [--samples 5] [--config cfg3]
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

MIX = {"cider": 1.0, "bleu4": 0.5, "rougel": 0.5}


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
    from cvc import synth, hip, metrics, opts as cvc_opts
    from cvc.cider import CiderD
    from cvc.model.captioner import DecodeAndGroundCaptionerGVDROI, PrecomputedRegionFeatures
    from cvc.trainer import Trainer, build_optimizer
    import overlap_ref as R
    dev = torch.device("cuda:0")
    d, S = synth.CONFIGS[args.config], args.samples
    o = cvc_opts.parse_opt([])
    o.vocab_size, o.itow, o.wtoi = d.V, {str(i): "w%d" % i for i in range(d.V)}, {"UNK": synth.UNK_IDX}
    o.seq_length, o.rnn_size, o.input_encoding_size, o.att_hid_size = d.T, d.R, d.E, d.A
    o.detect_size, o.vis_encoding_size, o.train_decoder_only = d.DET, d.G, False
    o.xe_loss_weight, o.caption_consistency_loss_weight, o.learning_rate, o.batch_size = 0.5, 0.5, 1e-4, d.B
    o.scst_samples, o.scst_temperature, o.scst_seed, o.scst_dropout = S, 1.0, 1, False
    sd = {k: torch.from_numpy(v) for k, v in synth.hot_path_state_dict(d, args.seed).items()}
    corpus = list(synth.captions(d, args.seed)) + list(synth.captions(dataclasses.replace(d, B=4000), args.seed + 1))
    table = CiderD.from_captions(corpus, dev)

    def fresh(weights):
        m = DecodeAndGroundCaptionerGVDROI(o, roi_extractor=PrecomputedRegionFeatures(d.DET, d.G))
        m.load_state_dict(sd, strict=False)
        m = m.to(dev).train()
        tr = Trainer(o, None, m, build_optimizer(m, o), None, None)
        tr._cider, tr.scst_reward_weights = table, weights
        return m, tr
    model, tr_cider = fresh(None)
    _model_mix, tr_mix = fresh(dict(MIX))
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    feats = {k: t(v) for k, v in synth.clip_features(d, args.seed).items()}
    b = {k: t(v) for k, v in synth.label_glue_batch(d, args.seed).items()}
    batch = (feats, b["input_seq"], b["gt_seq"], b["num"].cpu(), b["proposals"], b["gt_bboxs"], b["box_mask"],
             ["v_x_segment_%02d" % i for i in range(d.B)], torch.zeros(d.B, d.N, 1), b["frm_mask"], b["sample_idx"], feats["pnt_mask"][:, 1:])
    prepared = tr_cider._prepare(batch, True)
    refs, nref = prepared["gt_seqs"][:, :, :d.T].contiguous(), prepared["num"][:, 0].to(torch.int32)
    refs_h, nref_h = refs.cpu().numpy(), nref.cpu().numpy()
    smp_args = [prepared[k] for k in ("segs_feat", "input_seqs", "ppls", "gt_seqs", "num", "mask_bboxs", "gt_bboxs", "ppls_feat", "mask_frms",
                                      "sample_idx", "pnt_mask")]
    model.eval()
    with torch.no_grad():
        sampled = model._sample(*smp_args, sample_max=0, temperature=1.0, sample_n=S, seed=1, beam_size=1, top_k=0, top_p=1.0)[0].contiguous()
        greedy = model._sample(*smp_args, sample_max=1, beam_size=1)[0].contiguous()
    model.train()
    state = {}
    kinds = {
        "overlap_scst_rows": lambda: state.__setitem__("scst", metrics.overlap(sampled, refs, nref)),
        "overlap_val_rows": lambda: state.__setitem__("val", metrics.overlap(greedy, refs, nref)),
        "cider_scst_rows": lambda: table.score(sampled, refs, nref),
        "scst_step_cider": lambda: tr_cider.scst_step(batch),
        "scst_step_mix": lambda: tr_mix.scst_step(batch),
    }
    hosts = {
        "host_fp64_scst_rows": lambda: state.__setitem__("scst_h", R.score_batch(sampled.cpu().numpy(), refs_h, nref_h)),
        "host_fp64_val_rows": lambda: state.__setitem__("val_h", R.score_batch(greedy.cpu().numpy(), refs_h, nref_h)),
    }
    for fn in kinds.values():                 # warm-up: allocator, lazy workspaces, Adam state
        for _ in range(2):
            fn()
    res = {k: [] for k in list(kinds) + list(hosts)}
    for _ in range(args.rounds):
        for k, fn in kinds.items():
            res[k].append(ms(fn, args.steps if k.startswith("scst_step") else 20 * args.steps))
        for k, fn in hosts.items():
            res[k].append(ms(fn, 1))
    med = {k: round(float(np.median(v)), 4) for k, v in res.items()}
    exact = all(np.array_equal(state[k]["stats"].cpu().numpy(), state[k + "_h"]["stats"]) for k in ("scst", "val"))
    err = max(float(np.abs(state[k][m].cpu().double().numpy() - state[k + "_h"][m]).max()) for k in ("scst", "val") for m in ("bleu", "rouge"))
    out = {"metric": "token-overlap metrics kernel vs its fp64 host restatement; self-critical step with a reward mix vs CIDEr-D only, ms "
                     "(median of alternating rounds)", "unit": "ms", "lib": hip.version(), "config": args.config, "B": d.B, "T": d.T, "V": d.V,
           "samples_per_clip": S, "scst_rows": d.B * S, "val_rows": d.B, "Rmax": int(refs.shape[1]), "steps": args.steps, "rounds": args.rounds,
           "mix": MIX, **med,
           "overlap_speedup_vs_host_scst_rows": round(med["host_fp64_scst_rows"] / max(med["overlap_scst_rows"], 1e-9), 1),
           "overlap_speedup_vs_host_val_rows": round(med["host_fp64_val_rows"] / max(med["overlap_val_rows"], 1e-9), 1),
           "mix_over_cider_step": round(med["scst_step_mix"] / med["scst_step_cider"], 4),
           "stats_equal_host": bool(exact), "score_max_abs_err_vs_fp64": err,
           "mean_rouge_scst_rows": round(float(state["scst"]["rouge"].mean()), 5)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
