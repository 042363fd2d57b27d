#!/usr/bin/env python3
"""Consensus selection under a weighted utility mix (cvc_consensus_mix: the pair metrics CIDEr-D, BLEU-1..4 and ROUGE-L of every
candidate against every other one as its single reference, the weighted mean, the pick and the picked row in one launch) next to

* the gathered route: every ordered pair (i, j) of a clip gathered into one candidate row with one reference row, cvc_cider_d and
  cvc_caption_overlap on those B n (n - 1) rows, then torch for the mix, the weights, the arg-max and the gather of the picked rows
  (the index tensors are built once, outside the timing), and
* cvc_consensus_cider for the case both blocks cover: CIDEr-D alone with uniform weights (which keeps routing to the old kernel),

measured in one process (GPU box) at config 3 (B = 64, T = 20) with n = 5 and n = 20 candidates per clip and the table of 2 000
synthetic captions.  The candidates are the model's own samples (seeded random checkpoint: full-length captions, the most n-grams a
row can hold), the log-weights seeded normal numbers.  The kinds are timed in alternating rounds (median of the rounds), so clock and
cache drift fall on all alike; the two routes' utilities are compared.  Prints one JSON line (times in ms).

  python tools/bench_consensus_mix.py [--steps 5] [--rounds 5] [--config cfg3] [--utility cider:1,bleu4:0.5,rougel:0.5]
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
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--utility", default="cider:1,bleu4:0.5,rougel:0.5")
    args = ap.parse_args()
    from cvc import synth, hip, metrics, opts as cvc_opts
    from cvc.cider import CiderD
    from cvc.model.captioner import DecodeAndGroundCaptionerGVDROI, PrecomputedRegionFeatures
    mix = metrics.parse_reward_weights(args.utility, "--utility")
    dev = torch.device("cuda:0")
    d = synth.CONFIGS[args.config]
    o = cvc_opts.parse_opt([])
    o.vocab_size, o.itow, o.wtoi = d.V, {str(i): "w%d" % i for i in range(d.V)}, {"UNK": synth.UNK_IDX}
    o.seq_length, o.rnn_size, o.input_encoding_size, o.att_hid_size = d.T, d.R, d.E, d.A
    o.detect_size, o.vis_encoding_size, o.train_decoder_only = d.DET, d.G, False
    sd = {k: torch.from_numpy(v) for k, v in synth.hot_path_state_dict(d, args.seed).items()}
    table = CiderD.from_captions(list(synth.captions(dataclasses.replace(d, B=2000), args.seed + 1)), dev)
    model = DecodeAndGroundCaptionerGVDROI(o, roi_extractor=PrecomputedRegionFeatures(d.DET, d.G))
    model.load_state_dict(sd, strict=False)
    model = model.to(dev).eval()
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    feats = {k: t(v) for k, v in synth.clip_features(d, args.seed).items()}
    b = {k: t(v) for k, v in synth.label_glue_batch(d, args.seed).items()}
    smp_args = (feats, b["input_seq"], b["proposals"], b["gt_seq"], b["num"], b["box_mask"], b["gt_bboxs"], torch.zeros(d.B, 1, 1, device=dev),
                b["frm_mask"], b["sample_idx"], feats["pnt_mask"])
    plain = dict(sample_max=0, temperature=1.0, beam_size=1, top_k=0, top_p=1.0)
    kinds, state, meta = {}, {}, {}
    gen = torch.Generator(device="cpu").manual_seed(args.seed)
    for n in (5, 20):
        draws = [model._sample(*smp_args, sample_n=5, consensus=False, **dict(plain, seed=1 + k))[0].view(d.B, 5, d.T) for k in range(n // 5)]
        cand = torch.cat(draws, 1).reshape(d.B * n, d.T).contiguous()
        rows = d.B * n
        logw = (torch.randn(rows, generator=gen) * 3.0 - 8.0).to(dev)
        # the gathered route's constants: for row c * n + i its clip's other rows j in ascending order -> B n (n - 1) pairs
        j = torch.arange(n, device=dev)
        others = torch.stack([torch.cat((j[:k], j[k + 1:])) for k in range(n)])                                  # [n, n - 1]
        ref_idx = (torch.arange(d.B, device=dev).view(-1, 1, 1) * n + others.view(1, n, n - 1)).reshape(-1)      # [rows (n - 1)]
        cand_idx = torch.arange(rows, device=dev).repeat_interleave(n - 1)
        ones = torch.ones(rows * (n - 1), dtype=torch.int32, device=dev)
        base = torch.arange(d.B, device=dev) * n

        def block(cand=cand, n=n, logw=logw):
            state["block", n] = metrics.consensus(cand, n, mix, table, logw)

        def gathered(cand=cand, n=n, logw=logw, ref_idx=ref_idx, cand_idx=cand_idx, ones=ones, base=base):
            c, r = cand[cand_idx], cand[ref_idx].unsqueeze(1)
            u, _ = metrics.reward_mix(mix, table, c, r, ones)                 # cvc_cider_d + cvc_caption_overlap + the mix
            lw = logw.view(-1, n)
            w = torch.exp(lw - lw.max(1, keepdim=True)[0]).reshape(-1)[ref_idx].view(-1, n - 1)
            util = (w * u.view(-1, n - 1)).sum(1) / w.sum(1)
            pick = util.view(-1, n).argmax(1)
            state["gathered", n] = (util, pick, cand[base + pick])

        def block_cider_uniform(cand=cand, n=n):
            state["block_cider", n] = metrics.consensus(cand, n, {"cider": 1.0}, table)

        def old_cider_uniform(cand=cand, n=n):
            state["old_cider", n] = table.consensus(cand, n)
        kinds.update({f"block_n{n}": (block, 20), f"gathered_n{n}": (gathered, 20),
                      f"block_cider_uniform_n{n}": (block_cider_uniform, 20), f"consensus_cider_n{n}": (old_cider_uniform, 20)})
        meta[n] = dict(rows=rows, mean_len=float((cand != 0).to(torch.float32).cumprod(1).sum(1).mean()))
    for fn, _ in kinds.values():              # warm-up: allocator, code objects
        for _ in range(2):
            fn()
    res = {k: [] for k in kinds}
    for _ in range(args.rounds):
        for k, (fn, mult) in kinds.items():
            res[k].append(ms(fn, mult * args.steps))
    med = {k: round(float(np.median(v)), 4) for k, v in res.items()}
    out = {"metric": "consensus selection under a utility mix with weighted candidates: cvc_consensus_mix vs gathered single references on "
                     "cvc_cider_d + cvc_caption_overlap + torch (weights, arg-max, gather); and vs cvc_consensus_cider for CIDEr-D alone "
                     "with uniform weights, ms (median of alternating rounds)", "unit": "ms",
           "lib": hip.version(), "config": args.config, "B": d.B, "T": d.T, "V": d.V, "table_keys": len(table), "table_captions": table.n_doc,
           "utility": mix, "steps": args.steps, "rounds": args.rounds, **med,
           **{f"gathered_over_block_n{n}": round(med[f"gathered_n{n}"] / max(med[f"block_n{n}"], 1e-9), 2) for n in (5, 20)},
           **{f"block_over_consensus_cider_n{n}": round(med[f"block_cider_uniform_n{n}"] / max(med[f"consensus_cider_n{n}"], 1e-9), 2)
              for n in (5, 20)},
           **{f"max_abs_diff_vs_gathered_n{n}": float((state["block", n]["utility"] - state["gathered", n][0]).abs().max()) for n in (5, 20)},
           **{f"max_abs_diff_vs_consensus_cider_n{n}": float((state["block_cider", n]["utility"] - state["old_cider", n][0]).abs().max())
              for n in (5, 20)},
           **{f"nonzero_utilities_n{n}": int((state["block", n]["utility"] != 0).sum()) for n in (5, 20)},
           **{f"mean_caption_len_n{n}": round(meta[n]["mean_len"], 2) for n in (5, 20)}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
