#!/usr/bin/env python3
"""Consensus caption selection (cvc_consensus_cider: pairwise CIDEr-D among a clip's candidates, pick and picked row in one launch)
next to the route without the block -- the clip's other candidates gathered into a reference tensor, cvc_cider_d with one row per
clip, an arg-max and a gather of the picked rows -- and a consensus decode next to the plain sampling decode (n = 5, the
self-critical step's rollout shape, unless --decode_n says otherwise), measured in one process (GPU box) at config 3 (B = 64, T = 20) with n = 5 and n = 20 candidates per clip and the table of 2 000 synthetic captions.
The candidates are the model's own samples (seeded random checkpoint: full-length captions, the most n-grams a row can hold).  The
kinds are timed in alternating rounds (median of the rounds), so clock and cache drift fall on all alike; the utilities of the two
routes are compared bit for bit.  Prints one JSON line (times in ms).

  python tools/bench_consensus.py [--steps 5] [--rounds 5] [--config cfg3] [--decode_n 5]
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
    ap.add_argument("--decode_n", default="5", help="the candidate counts (of 5, 20) at which the two decodes are timed too ('' = none)")
    args = ap.parse_args()
    from cvc import synth, hip, opts as cvc_opts
    from cvc.cider import CiderD
    from cvc.model.captioner import DecodeAndGroundCaptionerGVDROI, PrecomputedRegionFeatures
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
    model.consensus_table = table
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    feats = {k: t(v) for k, v in synth.clip_features(d, args.seed).items()}
    b = {k: t(v) for k, v in synth.label_glue_batch(d, args.seed).items()}
    smp_args = (feats, b["input_seq"], b["proposals"], b["gt_seq"], b["num"], b["box_mask"], b["gt_bboxs"], torch.zeros(d.B, 1, 1, device=dev),
                b["frm_mask"], b["sample_idx"], feats["pnt_mask"])
    plain = dict(sample_max=0, temperature=1.0, seed=1, beam_size=1, top_k=0, top_p=1.0)
    kinds, state, meta = {}, {}, {}
    decode_n = [int(x) for x in args.decode_n.split(",") if x]
    for n in (5, 20):
        # n candidates per clip from n / 5 seeded decodes of 5 samples each (clip-major rows, as one decode of n would lay them out)
        draws = [model._sample(*smp_args, sample_n=5, consensus=False, **dict(plain, seed=1 + k))[0].view(d.B, 5, d.T) for k in range(n // 5)]
        cand = torch.cat(draws, 1).reshape(d.B * n, d.T).contiguous()
        rows = d.B * n
        # the gathered route's constants: for row c * n + j the clip's other rows in ascending order, and their number
        j = torch.arange(n, device=dev)
        others = torch.stack([torch.cat((j[:k], j[k + 1:])) for k in range(n)])                                  # [n, n - 1]
        idx = (torch.arange(d.B, device=dev).view(-1, 1, 1) * n + others.view(1, n, n - 1)).reshape(rows, n - 1)
        nref = torch.full((rows,), n - 1, dtype=torch.int32, device=dev)
        base = torch.arange(d.B, device=dev) * n

        def block(cand=cand, n=n):
            state["block", n] = table.consensus(cand, n)

        def gathered(cand=cand, n=n, idx=idx, nref=nref, base=base):
            u = table.score(cand, cand[idx], nref)
            pick = u.view(-1, n).argmax(1)
            state["gathered", n] = (u, pick, cand[base + pick])

        def decode_plain(n=n):
            model._sample(*smp_args, sample_n=n, consensus=False, **plain)

        def decode_consensus(n=n):
            model._sample(*smp_args, sample_n=n, consensus=True, **plain)
        kinds.update({f"block_n{n}": (block, 20), f"gathered_cider_d_n{n}": (gathered, 20)})
        if n in decode_n:
            kinds.update({f"decode_sampling_n{n}": (decode_plain, 1), f"decode_consensus_n{n}": (decode_consensus, 1)})
        meta[n] = dict(rows=rows, mean_len=float((cand != 0).to(torch.float32).cumprod(1).sum(1).mean()))
    for fn, _ in kinds.values():              # warm-up: allocator, code objects, the engines of both decodes
        for _ in range(2):
            fn()
    res = {k: [] for k in kinds}
    for _ in range(args.rounds):
        for k, (fn, mult) in kinds.items():
            res[k].append(ms(fn, mult * args.steps))
    med = {k: round(float(np.median(v)), 4) for k, v in res.items()}
    same = {n: bool(torch.equal(state["block", n][0], state["gathered", n][0])) for n in (5, 20)}
    # (picks: torch's arg-max does not promise the lowest index on a tie, the block does -- compared through the picked utilities)
    top = {n: bool(torch.equal(state["block", n][0].view(-1, n).gather(1, state["block", n][1].long().view(-1, 1)),
                               state["gathered", n][0].view(-1, n).gather(1, state["gathered", n][1].view(-1, 1)))) for n in (5, 20)}
    out = {"metric": "consensus selection: the pairwise block vs gathered references on cvc_cider_d (gather and arg-max included); a "
                     "consensus decode vs the plain sampling decode, ms (median of alternating rounds)", "unit": "ms",
           "lib": hip.version(), "config": args.config, "B": d.B, "T": d.T, "V": d.V, "table_keys": len(table), "table_captions": table.n_doc,
           "steps": args.steps, "rounds": args.rounds, **med,
           **{f"gathered_over_block_n{n}": round(med[f"gathered_cider_d_n{n}"] / max(med[f"block_n{n}"], 1e-9), 2) for n in (5, 20)},
           **{f"consensus_decode_extra_ms_n{n}": round(med[f"decode_consensus_n{n}"] - med[f"decode_sampling_n{n}"], 4) for n in (5, 20) if n in decode_n},
           **{f"utilities_bit_equal_n{n}": same[n] for n in (5, 20)}, **{f"picked_utilities_equal_n{n}": top[n] for n in (5, 20)},
           **{f"nonzero_utilities_n{n}": int((state["block", n][0] != 0).sum()) for n in (5, 20)},
           **{f"mean_caption_len_n{n}": round(meta[n]["mean_len"], 2) for n in (5, 20)}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
