#!/usr/bin/env python3
"""Spectral caption-set diversity (cvc_caption_set_spectrum: the similarity matrix of every clip's candidate set, its eigenvalues and
the Self-CIDEr / LSA scores in one launch) next to a torch route, measured in one process (GPU box) at config-3 sizes: 64 clips,
T = 20, n = 5 and n = 20 candidates per clip.

The candidates are synthetic: per clip a base caption and rows that replace about a third of its words (near-duplicates, as a
sampler's sets are), all live.  The table is that of 2 000 synthetic captions.

Kinds: cvc.metrics.set_spectrum in mode cider and in mode lsa (the launch and its three output allocations), and the torch route of
mode cider: the n-gram keys of every position, counts and first occurrences by comparing positions, the idf by torch.searchsorted,
the pairwise dot products of a clip by comparing all positions of all its rows, K = 1/4 sum_n cosines, batched torch.linalg.eigvalsh
in fp64 and the two scores.  That route is also the cross-check (K to 1e-5, the eigenvalues to 1e-5, the scores to 1e-5).  The kinds
are timed in alternating rounds (median of the rounds).  Prints one JSON line (times in ms) and, with --out, writes it to a file.

  python tools/bench_spectrum.py [--steps 5] [--rounds 5] [--out profiles/bench_spectrum_cfg3.json]
"""
import argparse
import dataclasses
import json
import math
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


def candidates(base, n, seed):
    """base [clips, T] (0-terminated) -> [clips * n, T]: row 0 of a clip is its base, the others replace about a third of its words
    by words of the same caption or of the next clip's"""
    rng = np.random.default_rng(seed)
    clips, T = base.shape
    out = np.repeat(base[:, None, :], n, 1)
    other = np.roll(base, 1, 0)
    for c in range(clips):
        L = int((np.cumprod(base[c] != 0)).sum())
        pool = np.concatenate([base[c][:L], other[c][other[c] != 0]])
        for j in range(1, n):
            hit = rng.random(L) < 1 / 3
            out[c, j, :L][hit] = rng.choice(pool, int(hit.sum()))
    return out.reshape(clips * n, T)


def torch_spectrum(cand, n_per, keys, idf, idf_unseen):
    """mode cider by torch ops -> (K [clips, n, n] fp32, lam [clips, n] fp64 descending, score [clips, 2] fp64)"""
    rows, T = cand.shape
    clips = rows // n_per
    alive = (cand != 0).to(torch.int64).cumprod(1)
    w = (cand + 1) * alive                                                  # 0 from the end mark on
    wp = torch.cat([w, w.new_zeros(rows, 3)], 1)
    key = torch.zeros_like(w)
    ok = torch.ones_like(w, dtype=torch.bool)
    earlier = torch.ones(T, T, dtype=torch.bool, device=cand.device).tril(-1)            # [p, q]: q < p
    K = torch.zeros(clips, n_per, n_per, device=cand.device)
    for n in range(1, 5):
        nxt = wp[:, n - 1:n - 1 + T]
        key = key | (nxt << (48 - 16 * (n - 1)))
        ok = ok & (nxt != 0)
        k = torch.where(ok, key, torch.zeros_like(key))
        eq = (k.unsqueeze(2) == k.unsqueeze(1)) & ok.unsqueeze(2)          # [rows, p, q]
        count = eq.sum(2)
        first = ~(eq & earlier).any(2) & ok
        at = torch.searchsorted(keys, k).clamp(max=keys.numel() - 1)
        wgt = torch.where(keys[at] == k, idf[at], torch.full((), idf_unseen, device=cand.device))
        v = torch.where(first, count.to(torch.float32) * wgt, torch.zeros((), device=cand.device))
        norm = v.pow(2).sum(1).sqrt().view(clips, n_per)
        kc, vc = k.view(clips, n_per * T), v.view(clips, n_per * T)
        match = (kc.unsqueeze(2) == kc.unsqueeze(1)) & (kc.unsqueeze(2) != 0)
        dot = (match * vc.unsqueeze(2) * vc.unsqueeze(1)).view(clips, n_per, T, n_per, T).sum((2, 4))
        den = norm.unsqueeze(2) * norm.unsqueeze(1)
        K += 0.25 * torch.where(den > 0, dot / den.clamp(min=1e-30), torch.zeros_like(dot))
    K = 0.5 * (K + K.transpose(1, 2))
    lam = torch.linalg.eigvalsh(K.to(torch.float64)).flip(1)
    tr = K.to(torch.float64).diagonal(dim1=1, dim2=2).sum(1)
    logm = math.log(n_per)
    s0 = -torch.log((lam[:, 0] / tr).clamp(max=1.0)) / logm
    s1 = -torch.log(lam[:, 0].sqrt() / lam.clamp(min=0).sqrt().sum(1)) / logm
    return K, lam, torch.stack([s0, s1], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from cvc import synth, hip, metrics
    from cvc.cider import CiderD
    dev = torch.device("cuda:0")
    d = synth.CONFIGS[args.config]
    assert d.V < 32768, "the torch route searches the table's keys as signed values"
    table = CiderD.from_captions(list(synth.captions(dataclasses.replace(d, B=2000), args.seed + 1)), dev)
    base = np.stack([np.asarray(c, np.int64)[:d.T] for c in synth.captions(dataclasses.replace(d, B=64), args.seed)])
    base[:, -1] = 0
    kinds, state, meta = {}, {}, {}
    for n in (5, 20):
        cand = torch.from_numpy(candidates(base, n, args.seed + n)).to(dev)

        def block_cider(cand=cand, n=n):
            state["cider", n] = metrics.set_spectrum(cand, n, cider=table, want_gram=True)

        def block_cider_no_gram(cand=cand, n=n):
            metrics.set_spectrum(cand, n, cider=table)

        def block_lsa(cand=cand, n=n):
            state["lsa", n] = metrics.set_spectrum(cand, n)

        def torch_route(cand=cand, n=n):
            state["torch", n] = torch_spectrum(cand, n, table.keys, table.idf, table.idf_unseen)
        kinds.update({f"block_cider_n{n}": (block_cider, 20), f"block_cider_no_gram_n{n}": (block_cider_no_gram, 20),
                      f"block_lsa_n{n}": (block_lsa, 20), f"torch_cider_n{n}": (torch_route, 4)})
        meta[n] = dict(mean_len=float((cand != 0).to(torch.float32).cumprod(1).sum(1).mean()))
    for fn, _ in kinds.values():                  # warm-up: allocator, code objects
        for _ in range(3):
            fn()
    res = {key: [] for key in kinds}
    for _ in range(args.rounds):
        for key, (fn, mult) in kinds.items():
            res[key].append(ms(fn, mult * args.steps))
    med = {key: round(float(np.median(v)), 4) for key, v in res.items()}
    spread = {key: round(float(max(v) - min(v)), 4) for key, v in res.items()}
    check = {}
    for n in (5, 20):
        K, lam, score = state["torch", n]
        blk = state["cider", n]
        check[f"max_abs_K_diff_n{n}"] = float((blk["gram"][:, :n, :n] - K).abs().max())
        check[f"max_abs_lam_diff_n{n}"] = float((blk["lam"][:, :n] - lam).abs().max())
        check[f"max_abs_score_diff_n{n}"] = float((blk["score"].to(torch.float64) - score).abs().max())
        check[f"sweeps_max_n{n}"] = int(blk["info"][:, 1].max())
        check[f"Self_CIDEr_n{n}"] = round(float(blk["score"][:, 0].mean()), 4)
        check[f"LSA_n{n}"] = round(float(state["lsa", n]["score"][:, 1].mean()), 4)
        assert check[f"max_abs_K_diff_n{n}"] <= 1e-5 and check[f"max_abs_lam_diff_n{n}"] <= 1e-5 and check[f"max_abs_score_diff_n{n}"] <= 1e-5, check
    out = {"metric": "spectral caption-set diversity: cvc_caption_set_spectrum (modes cider and lsa) vs a torch route (n-gram keys, "
                     "pairwise matches, batched fp64 eigvalsh), ms (median of alternating rounds)", "unit": "ms",
           "lib": hip.version(), "config": args.config, "clips": 64, "T": d.T, "V": d.V, "table_captions": table.n_doc,
           "steps": args.steps, "rounds": args.rounds, **med, **{f"spread_{key}": v for key, v in spread.items()},
           **{f"torch_over_block_n{n}": round(med[f"torch_cider_n{n}"] / max(med[f"block_cider_n{n}"], 1e-9), 2) for n in (5, 20)},
           **check, **{f"mean_caption_len_n{n}": round(meta[n]["mean_len"], 2) for n in (5, 20)}}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
