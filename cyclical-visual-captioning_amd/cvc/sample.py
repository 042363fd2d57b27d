#!/usr/bin/env python3
"""Sampled captions of the validation split from a checkpoint: n captions per segment, every word drawn from softmax(logits /
temperature) without UNK, written to <results_dir>/densecap-<val_split>-<id>_samples.json (Trainer.sample).

  python -m cvc.sample --temperature 0.7 --sample_n 5 --sample_seed 1 --path_opt cfgs/cyclical.yml --resume True --id my_run
  python -m cvc.sample --temperature 1.0 --top_k 40 --top_p 0.9 ...      (top-k, then nucleus truncation of the distribution)

  python -m cvc.sample --sample_n 16 --consensus ...                     (also the consensus pick and the samples' utilities)
  python -m cvc.sample --sample_n 5 --without_replacement ...            (5 DISTINCT captions per segment in draw order, by
                                                                          stochastic beam search, with each one's logq and G)
  python -m cvc.sample --sample_n 5 --diversity ...                      (also every segment's Div-1, Div-2, mBLEU-4 and distinct
                                                                          captions, and the split's summary with the oracle CIDEr-D)
  python -m cvc.sample --sample_n 5 --diversity --self_cider ...         (also every segment's Self-CIDEr and LSA diversity, and
                                                                          their means in the summary)

--temperature / --sample_n / --sample_seed / --top_k / --top_p / --consensus / --without_replacement / --diversity / --self_cider are this module's own; every other flag is cvc.main's (options, YAML overlay, dataset,
--resume with --load_best_score: the same checkpoint loading as an --inference_only evaluation).
"""
from __future__ import annotations

import argparse
import sys

from . import main as cvc_main


def parse(argv=None):
    """-> (this module's own flags, the rest for cvc.main)"""
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter, add_help=False)
    p.add_argument("--temperature", type=float, default=1.0, help="sampling temperature tau > 0 (not --softmax_temp, the attention's)")
    p.add_argument("--sample_n", type=int, default=5, help="captions per segment")
    p.add_argument("--sample_seed", type=int, default=0, help="seed of the sampling noise")
    p.add_argument("--top_k", type=int, default=0, help="keep the k most likely words (and ties with the k-th); 0 = off")
    p.add_argument("--top_p", type=float, default=1.0, help="nucleus: keep the most likely words up to mass p in (0, 1]; 1 = off")
    p.add_argument("--consensus", action="store_true",
                   help="add to every segment the index of its consensus pick and the samples' utilities (CIDEr-D against the other "
                        "samples, training captions' table); needs --sample_n > 1")
    p.add_argument("--without_replacement", action="store_true",
                   help="draw the --sample_n captions of a segment without replacement (stochastic beam search at --temperature): "
                        "pairwise distinct, in draw order, with each one's logq and G; needs --sample_n > 1, refused with --top_k / --top_p")
    p.add_argument("--diversity", action="store_true",
                   help="add to every segment the diversity of its --sample_n captions (Div-1, Div-2, mBLEU-4, distinct captions; "
                        "cvc.metrics.set_diversity) and to the file the split's summary with the oracle and mean CIDEr-D; needs "
                        "--sample_n > 1")
    p.add_argument("--self_cider", action="store_true",
                   help="with --diversity: add to every segment's diversity the Self-CIDEr and LSA diversity of its captions "
                        "(cvc.metrics.set_spectrum) and to the summary their means over the split")
    own, rest = p.parse_known_args(argv)
    if own.self_cider and not own.diversity:
        raise SystemExit("--self_cider needs --diversity (it adds to the diversity of every segment's captions)")
    if own.diversity and own.sample_n < 2:
        raise SystemExit("--diversity needs --sample_n > 1 (the diversity of a set of one caption says nothing)")
    if own.without_replacement and own.sample_n < 2:
        raise SystemExit("--without_replacement needs --sample_n > 1")
    if own.without_replacement and (own.top_k != 0 or own.top_p != 1.0):
        raise SystemExit("--without_replacement is refused with --top_k / --top_p")
    if own.consensus and own.sample_n < 2:
        raise SystemExit("--consensus needs --sample_n > 1")
    if not own.temperature > 0:
        raise SystemExit("--temperature must be > 0")
    if own.sample_n < 1:
        raise SystemExit("--sample_n must be >= 1")
    if own.top_k < 0:
        raise SystemExit("--top_k must be >= 0")
    if not 0 < own.top_p <= 1:
        raise SystemExit("--top_p must lie in (0, 1]")
    return own, rest


def main(argv=None):
    own, rest = parse(argv)
    if "--inference_only" not in rest:
        rest = rest + ["--inference_only"]
    return cvc_main.main(rest, sample=(own.sample_n, own.temperature, own.sample_seed, own.top_k, own.top_p, own.consensus, own.without_replacement, own.diversity) + ((True,) if own.self_cider else ()))


if __name__ == "__main__":
    sys.exit(main())
