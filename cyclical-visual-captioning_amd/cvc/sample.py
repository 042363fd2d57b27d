#!/usr/bin/env python3
"""Sampled captions of the validation split from a checkpoint: n captions per segment, every word drawn from softmax(logits /
temperature) without UNK, written to <results_dir>/densecap-<val_split>-<id>_samples.json (Trainer.sample).

  python -m cvc.sample --temperature 0.7 --sample_n 5 --sample_seed 1 --path_opt cfgs/cyclical.yml --resume True --id my_run

--temperature / --sample_n / --sample_seed are this module's own; every other flag is cvc.main's (options, YAML overlay, dataset,
--resume with --load_best_score: the same checkpoint loading as an --inference_only evaluation).
"""
from __future__ import annotations

import argparse
import sys

from . import main as cvc_main


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter, add_help=False)
    p.add_argument("--temperature", type=float, default=1.0, help="sampling temperature tau > 0 (not --softmax_temp, the attention's)")
    p.add_argument("--sample_n", type=int, default=5, help="captions per segment")
    p.add_argument("--sample_seed", type=int, default=0, help="seed of the sampling noise")
    own, rest = p.parse_known_args(argv)
    if not own.temperature > 0:
        raise SystemExit("--temperature must be > 0")
    if own.sample_n < 1:
        raise SystemExit("--sample_n must be >= 1")
    if "--inference_only" not in rest:
        rest = rest + ["--inference_only"]
    return cvc_main.main(rest, sample=(own.sample_n, own.temperature, own.sample_seed))


if __name__ == "__main__":
    sys.exit(main())
