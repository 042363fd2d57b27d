#!/usr/bin/env python3
"""Teacher-forced scores of the validation split's ground-truth captions from a checkpoint: per segment the caption's log-prob, its
number of scored words and how many of them are the model's arg-max, written to <results_dir>/densecap-<val_split>-<id>_scores.json
(Trainer.score); perplexity and top-1 accuracy are printed.  With --ground_gt also the grounding on the GT sentences
(Trainer.ground_gt): attn-gt-sent-results-<val_split>-<id>.json, grd-gt-sent-results-<val_split>-<id>.json and the box accuracies.

  python -m cvc.score --path_opt cfgs/cyclical.yml --resume True --id my_run
  python -m cvc.score --ground_gt --resume True --id my_run ...

--ground_gt is this module's own; every other flag is cvc.main's (options, YAML overlay, dataset, --resume with
--load_best_score: the same checkpoint loading as an --inference_only evaluation).
"""
from __future__ import annotations

import argparse
import sys

from . import main as cvc_main


def parse(argv=None):
    """-> (this module's own flags, the rest for cvc.main)"""
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter, add_help=False)
    p.add_argument("--ground_gt", action="store_true", help="also ground the GT sentences (box accuracy of attention and grounder)")
    return p.parse_known_args(argv)


def main(argv=None):
    own, rest = parse(argv)
    if "--inference_only" not in rest:
        rest = rest + ["--inference_only"]
    return cvc_main.main(rest, score=dict(ground_gt=own.ground_gt))


if __name__ == "__main__":
    sys.exit(main())
