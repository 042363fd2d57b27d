#!/usr/bin/env python3
"""Entry point with the reference's control flow (main.py:37-280): options + YAML overlay, seeds, data, model,
optimizer (one group per tensor), epoch loop train -> eval -> ReduceLROnPlateau -> checkpoints (`model.pth`,
`model-best.pth`, `infos_*.pkl`, `histories_*.pkl`).  Differences: one process per GPU (torchrun) with an RCCL
gradient all-reduce instead of nn.DataParallel; the dataset is the synthetic stand-in unless a loader is injected.

  python -m cvc.main --path_opt cfgs/cyclical.yml --synthetic_clips 256 --max_epochs 2
"""
from __future__ import annotations

import argparse
import json
import os
import pickle
import random
import sys

import numpy as np
import torch
from torch.optim.lr_scheduler import ReduceLROnPlateau
from torch.utils.data import DataLoader

from . import opts as cvc_opts
from . import synth
from .data_synth import SyntheticCaptionDataset, collate
from .distributed import GradReducer, init_from_env, shard_range, exchange_comm, destroy_exchange_comm
from .misc import utils
from .model.create_model import build_model
from .trainer import Trainer, build_optimizer, ss_prob_at


LAST_TRAINER = None


def build_parser():
    """the reference's option surface (cvc.opts) plus the flags of this entry point"""
    parser = cvc_opts.build_parser()
    parser.add_argument("--synthetic_clips", type=int, default=128)
    parser.add_argument("--decode_weights", choices=("fp32", "bf16"), default="fp32",
                        help="precision of the caption decode's weight matrices: bf16 stores the six GEMM matrices rounded to bf16 "
                             "(greedy / one sample per clip, <= 64 rows; other decodes are refused, never run in fp32 instead)")
    # constrained decoding (DecodeEngine; eval, cvc.sample): flags of this entry point, not of the reference's option surface
    parser.add_argument("--no_repeat_ngram", type=int, default=0, help="never complete an n-gram the caption already holds; 0 = off")
    parser.add_argument("--no_immediate_repeat", action="store_true", help="never choose the previous word again")
    parser.add_argument("--min_caption_len", type=int, default=0, help="no end of sentence before this many words; 0 = off")
    parser.add_argument("--ban_words", type=str, default="", help="comma-separated words (or word ids) that are never chosen")
    parser.add_argument("--bad_endings", type=str, default="", help="comma-separated words (or word ids) a caption may not end on")
    # diverse (group) beam search and the length penalty of the final ranking (DecodeEngine beam_groups / diversity / length_penalty)
    parser.add_argument("--group_size", type=int, default=1, help="groups of diverse beam search (divides --beam_size); 1 = off")
    parser.add_argument("--diversity_lambda", type=float, default=0.0, help="Hamming diversity penalty between the groups; 0 = off")
    parser.add_argument("--length_penalty", type=float, default=0.0,
                        help="rank the final hypotheses by score / length^alpha; 0 = by score")
    # lexically constrained beam search (DecodeEngine force_n): words every caption should contain, or the clip's detections
    parser.add_argument("--force_words", type=str, default="", help="up to 3 comma-separated words (or word ids) every caption should "
                                                                    "contain (beam search; beam_size a multiple of their number + 1)")
    parser.add_argument("--force_detected", type=int, default=0,
                        help="force per clip the words of its C best-scored detection classes (C <= 3); 0 = off")
    parser.add_argument("--no_cfg", action="store_true", help="skip the YAML overlay (pure CLI)")
    parser.add_argument("--synthetic_raw", action="store_true",
                        help="feed raw frame / region features through the once-per-clip encoder (model/backbone.py) "
                             "instead of pre-extracted features")
    # self-critical training (Trainer.scst_step): sampled rollouts, CIDEr-D reward on the device
    parser.add_argument("--scst_after", type=int, default=-1,
                        help="take self-critical steps (CIDEr-D reward of sampled captions) from this epoch on; -1 = never")
    parser.add_argument("--scst_samples", type=int, default=5,
                        help="sampled captions per clip; > 1: leave-one-out baseline over the clip's samples, 1: greedy baseline")
    parser.add_argument("--scst_temperature", type=float, default=1.0, help="temperature of the rollouts")
    parser.add_argument("--scst_seed", type=int, default=1, help="seed of the rollouts' noise")
    parser.add_argument("--scst_dropout", action="store_true",
                        help="keep the training dropout on in the self-critical gradient pass (default: off, the policy that was sampled)")
    parser.add_argument("--scst_wor", action="store_true",
                        help="draw the self-critical rollouts WITHOUT replacement (a stochastic beam of scst_samples + 1 slots: no two "
                             "rollouts of a clip are the same sentence) and weight them by importance; 2 <= scst_samples <= 7")
    parser.add_argument("--scst_reward", type=str, default="cider:1",
                        help="the self-critical reward as name:weight pairs over cider, bleu1..bleu4, rougel (cvc.metrics), e.g. "
                             "cider:1,bleu4:0.5,rougel:0.5; the weights apply to the raw scales: CIDEr-D in [0, 10], the others in [0, 1]")
    # validation scores without external toolkits (Trainer(device_metrics=True); cvc.metrics)
    parser.add_argument("--val_metrics", choices=("none", "device"), default="none",
                        help="device: BLEU-1..4, ROUGE-L and CIDEr-D of the validation captions by word id, scored on the GPU; they "
                             "drive ReduceLROnPlateau and model-best.pth (not the toolkits' numbers: no PTB tokenizer)")
    # scheduled sampling (Trainer.train_step_prepared with model.ss_prob > 0): loop A fed the model's own sampled words
    parser.add_argument("--scheduled_sampling_start", type=int, default=-1,
                        help="from this epoch on a growing share of the decoder's training inputs are its own sampled words; -1 = never")
    parser.add_argument("--scheduled_sampling_increase_every", type=int, default=5, help="raise the share every this many epochs")
    parser.add_argument("--scheduled_sampling_increase_prob", type=float, default=0.05, help="by this much")
    parser.add_argument("--scheduled_sampling_max_prob", type=float, default=0.25, help="up to this share")
    parser.add_argument("--scheduled_sampling_temperature", type=float, default=1.0, help="temperature of the sampled words")
    parser.add_argument("--scheduled_sampling_seed", type=int, default=1, help="seed of the sampled words' noise and of the coins")
    # label smoothing of the cross-entropy steps (both language criteria of a training pass; cvc.functional.vocab_head_nll)
    parser.add_argument("--label_smoothing", type=float, default=0.0,
                        help="train against (1 - eps) one-hot + eps / vocabulary (torch's cross_entropy label_smoothing), eps in [0, 1); "
                             "0 = off.  Self-critical steps, scoring and evaluation are never smoothed; with eps > 0 the display line "
                             "also shows the unsmoothed NLL")
    # entropy regulariser of the vocabulary criterion (cvc.functional.vocab_head_nll entropy_beta=): all three are off by default
    # and then leave no key in the options -- every launch is what it was
    parser.add_argument("--confidence_penalty", type=float, default=argparse.SUPPRESS,
                        help="beta: the cross-entropy and scheduled-sampling steps add -beta x the mean entropy of the word "
                             "distribution to both language losses (Pereyra et al. 2017; beta > 0 penalises confident distributions); "
                             "the display line also shows the mean entropy H.  Evaluation and scoring carry no penalty")
    parser.add_argument("--scst_entropy", type=float, default=argparse.SUPPRESS,
                        help="beta: the self-critical steps add the entropy bonus -beta x the mean entropy of the word distribution "
                             "over the rollouts' steps to the loss (Williams & Peng 1991), against the collapse of the policy onto the "
                             "greedy caption.  The entropy is the model's full-vocabulary one at temperature 1, not the sampler's")
    parser.add_argument("--log_entropy", action="store_true", default=argparse.SUPPRESS,
                        help="report the mean entropy H of the word distribution on the display line and in the histories without "
                             "changing the loss (beta = 0 wherever no coefficient is given)")
    # consensus (minimum-Bayes-risk) caption selection at evaluation (model._sample(consensus=...); DecodeEngine.consensus)
    parser.add_argument("--consensus", choices=("off", "samples", "beam"), default="off",
                        help="keep per clip the candidate with the highest mean CIDEr-D against the clip's other candidates (training "
                             "captions' table): samples = --consensus_samples sampled captions (with --top_k / --top_p and the "
                             "constraints as they are set), beam = the --beam_size hypotheses of beam search")
    parser.add_argument("--consensus_samples", type=int, default=16, help="sampled candidates per clip (2 .. 32)")
    parser.add_argument("--consensus_temperature", type=float, default=1.0, help="temperature of the sampled candidates")
    parser.add_argument("--consensus_seed", type=int, default=1, help="seed of the sampled candidates' noise")
    # the selection's utility and the candidates' weights (DecodeEngine.consensus; csrc/consensus_mix.hip): absent by default and
    # then no key in the options, no launch changes
    parser.add_argument("--consensus_utility", type=str, default=argparse.SUPPRESS,
                        help="the utility of the consensus selection, a mix in --scst_reward's form over cider, bleu1..bleu4, rougel "
                             "(e.g. cider:1,bleu4:0.5,rougel:0.5): each of a clip's other candidates is ONE reference, the pick has "
                             "the highest (weighted) mean; default: CIDEr-D alone.  Needs --consensus samples|beam (cvc.sample: "
                             "its --consensus)")
    parser.add_argument("--consensus_weights", choices=("uniform", "model"), default=argparse.SUPPRESS,
                        help="how much each other candidate counts as a reference: uniform (default), or model = by "
                             "exp(--consensus_alpha x the model's log-prob of the hypothesis); model needs --consensus beam without "
                             "--stochastic_beam (sampled candidates are draws: their uniform mean is the expectation already)")
    parser.add_argument("--consensus_alpha", type=float, default=argparse.SUPPRESS,
                        help="with --consensus_weights model: the exponent on the hypotheses' probabilities, finite and >= 0 "
                             "(default 1; 0 = uniform)")
    # stochastic beam search at evaluation (model._sample(stochastic_beam=...); DecodeEngine stochastic)
    parser.add_argument("--stochastic_beam", action="store_true",
                        help="beam search by Gumbel-perturbed keys: the --beam_size hypotheses are distinct samples drawn without "
                             "replacement, the reported caption is the first draw (an ordinary sample); composes with the "
                             "constraints and --consensus beam, not with --group_size, --length_penalty or forced words")
    parser.add_argument("--stochastic_tau", type=float, default=1.0, help="temperature of the stochastic beam's sampling distribution")
    parser.add_argument("--sample_seed", type=int, default=0, help="seed of the stochastic beam's noise")
    # caption-set diversity of the evaluation's candidates (cvc.metrics.DiversityScorer): off by default and then no key in the options
    parser.add_argument("--val_diversity", action="store_true", default=argparse.SUPPRESS,
                        help="score the diversity of every clip's candidate set in validation (Div_1, Div_2, mBLEU_4, Unique and the "
                             "oracle CIDEr-D, on the GPU); needs --val_metrics device and a candidate set, i.e. --consensus samples|beam")
    parser.add_argument("--val_self_cider", action="store_true", default=argparse.SUPPRESS,
                        help="with --val_diversity: also score Self_CIDEr and LSA, the spectral diversity of every clip's candidate "
                             "set (cvc.metrics.SpectrumScorer, on the GPU)")
    # ensemble decoding (cvc.model.CaptionEnsemble): off by default and then no key in the options, no launch changes
    parser.add_argument("--ensemble", type=str, default=argparse.SUPPRESS,
                        help="comma-separated checkpoint files (state dicts of models built from the same options): evaluation, "
                             "cvc.sample and cvc.score decode with the resumed checkpoint (member 0) and these together, one word "
                             "choice per step from the combined distribution; needs --resume True.  Training steps never see it")
    parser.add_argument("--ensemble_weights", type=str, default=argparse.SUPPRESS,
                        help="comma-separated positive weights, one per member (the resumed checkpoint first); default: uniform")
    parser.add_argument("--ensemble_combine", choices=("prob", "logprob"), default=argparse.SUPPRESS,
                        help="prob: the weighted mean of the members' probabilities (default); logprob: of their log-probs")
    # word-level distillation from an ensemble of frozen checkpoints (cvc.model.CaptionEnsemble.soft_targets; cvc.functional
    # vocab_head_nll distill=): off by default and then no key in the options, no launch changes
    parser.add_argument("--distill_from", type=str, default=argparse.SUPPRESS,
                        help="comma-separated checkpoint files (state dicts of models built from the same options), the TEACHER: the "
                             "cross-entropy steps train loop A against the teacher's next-word distribution at every position of the "
                             "ground-truth captions, mixed with the one-hot loss; eager steps, the display line also shows NLL and KD.  "
                             "Not with --label_smoothing, --confidence_penalty / --log_entropy or scheduled sampling; self-critical "
                             "steps (--scst_after) are not distilled")
    parser.add_argument("--distill_weights", type=str, default=argparse.SUPPRESS,
                        help="comma-separated positive weights, one per teacher checkpoint; default: uniform")
    parser.add_argument("--distill_combine", choices=("prob", "logprob"), default=argparse.SUPPRESS,
                        help="prob: the weighted mean of the teachers' probabilities (default); logprob: of their log-probs")
    parser.add_argument("--distill_alpha", type=float, default=argparse.SUPPRESS,
                        help="the soft loss's share in [0, 1] (default 0.5): loss = (1 - alpha) NLL + alpha tau^2 KL(teacher || student)")
    parser.add_argument("--distill_temperature", type=float, default=argparse.SUPPRESS,
                        help="tau > 0 (default 1.0): both distributions are softmax(. / tau)")
    # weight averaging (Trainer(ema=...); cvc.optim._ClipStep.attach_ema): absent, they add no key and change no launch
    parser.add_argument("--ema_decay", type=float, default=argparse.SUPPRESS,
                        help="keep an exponential moving average of the weights with this decay, inside the native optimizer step; "
                             "validation, model-best.pth and the LR plateau schedule then use the averaged weights, model-ema.pth "
                             "holds them and model.pth stays the live ones; in [0, 1), 0 = off")
    parser.add_argument("--ema_warmup", action="store_true", default=argparse.SUPPRESS,
                        help="with --ema_decay: the decay of step n is min(decay, (1 + n) / (10 + n))")
    return parser


def check_ema_flags(opt):
    """--ema_decay lies in [0, 1) (a NaN does not) and needs the native optimizer step; --ema_warmup needs --ema_decay: anything
    else ends the run with a message, before any set-up"""
    d = getattr(opt, "ema_decay", None)
    if d is not None and not 0.0 <= d < 1.0:
        raise SystemExit("--ema_decay must lie in [0, 1), got %r" % (d,))
    if getattr(opt, "ema_warmup", False) and not d:
        raise SystemExit("--ema_warmup shapes the decay of --ema_decay: it needs --ema_decay d with 0 < d < 1")
    if d:
        from .trainer import CLIP_ADAM
        if not CLIP_ADAM:
            raise SystemExit("--ema_decay needs the native optimizer step (cvc.optim): the average is kept inside its update launch "
                             "and CVC_CLIP_ADAM=0 selects the library optimizers, which get none")


def check_distill_flags(opt):
    """--distill_from and its companions -> dict(paths, weights or None, combine, alpha, tau), or None with the flag absent.  Ends the
    run with a message, before any set-up: a companion flag without --distill_from, alpha outside [0, 1], a temperature that is not
    finite or <= 0, a weight count that does not match, malformed weights, more than 8 members, a missing file, and the combinations
    with label smoothing, the confidence penalty and scheduled sampling."""
    import math
    spec = getattr(opt, "distill_from", None)
    companions = ("distill_weights", "distill_combine", "distill_alpha", "distill_temperature")
    if spec is None:
        if any(hasattr(opt, k) for k in companions):
            raise SystemExit("--distill_weights / --distill_combine / --distill_alpha / --distill_temperature need --distill_from")
        return None
    alpha, tau = getattr(opt, "distill_alpha", 0.5), getattr(opt, "distill_temperature", 1.0)
    if not 0.0 <= alpha <= 1.0:                # (a NaN fails the comparison)
        raise SystemExit("--distill_alpha must lie in [0, 1], got %r" % (alpha,))
    if not (math.isfinite(tau) and tau > 0.0):
        raise SystemExit("--distill_temperature must be finite and > 0, got %r" % (tau,))
    if getattr(opt, "label_smoothing", 0.0) > 0 or hasattr(opt, "confidence_penalty") or getattr(opt, "log_entropy", False):
        raise SystemExit("--distill_from excludes --label_smoothing > 0, --confidence_penalty and --log_entropy: the teacher's row is the "
                         "target distribution")
    if getattr(opt, "scheduled_sampling_start", -1) >= 0:
        raise SystemExit("--distill_from and scheduled sampling (--scheduled_sampling_start) exclude each other: the student would be fed "
                         "words the teacher never saw")
    paths = [p.strip() for p in spec.split(",") if p.strip()]
    if not paths:
        raise SystemExit("--distill_from names no checkpoint file")
    weights = None
    if hasattr(opt, "distill_weights"):
        try:
            weights = [float(w) for w in opt.distill_weights.split(",")]
        except ValueError:
            raise SystemExit("--distill_weights must be comma-separated numbers, got %r" % (opt.distill_weights,)) from None
        if len(weights) != len(paths):
            raise SystemExit("--distill_weights has %d weights for %d teacher checkpoints" % (len(weights), len(paths)))
        if not all(np.isfinite(w) and w > 0 for w in weights):
            raise SystemExit("--distill_weights must be finite numbers > 0, got %r" % (opt.distill_weights,))
    if len(paths) > 8:
        raise SystemExit("--distill_from: an ensemble has at most 8 members, got %d" % len(paths))
    for p in paths:
        if not os.path.isfile(p):
            raise SystemExit("--distill_from: no such checkpoint file: %s" % p)
    return dict(paths=paths, weights=weights, combine=getattr(opt, "distill_combine", "prob"), alpha=float(alpha), tau=float(tau))


def check_ensemble_flags(opt):
    """--ensemble and its two companions -> (checkpoint paths, weights or None, combine), or None with the flag absent.  Ends the run
    with a message, before any set-up: no --resume True, a weight count that does not match, malformed weights, a missing file, a
    companion flag without --ensemble."""
    spec = getattr(opt, "ensemble", None)
    if spec is None:
        if hasattr(opt, "ensemble_weights") or hasattr(opt, "ensemble_combine"):
            raise SystemExit("--ensemble_weights / --ensemble_combine need --ensemble")
        return None
    paths = [p.strip() for p in spec.split(",") if p.strip()]
    if not paths:
        raise SystemExit("--ensemble names no checkpoint file")
    if not opt.resume:
        raise SystemExit("--ensemble needs --resume True: the resumed checkpoint is member 0 of the ensemble")
    if getattr(opt, "eval_obj_grounding_gt", False):
        raise SystemExit("--ensemble and --eval_obj_grounding_gt exclude each other: the grounding on GT sentences reads one model's "
                         "frame-masked attention and grounder")
    weights = None
    if hasattr(opt, "ensemble_weights"):
        try:
            weights = [float(w) for w in opt.ensemble_weights.split(",")]
        except ValueError:
            raise SystemExit("--ensemble_weights must be comma-separated numbers, got %r" % (opt.ensemble_weights,)) from None
        if len(weights) != len(paths) + 1:
            raise SystemExit("--ensemble_weights has %d weights for %d members (the resumed checkpoint and %d of --ensemble)"
                             % (len(weights), len(paths) + 1, len(paths)))
        if not all(np.isfinite(w) and w > 0 for w in weights):
            raise SystemExit("--ensemble_weights must be finite numbers > 0, got %r" % (opt.ensemble_weights,))
    if len(paths) + 1 > 8:
        raise SystemExit("--ensemble: an ensemble has at most 8 members, got %d" % (len(paths) + 1))
    for p in paths:
        if not os.path.isfile(p):
            raise SystemExit("--ensemble: no such checkpoint file: %s" % p)
    return paths, weights, getattr(opt, "ensemble_combine", "prob")


def check_member_state(path, state, reference, flag="--ensemble"):
    """an --ensemble member's (or a --distill_from teacher's) state dict against the resumed (the trained) model's: a vocabulary of
    another size (the embedding, the vocabulary head) or any other tensor of another shape ends the run with a message"""
    for k in ("embed.0.weight", "logit.weight"):
        if k in state and k in reference and tuple(state[k].shape) != tuple(reference[k].shape):
            raise SystemExit("%s: %s has a different vocabulary: %s is %s, the resumed checkpoint's %s (the members choose one "
                             "word from one vocabulary)" % (flag, path, k, tuple(state[k].shape), tuple(reference[k].shape)))
    bad = sorted(k for k in reference if k not in state or tuple(state[k].shape) != tuple(reference[k].shape))
    if bad:
        raise SystemExit("%s: %s does not fit a model built from these options: %s" % (flag, path, ", ".join(bad[:4])))


def check_val_diversity_flag(opt):
    """--val_diversity needs the device metrics and an evaluation that decodes a candidate set per clip: anything else ends the run
    with a message, before any set-up"""
    if getattr(opt, "val_self_cider", False) and not getattr(opt, "val_diversity", False):
        raise SystemExit("--val_self_cider needs --val_diversity (it scores the same candidate sets)")
    if not getattr(opt, "val_diversity", False):
        return
    if opt.val_metrics != "device":
        raise SystemExit("--val_diversity needs --val_metrics device (the diversity scores are computed on the GPU next to them)")
    if opt.consensus == "off":
        raise SystemExit("--val_diversity needs a candidate set per clip in evaluation: --consensus samples or --consensus beam")


def check_consensus_mix_flags(opt, sample=None):
    """--consensus_utility / --consensus_weights / --consensus_alpha refine a consensus selection: given without one (--consensus
    samples|beam; under cvc.sample its own --consensus), with a mix that does not parse, with model weights over sampled candidates,
    or with an alpha that is not a finite number >= 0, the run ends with a message, before any set-up.  The parsed mix replaces the
    string in opt.consensus_utility ({name: weight}, what the model reads)."""
    import math
    given = [k for k in ("consensus_utility", "consensus_weights", "consensus_alpha") if hasattr(opt, k)]
    if not given:
        return
    selecting = (len(sample) > 5 and bool(sample[5])) if sample is not None else opt.consensus != "off"
    if not selecting:
        raise SystemExit("--%s refines the consensus selection: it needs --consensus samples or --consensus beam (python -m cvc.sample: "
                         "--consensus)" % given[0])
    if hasattr(opt, "consensus_utility"):
        from .metrics import parse_reward_weights
        opt.consensus_utility = parse_reward_weights(opt.consensus_utility, "--consensus_utility")
        if not any(w > 0 for w in opt.consensus_utility.values()):
            raise SystemExit("--consensus_utility: every weight is 0 -- the utility would weigh nothing")
    if getattr(opt, "consensus_weights", "uniform") == "model":
        if sample is not None or opt.consensus != "beam" or opt.stochastic_beam:
            raise SystemExit("--consensus_weights model weights the hypotheses of a beam by the model's probability: it needs "
                             "--consensus beam without --stochastic_beam (the candidates of --consensus samples, of cvc.sample and of "
                             "a stochastic beam are draws, whose uniform mean is the expectation already)")
    alpha = getattr(opt, "consensus_alpha", None)
    if alpha is not None and not (math.isfinite(alpha) and alpha >= 0):
        raise SystemExit("--consensus_alpha must be a finite number >= 0, got %r" % (alpha,))


def check_label_smoothing_flag(eps):
    """--label_smoothing lies in [0, 1) (a NaN does not): anything else ends the run with a message, before any set-up"""
    if not 0.0 <= eps < 1.0:
        raise SystemExit("--label_smoothing must lie in [0, 1), got %r" % (eps,))


def check_entropy_flags(opt):
    """--confidence_penalty and --scst_entropy are finite numbers where given: anything else ends the run with a message, before any
    set-up"""
    import math
    for name in ("confidence_penalty", "scst_entropy"):
        beta = getattr(opt, name, None)
        if beta is not None and not math.isfinite(beta):
            raise SystemExit("--%s must be a finite number, got %r" % (name, beta))


def main(argv=None, sample=None, score=None):
    """sample: (n, temperature, seed), (n, temperature, seed, top_k, top_p), (n, temperature, seed, top_k, top_p, consensus) or (..., consensus, without_replacement) or (..., without_replacement, diversity) or (..., diversity, self_cider) -- set up as for evaluation (checkpoint loading included), then write the validation split's
    sampled captions (Trainer.sample) instead of the epoch loop (python -m cvc.sample).
    score: dict(ground_gt=bool) -- the same set-up, then the teacher-forced scores of the validation split's GT captions
    (Trainer.score) and, if asked for, the grounding on the GT sentences (Trainer.ground_gt) (python -m cvc.score)."""
    parser = build_parser()
    opt = parser.parse_args(argv)
    check_label_smoothing_flag(opt.label_smoothing)
    check_entropy_flags(opt)
    check_val_diversity_flag(opt)
    check_consensus_mix_flags(opt, sample)
    check_ema_flags(opt)
    if not opt.no_cfg:
        opt = cvc_opts.load_cfg(opt)
    ensemble = check_ensemble_flags(opt)
    distill = check_distill_flags(opt)
    if ensemble is not None and score is not None and score.get("ground_gt"):
        raise SystemExit("--ensemble and --ground_gt exclude each other: the grounding on GT sentences reads one model's frame-masked "
                         "attention and grounder")
    opt.test_mode = opt.val_split in ["testing", "hidden_test"]                       # reference main.py:57
    rank, world, local_rank = init_from_env(opt.dist_backend) if "RANK" in os.environ else (0, 1, 0)
    device = torch.device("cuda", local_rank) if torch.cuda.is_available() else None
    if device is None:
        raise SystemExit("cvc.main needs an MI355X: the hot path has no CPU fallback")
    torch.cuda.set_device(device)
    random.seed(opt.seed); np.random.seed(opt.seed); torch.manual_seed(opt.seed)     # reference main.py:63-67

    per_rank_bs = max(1, opt.batch_size // world)
    if opt.input_dic:
        # ---- the reference's on-disk dataset (misc/dataloader_anet.py; main.py:78-114): .npy features, proposal arrays,
        # annotation JSONs -> 12-tuples -> raw features through the once-per-clip encoder
        from .misc.dataloader_anet import ANetEntitiesDataset, collate as anet_collate
        full = ANetEntitiesDataset(opt, split=opt.train_split, seq_per_img=opt.seq_per_img)
        val_full = ANetEntitiesDataset(opt, split=opt.val_split, seq_per_img=opt.seq_per_img, num_proposals=full.num_proposals,
                                       label_proposals=full.label_proposals)
        sl = shard_range(len(full), rank, world, equal=True)
        vsl = shard_range(len(val_full), rank, world)
        loader = DataLoader(torch.utils.data.Subset(full, range(sl.start, sl.stop)), batch_size=per_rank_bs, shuffle=True,
                            num_workers=opt.num_workers, collate_fn=anet_collate, drop_last=True)
        val_loader = DataLoader(torch.utils.data.Subset(val_full, range(vsl.start, vsl.stop)), batch_size=per_rank_bs, shuffle=False,
                                num_workers=opt.num_workers, collate_fn=anet_collate)
        opt.vocab_size, opt.detect_size = full.vocab_size, full.detect_size                # reference main.py:100-114
        opt.glove_w, opt.glove_vg_cls, opt.glove_clss = (torch.from_numpy(getattr(full, k)).float()
                                                         for k in ("glove_w", "glove_vg_cls", "glove_clss"))
        for k in ("wtoi", "itow", "itod", "ltow", "itoc", "wtol", "wtod", "vg_cls"):
            setattr(opt, k, getattr(full, k))
    else:
        dims = synth.Dims(B=opt.batch_size, N=opt.num_prop_per_frm, F=opt.t_attn_size, R=opt.rnn_size, A=opt.att_hid_size,
                          E=opt.input_encoding_size, T=opt.seq_length, G=opt.vis_encoding_size, K=min(8, opt.num_prop_per_frm))
        full = SyntheticCaptionDataset(dims, opt.synthetic_clips, opt.seed, opt.train_split, raw=opt.synthetic_raw)
        # clips are sharded across ranks; every rank gets the SAME number of clips (the remainder is dropped) so that all
        # ranks run the same number of steps and issue the same collectives
        sl = shard_range(len(full), rank, world, equal=True)
        train_set = torch.utils.data.Subset(full, range(sl.start, sl.stop))
        loader = DataLoader(train_set, batch_size=per_rank_bs, shuffle=True, num_workers=0, collate_fn=collate, drop_last=True)
        val_loader = DataLoader(train_set, batch_size=per_rank_bs, shuffle=False, num_workers=0, collate_fn=collate)
        # fields the reference injects into opt from the dataset (main.py:100-114)
        opt.vocab_size, opt.itow, opt.wtoi, opt.itod, opt.detect_size = full.vocab_size, full.itow, full.wtoi, full.itod, dims.DET
        if opt.synthetic_raw:
            if opt.att_feat_size != opt.vis_encoding_size:
                raise SystemExit("--synthetic_raw needs att_feat_size == vis_encoding_size (fc7 is square, backbone.py:115)")
            opt.glove_clss, opt.glove_vg_cls = torch.from_numpy(full.glove_clss), torch.from_numpy(full.glove_vg_cls)
            opt.vg_cls, opt.detectron_tables = full.vg_cls, full.tables

    if opt.no_repeat_ngram < 0 or opt.min_caption_len < 0:
        raise SystemExit("--no_repeat_ngram and --min_caption_len must be >= 0")
    if opt.group_size < 1 or opt.diversity_lambda < 0 or opt.length_penalty < 0:
        raise SystemExit("--group_size must be >= 1, --diversity_lambda and --length_penalty >= 0")
    if opt.scst_samples < 1 or opt.scst_temperature <= 0:
        raise SystemExit("--scst_samples must be >= 1 and --scst_temperature > 0")
    if opt.scst_wor and not 2 <= opt.scst_samples <= 7:
        raise SystemExit("--scst_wor needs 2 <= --scst_samples <= 7 (a stochastic beam of scst_samples + 1 <= 8 slots; one rollout's own "
                         "baseline cancels it)")
    if (opt.scheduled_sampling_increase_every < 1 or opt.scheduled_sampling_temperature <= 0 or opt.scheduled_sampling_increase_prob < 0
            or not 0 <= opt.scheduled_sampling_max_prob <= 1):
        raise SystemExit("--scheduled_sampling_increase_every must be >= 1, --scheduled_sampling_temperature > 0, "
                         "--scheduled_sampling_increase_prob >= 0 and --scheduled_sampling_max_prob in [0, 1]")
    if not 2 <= opt.consensus_samples <= 32 or opt.consensus_temperature <= 0:
        raise SystemExit("--consensus_samples lies in 2 .. 32 and --consensus_temperature must be > 0")
    if opt.stochastic_beam and (opt.beam_size < 2 or not opt.stochastic_tau > 0):
        raise SystemExit("--stochastic_beam needs --beam_size > 1 and --stochastic_tau > 0")
    if opt.consensus == "beam" and opt.beam_size < 2:
        raise SystemExit("--consensus beam chooses among the hypotheses of beam search: it needs --beam_size > 1")
    from .metrics import parse_reward_weights
    opt.scst_reward_weights = parse_reward_weights(opt.scst_reward)                                       # (Trainer reads these)
    opt.ss_temperature, opt.ss_seed = opt.scheduled_sampling_temperature, opt.scheduled_sampling_seed     # (Trainer reads these)
    opt.force_word_ids = word_ids(opt.force_words, opt.wtoi, "--force_words")
    if len(opt.force_word_ids) > 3 or not 0 <= opt.force_detected <= 3 or (opt.force_word_ids and opt.force_detected):
        raise SystemExit("--force_words takes at most 3 words, --force_detected lies in 0 .. 3, and only one of them is given")
    opt.ban_word_ids = word_ids(opt.ban_words, opt.wtoi, "--ban_words")
    opt.bad_ending_ids = word_ids(opt.bad_endings, opt.wtoi, "--bad_endings")
    model = build_model(opt, device)
    save_dir = os.path.join(opt.checkpoint_path, opt.exp_name)

    # ---- resume (reference main.py:119-163): state_dict + infos (+ histories) of `model.pth` or `model-best.pth`
    infos, histories = {}, {}
    if opt.resume:
        suffix = "-best" if opt.load_best_score else ""
        model_path = os.path.join(save_dir, "model%s.pth" % suffix)
        info_path = os.path.join(save_dir, "infos_" + opt.id + suffix + ".pkl")
        with open(info_path, "rb") as f:
            infos = pickle.load(f)
        model.load_state_dict(torch.load(model_path, map_location=device))
        hist_path = os.path.join(save_dir, "histories_" + opt.id + ".pkl")
        if os.path.isfile(hist_path):
            with open(hist_path, "rb") as f:
                histories = pickle.load(f)
        if rank == 0:
            print("resumed %s (epoch %s, best CIDEr %s)" % (model_path, infos.get("epoch"), infos.get("best_val_score")))
    elif opt.inference_only:
        raise SystemExit("--inference_only needs --resume True (a checkpoint under %s): refusing to evaluate randomly "
                         "initialised weights" % save_dir)
    best = infos.get("best_val_score", None)
    if opt.resume_decoder_exp_name != "" and not opt.resume:                           # reference main.py:156-160
        start_epoch = getattr(opt, "start_epoch", 0)
    else:
        start_epoch = infos.get("epoch", 0)
    val_result_history = histories.get("val_result_history", {})
    lr_history = histories.get("lr_history", {})
    ss_prob_history = histories.get("ss_prob_history", {})

    optimizer = build_optimizer(model, opt)
    # the weight average is a training matter: an evaluation-only run (--inference_only, cvc.sample, cvc.score) decodes the checkpoint
    # it resumed, as without the flags
    ema = None
    if getattr(opt, "ema_decay", 0) and not (opt.inference_only or sample is not None or score is not None):
        ema = (opt.ema_decay, bool(getattr(opt, "ema_warmup", False)))
    # flat gradient arenas; exchanges only when world > 1 -- on the package's own RCCL communicator (--dist_backend rccl, the
    # default: torch.distributed on gloo is the control plane only), whose collectives are captured into the step's HIP graph
    comm = exchange_comm() if (world > 1 and opt.dist_backend == "rccl") else None
    reducer = GradReducer(model.named_parameters(), comm=comm)
    trainer = Trainer(opt, full, model, optimizer, loader, val_loader, grad_reducer=reducer, device_metrics=opt.val_metrics == "device",
                      **(dict(val_diversity=True) if getattr(opt, "val_diversity", False) else {}),
                      **(dict(val_self_cider=True) if getattr(opt, "val_self_cider", False) else {}),
                      **(dict(ema=ema or False) if hasattr(opt, "ema_decay") else {}))       # (False: none, whatever opt says)
    if ema is not None and opt.resume:
        # the shadows and their step count go on from model-ema.pth; a run directory from before the average has none
        ema_path = os.path.join(save_dir, "model-ema.pth")
        if os.path.isfile(ema_path):
            optimizer.load_ema_state_dict(model, torch.load(ema_path, map_location=device))
            if rank == 0:
                print("resumed %s (%d averaged steps)" % (ema_path, optimizer.ema_updates))
        elif rank == 0:
            print("no %s: the weight average starts from the resumed weights" % ema_path)
    if ensemble is not None:                                   # evaluation, cvc.sample and cvc.score decode through the ensemble
        from .model.ensemble import CaptionEnsemble
        members = [getattr(model, "module", model)]
        for p in ensemble[0]:
            state = torch.load(p, map_location=device)
            check_member_state(p, state, members[0].state_dict())
            member = build_model(opt, device)
            member.load_state_dict(state)
            members.append(getattr(member, "module", member))
        trainer.ensemble = CaptionEnsemble(members, weights=ensemble[1], combine=ensemble[2])
        if rank == 0:
            print("ensemble of %d checkpoints (%s)" % (len(members), ensemble[2]))
    if distill is not None and not opt.inference_only and sample is None and score is None:
        # the teacher: frozen checkpoints behind one CaptionEnsemble, on the trained model (Trainer._kd_step_prepared reads it there)
        from .model.ensemble import CaptionEnsemble
        core = getattr(model, "module", model)
        teachers = []
        for p in distill["paths"]:
            state = torch.load(p, map_location=device)
            check_member_state(p, state, core.state_dict(), flag="--distill_from")
            member = build_model(opt, device)
            member.load_state_dict(state)
            member = getattr(member, "module", member).eval()
            member.requires_grad_(False)
            teachers.append(member)
        core.distill = dict(teacher=CaptionEnsemble(teachers, weights=distill["weights"], combine=distill["combine"]),
                            alpha=distill["alpha"], tau=distill["tau"])
        if rank == 0:
            print("distilling from %d checkpoints (%s), alpha %g, temperature %g" % (len(teachers), distill["combine"], distill["alpha"],
                                                                                      distill["tau"]))
    global LAST_TRAINER
    LAST_TRAINER = trainer                                     # (tests and notebooks: graph / deferred-error statistics of the run)
    if sample is not None:
        path = trainer.sample(*sample[:3], **dict(zip(("top_k", "top_p", "consensus", "without_replacement", "diversity", "self_cider"), sample[3:])))
        if rank == 0:
            print("samples written to %s" % path)
        if comm is not None:
            destroy_exchange_comm()
        return 0
    if score is not None:
        stats = trainer.score()
        if score.get("ground_gt"):
            stats.update(trainer.ground_gt())
        if rank == 0:
            print("scores written to %s: %s" % (trainer.scores_file, json.dumps(stats)))
        if comm is not None:
            destroy_exchange_comm()
        return 0
    scheduler = ReduceLROnPlateau(optimizer, 'max', patience=opt.patience, min_lr=opt.min_lr)
    tb = utils.set_tb_logger(opt.tb_log_dir, opt.exp_name, opt.resume) if (rank == 0 and opt.tensorboard and not opt.inference_only) else None

    for epoch in range(start_epoch, opt.max_epochs):
        if not opt.inference_only:
            if opt.scheduled_sampling_start >= 0:               # the schedule is on: the epoch's share, set before the epoch and recorded
                core = getattr(model, "module", model)
                core.ss_prob = ss_prob_at(epoch, opt.scheduled_sampling_start, opt.scheduled_sampling_increase_every,
                                          opt.scheduled_sampling_increase_prob, opt.scheduled_sampling_max_prob)
                ss_prob_history[epoch] = core.ss_prob
            trainer.train(epoch, tb)
        if epoch % max(opt.val_every_epoch, 1) != 0:        # reference main.py:221: scheduler + checkpoints only with an eval
            continue
        stats = trainer.eval(epoch, tb)
        if opt.inference_only:
            break
        score = stats.get("CIDEr")                            # None without a scorer (--val_metrics device, or an external one)
        if world > 1:                                         # only rank 0 scores: every rank must step its LR schedule alike
            box = [score]
            torch.distributed.broadcast_object_list(box, src=0)
            score = box[0]
        if score is not None:                                 # no score -> no plateau evidence: leave the LR alone
            scheduler.step(score)
        if rank == 0:
            os.makedirs(save_dir, exist_ok=True)
            best_flag = score is not None and (best is None or score > best)
            if best_flag:
                best = score
            torch.save(model.state_dict(), os.path.join(save_dir, "model.pth"))         # the live weights: what training resumes from
            ema_sd = optimizer.ema_state_dict(model) if trainer.ema_active else None
            if ema_sd is not None:
                torch.save(ema_sd, os.path.join(save_dir, "model-ema.pth"))
            val_result_history[epoch] = dict(stats)
            lr_history[epoch] = optimizer.param_groups[0]["lr"]
            infos = {"iter": (epoch + 1) * max(len(loader) - 1, 0), "epoch": epoch, "best_val_score": best, "vocab": full.itow,
                     "opt": {k: v for k, v in vars(opt).items() if _picklable(v)}}
            if ema_sd is not None:
                infos.update(ema_updates=ema_sd["updates"], ema_decay=ema[0], ema_warmup=ema[1])
            histories = {"val_result_history": val_result_history, "loss_history": {}, "lr_history": lr_history,
                         "ss_prob_history": dict(ss_prob_history), "reward_history": dict(trainer.reward_history),
                         "nll_history": dict(trainer.nll_history), "entropy_history": dict(trainer.entropy_history),
                         **({"kd_history": dict(trainer.kd_history)} if distill is not None else {})}
            with open(os.path.join(save_dir, "infos_" + opt.id + ".pkl"), "wb") as f:
                pickle.dump(infos, f)
            with open(os.path.join(save_dir, "histories_" + opt.id + ".pkl"), "wb") as f:
                pickle.dump(histories, f)
            if best_flag or not os.path.isfile(os.path.join(save_dir, "model-best.pth")):
                # (the weights that were scored: the averaged ones when there is an average)
                torch.save(model.state_dict() if ema_sd is None else {k: v for k, v in ema_sd.items() if k != "updates"},
                           os.path.join(save_dir, "model-best.pth"))
                with open(os.path.join(save_dir, "infos_" + opt.id + "-best.pkl"), "wb") as f:
                    pickle.dump(infos, f)
    if comm is not None:
        trainer._graphs.clear()                               # captured steps hold work on the communicator
        destroy_exchange_comm()
    return 0


def word_ids(spec: str, wtoi, flag: str):
    """"a,the,17" -> word ids: an entry is an integer id or a word of the dataset's vocabulary (wtoi); an unknown word is a
    SystemExit that names it."""
    out = []
    for w in (x.strip() for x in (spec or "").split(",")):
        if not w:
            continue
        if w.lstrip("-").isdigit():
            out.append(int(w))
        elif w in wtoi:
            out.append(int(wtoi[w]))
        else:
            raise SystemExit("%s: unknown word %r (not in the dataset's vocabulary)" % (flag, w))
    return out


def _picklable(v):
    try:
        pickle.dumps(v)
        return True
    except Exception:
        return False


if __name__ == "__main__":
    sys.exit(main())
