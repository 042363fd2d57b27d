"""Validation scores on the device (Trainer(device_metrics=True), cvc.main --val_metrics device) at tiny synthetic dimensions: what
the epoch loop records and selects by, and eval's six numbers against the restatements (tests/overlap_ref.py, tests/cider_ref.py) on a
re-decode of the same validation batches.  Every test prints its figures before it asserts."""
import math
import os
import pickle

import numpy as np
import pytest
import torch

import cider_ref as C
import overlap_ref as R

pytestmark = pytest.mark.gpu

KEYS = ["Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L", "CIDEr"]
FLOOR = 2.0 ** -23            # tests/test_gpu_overlap.py
FLOOR_CIDER = 2.0 ** -20      # tests/test_gpu_cider.py


def _main(tmp, name, epochs, *extra):
    from cvc import main as cvc_main
    rc = cvc_main.main(["--no_cfg", "--max_epochs", str(epochs), "--batch_size", "4", "--synthetic_clips", "12", "--num_prop_per_frm", "7",
                        "--t_attn_size", "5", "--rnn_size", "32", "--att_hid_size", "16", "--input_encoding_size", "16", "--seq_length", "6",
                        "--vis_encoding_size", "24", "--tensorboard", "0", "--disp_interval", "1", "--exp_name", name, "--learning_rate", "0.001",
                        "--results_dir", str(tmp / "results"), "--checkpoint_path", str(tmp) + "/", "--id", name, *extra])
    assert rc == 0
    load = lambda f: pickle.load(open(os.path.join(tmp, name, f), "rb"))
    return cvc_main.LAST_TRAINER, load("infos_%s.pkl" % name), load("histories_%s.pkl" % name)


def test_main_records_scores_and_selects_the_best_checkpoint_by_them(tmp_path):
    tr, infos, hist = _main(tmp_path, "m", 2, "--val_metrics", "device")
    h = hist["val_result_history"]
    print(f"[metrics eval] --val_metrics device: history {h}, best_val_score {infos['best_val_score']}")
    assert sorted(h) == [0, 1] and tr.device_metrics
    for e in (0, 1):
        assert sorted(h[e]) == sorted(KEYS), h[e]
        assert all(isinstance(h[e][k], float) and math.isfinite(h[e][k]) and h[e][k] >= 0.0 for k in KEYS), h[e]
        assert all(h[e][k] <= 1.0 for k in KEYS[:5]) and h[e]["CIDEr"] <= 10.0
    assert infos["best_val_score"] == max(h[e]["CIDEr"] for e in h)
    assert os.path.isfile(os.path.join(tmp_path, "m", "model-best.pth"))
    best = pickle.load(open(os.path.join(tmp_path, "m", "infos_m-best.pkl"), "rb"))
    assert h[best["epoch"]]["CIDEr"] == infos["best_val_score"]
    tr0, infos0, hist0 = _main(tmp_path, "n", 2)
    print(f"[metrics eval] without the flag: history {hist0['val_result_history']}, best_val_score {infos0['best_val_score']}")
    assert not tr0.device_metrics and infos0["best_val_score"] is None
    assert all(dict(v) == {} for v in hist0["val_result_history"].values()) and sorted(hist0["val_result_history"]) == [0, 1]


class _OwnCaptionsAsReferences(torch.utils.data.Dataset):
    """the wrapped dataset with references made from the model's own greedy captions, so that the scores are not all zero after two
    training steps: clip i gets two references -- its decoded caption (i % 3 == 0: as it is; 1: one word changed; 2: the dataset's own
    reference instead) and the decoded caption's first three words.  The decode does not read the references."""

    def __init__(self, base, decoded):
        self.base, self.decoded = base, decoded

    def __len__(self):
        return len(self.base)

    def __getitem__(self, i):
        it = list(self.base[i])
        gt, num = it[2].clone(), it[3].clone()
        own = torch.zeros(gt.shape[1], dtype=gt.dtype)
        own[:self.decoded.shape[1]] = torch.from_numpy(self.decoded[i])
        if i % 3 == 1:
            own[1] = own[1] % 5 + 1
        if i % 3 != 2:
            gt[0] = own
        gt[1] = 0
        gt[1, :3] = own[:3]
        num[0] = 2
        it[2], it[3] = gt, num
        return tuple(it)


def _decode(tr):
    from cvc.prefetch import DevicePrefetcher
    seqs, refs, nrefs = [], [], []
    tr.model.eval()
    with torch.no_grad():
        for b in DevicePrefetcher(tr.val_loader, lambda raw: tr._prepare(raw, False), tr.device):
            seq = tr._call(b, True)[0]
            seqs.append(seq.cpu().numpy())
            refs.append(b["gt_seqs"][:, :, :seq.size(1)].cpu().numpy())
            nrefs.append(b["num"][:, 0].cpu().numpy())
    return np.concatenate(seqs), np.concatenate(refs), np.concatenate(nrefs).astype(np.int32)


def test_eval_against_the_restatements_on_a_redecode(tmp_path):
    """greedy decode is bit-reproducible: the captions eval scored are the captions decoded here.  Corpus BLEU: the integer sums and
    the host's fp64 formula are the restatement's, hence 1e-12 relative.  ROUGE_L and CIDEr are means of fp32 per-caption scores: a mean's
    error is at most the largest per-caption error, so the bound is the per-caption rule's -- 4 x the largest error of the restatement
    evaluated in fp32, with the floors 2^-23 (ROUGE-L) and 2^-20 (CIDEr-D)."""
    from cvc.trainer import Trainer
    tr0, _infos, _hist = _main(tmp_path, "e", 1)
    decoded = _decode(tr0)[0]
    loader = torch.utils.data.DataLoader(_OwnCaptionsAsReferences(tr0.val_loader.dataset, decoded), batch_size=4, shuffle=False,
                                         collate_fn=tr0.val_loader.collate_fn)
    tr = Trainer(tr0.opts, tr0.dataset, tr0.model, tr0.optimizer, None, loader, device_metrics=True)
    got = tr.eval(0)
    print(f"[metrics eval] eval(0): {got}")
    assert list(got) == KEYS
    assert Trainer(tr0.opts, tr0.dataset, tr0.model, tr0.optimizer, None, loader).eval(0) == {}          # the keyword is off: as ever
    seq, ref, nref = _decode(tr)
    assert seq.shape == (12, 6) and ref.shape[0] == 12 and (nref == 2).all() and np.array_equal(seq, decoded)
    # the table's corpus: the validation loader's own captions
    ds = tr.val_loader.dataset
    caps = []
    for i in range(len(ds)):
        it = ds[i]
        caps.extend(np.asarray(it[2])[r] for r in range(int(np.asarray(it[3]).reshape(-1)[0])))
    assert len(caps) == 24 and tr._val_cider.n_doc == 24
    df, n_doc = C.doc_freq(caps)
    o64, o32 = R.score_batch(seq, ref, nref), R.score_batch(seq, ref, nref, dt=np.float32)
    c64, c32 = C.score_batch(seq, ref, nref, df, n_doc)[0], C.score_batch(seq, ref, nref, df, n_doc, dt=np.float32)[0]
    want_bleu = R.corpus(o64["stats"].sum(0))
    print(f"[metrics eval] restatement: summed statistics {o64['stats'].sum(0).tolist()}, corpus BLEU {want_bleu.tolist()}, ROUGE_L "
          f"{o64['rouge'].mean():.7f}, CIDEr {c64.mean():.7f}; captions with words {int((o64['stats'][:, 8] > 0).sum())}/12")
    # not vacuous: 4-grams match, and not everywhere; the two means are neither 0 nor at their maximum
    assert 0 < o64["stats"][:, 3].sum() < o64["stats"][:, 7].sum() and 0.0 < o64["rouge"].mean() < 1.0 and 0.0 < c64.mean() < 10.0
    for k in range(4):
        assert got["Bleu_%d" % (k + 1)] == pytest.approx(want_bleu[k], rel=1e-12, abs=0), k
    for name, w64, w32, floor in (("ROUGE_L", o64["rouge"], o32["rouge"], FLOOR), ("CIDEr", c64, c32, FLOOR_CIDER)):
        bound = max(4.0 * float(np.abs(w32 - w64).max()), floor)
        err = abs(got[name] - float(w64.mean()))
        print(f"[metrics eval] {name}: eval {got[name]:.9f}, fp64 {w64.mean():.9f}, |err| {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (name, err, bound)
