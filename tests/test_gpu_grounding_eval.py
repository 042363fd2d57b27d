"""Trainer.eval with --val_metrics device --eval_obj_grounding over the on-disk fixture dataset (cvc.main, one epoch): the grounding scores
in lang_stats against the restatement (tests/grounding_ref.py) on a re-decode of the same batches, the grounding file built from the
kernel's picks against the host route's, and the key sets with either switch alone."""
import json
import pickle

import numpy as np
import pytest
import torch

import grounding_ref as R

pytestmark = pytest.mark.gpu


def test_eval_scores_the_generated_captions_grounding_and_writes_the_same_file(tmp_path):
    from cvc import main as cvc_main
    from cvc import metrics, synth
    from cvc.data_fixture import write_tiny_anet_dataset, CLASSES, VG_CLASSES
    from cvc.misc import utils
    from cvc.prefetch import DevicePrefetcher
    root = tmp_path / "anet"
    o = write_tiny_anet_dataset(str(root), seed=7, feat=24, rgb_dim=2048, bn_dim=1024, n_videos=6)
    d = synth.Dims(G=24, DET=len(CLASSES))
    tables = synth.detectron_tables(d, 7, n_vg=len(VG_CLASSES) + 1)
    wdir = root / "detectron"
    wdir.mkdir()
    for k in ("fc7_w", "fc7_b", "cls_score_w", "cls_score_b"):
        pickle.dump(tables[k], open(wdir / (k + ".pkl"), "wb"))
    argv = ["--no_cfg", "--max_epochs", "1", "--batch_size", "2", "--num_workers", "0", "--seq_per_img", "1",
            "--input_dic", o.input_dic, "--input_json", o.input_json, "--grd_reference", o.grd_reference, "--proposal_h5", o.proposal_h5,
            "--feature_root", o.feature_root, "--seg_feature_root", o.seg_feature_root, "--glove_path", o.glove_path,
            "--vg_vocab_file", o.vg_vocab_file, "--detectron_weights_dir", str(wdir), "--exclude_bgd_det",
            "--num_sampled_frm", "2", "--num_prop_per_frm", "5", "--t_attn_size", "6", "--att_feat_size", "24", "--vis_encoding_size", "24",
            "--rnn_size", "32", "--att_hid_size", "16", "--input_encoding_size", "16", "--seq_length", "8",
            "--train_split", "training", "--val_split", "validation", "--tensorboard", "0", "--disp_interval", "100",
            "--checkpoint_path", str(tmp_path) + "/", "--exp_name", "disk", "--learning_rate", "0.001",
            "--results_dir", str(tmp_path / "results"), "--id", "g1"]
    assert cvc_main.main(argv + ["--val_metrics", "device", "--eval_obj_grounding"]) == 0
    tr = cvc_main.LAST_TRAINER
    opts = tr.opts
    history = pickle.load(open(tmp_path / "disk" / "histories_g1.pkl", "rb"))["val_result_history"][0]
    assert set(history) == set(metrics.KEYS) | set(metrics.GROUNDING_KEYS)                 # written to the history like the other scores

    word_cls = utils.word_class_table(opts).numpy()

    def scores_and_file(label):
        """eval with both switches against the restatement on a re-decode of the same batches (1e-12), then the grounding file
        against the one the host route writes with the device metrics off; -> (lang_stats, object words)"""
        tr.device_metrics = True
        stats = tr.eval(0)
        assert set(stats) == set(metrics.KEYS) | set(metrics.GROUNDING_KEYS)
        dev_file = json.load(open(tr.attn_file))
        table, words = None, 0
        with torch.no_grad():
            for b in DevicePrefetcher(tr.val_loader, lambda raw: tr._prepare(raw, False), tr.device):
                seq, att, _ = tr._call(b, True)
                ref = R.score_batch(seq.cpu().numpy(), att.float().cpu().numpy(), b["ppls"].cpu().numpy(), b["gt_bboxs"].cpu().numpy(),
                                    b["num"][:, 2].cpu().numpy(), word_cls, opts.num_sampled_frm, opts.num_prop_per_frm, len(opts.itod),
                                    table=table)
                table = ref["table"]
                words += int((ref["pick"][:, :, 0] >= 0).sum())
        want = R.result(table)
        print(f"[grounding eval] {label}: object words {words}, table column sums {table.sum(0).tolist()}")
        for k in metrics.GROUNDING_KEYS:
            print(f"[grounding eval] {label}: {k}: eval {stats[k]!r} restatement {want[k]!r}")
        for k in metrics.GROUNDING_KEYS:
            assert abs(stats[k] - want[k]) <= 1e-12, k
        assert table[:, 0].sum() > 0                                                        # the split has annotated boxes
        tr.device_metrics = False
        alone = tr.eval(0)
        assert set(alone) == set()                                                          # --eval_obj_grounding alone: no score, as before
        host_file = json.load(open(tr.attn_file))
        assert dev_file == host_file and dev_file["eval_mode"] == "gen"
        entries = [e for segs in host_file["results"].values() for e in segs.values()]
        assert entries and all(set(e) == {"clss", "idx_in_sent", "bbox_for_all_frames"} for e in entries)
        assert sum(len(e["clss"]) for e in entries) == words
        assert all(len(bx) == 2 and all(len(f) == 4 for f in bx) for e in entries for bx in e["bbox_for_all_frames"])
        print(f"[grounding eval] {label}: {len(entries)} segments, {words} object words in the file")
        return stats, words

    # ---- the epoch's weights (they have not moved since the epoch's eval: the history's scores come back)
    stats, _ = scores_and_file("after the epoch")
    assert all(stats[k] == history[k] for k in metrics.GROUNDING_KEYS)

    # ---- three optimizer steps leave a checkpoint that may name no object at all: the same checks with the vocabulary head tilted
    # towards the object words every segment of the fixture has boxes of, so that the captions are full of them (a class many times
    # in a caption, no end mark) and the hit tests run
    core = getattr(tr.model, "module", tr.model)
    with torch.no_grad():
        core.logit.bias[[int(opts.wtoi[w]) for w in ("man", "dog", "woman")]] += 2.0
    core.invalidate_decode_cache()
    stats, words = scores_and_file("tilted head")
    assert words >= 4

    # ---- --val_metrics device alone: the six caption scores, no grounding key, no grounding file
    tr.device_metrics, opts.eval_obj_grounding = True, False
    assert set(tr.eval(0)) == set(metrics.KEYS) and tr.attn_file is None
