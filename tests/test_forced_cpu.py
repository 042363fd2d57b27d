"""Teacher-forced decode, the parts that need no GPU: the block's reference (tests/forced_ref.py) against brute-force definitions, the
pick / hit / accuracy arithmetic of Trainer.ground_gt against a numpy restatement on the CPU oracle's training pass, the JSON
layout, cvc.score's argument parsing, the block's declarations and the engine's refusals."""
import argparse
import collections
import json
import os
import re

import numpy as np
import pytest
import torch

from cvc import synth
import forced_ref as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the reference against brute force
@pytest.mark.parametrize("M,V,nparts", [(7, 33, 1), (5, 500, 3)])
def test_reference_vs_brute_force(M, V, nparts):
    g = torch.Generator().manual_seed(V + nparts)
    parts = torch.randn(nparts, M, V, generator=g)
    bias = torch.randn(V, generator=g)
    parts[:, 1, 4] = parts[:, 1, 9]                       # exact ties around the given word
    parts[:, 2, 12] = parts[:, 2, 9]
    bias[4] = bias[12] = bias[9]
    words = torch.randint(0, V, (M,), generator=g)
    words[1] = words[2] = 9
    words[3], words[4] = V, -1
    z = FR.finished(parts, bias)
    # the slab order: ((p0 + p1) + p2) + bias in fp32
    acc = parts[0].numpy().copy()
    for k in range(1, nparts):
        acc = (acc + parts[k].numpy()).astype(np.float32)
    assert np.array_equal(z.numpy(), (acc + bias.numpy()).astype(np.float32))
    lp, rk = FR.forced_select(z, words.numpy())
    lsm = torch.log_softmax(z.double(), 1).numpy()
    for r in range(M):
        w = int(words[r])
        if not 0 <= w < V:
            assert np.isnan(lp[r]) and rk[r] == -1
            continue
        # rank = the word's position when the row is sorted by falling logit, lower index first among equals
        order = sorted(range(V), key=lambda v: (-float(z[r, v]), v))
        assert rk[r] == order.index(w)
        assert abs(lp[r] - lsm[r, w]) < 1e-12
    assert rk[1] == int((z[1] > z[1, 9]).sum()) + 1 and rk[2] == int((z[2] > z[2, 9]).sum())
    # NaN logits compare false; the log-prob of such a row is NaN
    z[0, (int(words[0]) + 1) % V] = float("nan")
    lp2, rk2 = FR.forced_select(z, words.numpy())
    assert np.isnan(lp2[0]) and 0 <= rk2[0] <= rk[0]
    # the band of ranks a tolerance allows contains the exact rank; without a tolerance it is [#greater, #greater-or-equal]
    for r in (1, 2):
        lo, hi = FR.rank_band(lsm[r], 9, 1e-4)
        assert lo <= rk[r] <= hi
        others = np.delete(lsm[r], 9)
        assert FR.rank_band(lsm[r], 9, 0.0) == (int((others > lsm[r, 9]).sum()), int((others >= lsm[r, 9]).sum()))


# ------------------------------------------------------------------ ground_gt's arithmetic on the oracle's training pass
@pytest.mark.parametrize("name,seed", [("tiny", 4321), ("tiny", 99), ("cfg1", 4321), ("cfg1", 99)])
def test_ground_picks_and_accuracy_vs_numpy_on_the_oracle(name, seed):
    from oracle import ref_cpu as O
    from cvc.trainer import ground_picks, ground_accuracy
    d = synth.CONFIGS[name]
    sd, f_np, b_np = synth.hot_path_state_dict(d, seed), synth.clip_features(d, seed), synth.label_glue_batch(d, seed)
    c = {}
    with torch.no_grad():
        O.cyclical_forward(O.to_torch(sd), O.to_torch(f_np), O.to_torch(b_np), T=d.T, vocab_size=d.V, train_decoder_only=True, collect=c)
    fmo, labels = c["frm_mask_output"], c["roi_labels"]
    cls = b_np["input_seq"][:, 0, 1:d.T + 1, 0] - d.V
    annotated = (~b_np["box_mask"][:, 0, :, 1:d.T + 1]).any(1)
    hits = {}
    for key in ("att2_weights", "ground_weights"):
        w = c[key]
        pick, hit = ground_picks(w, fmo, labels)
        pick_n, hit_n = FR.ground_picks(w.numpy(), fmo.numpy(), labels.numpy())
        assert np.array_equal(pick.numpy(), pick_n) and np.array_equal(hit.numpy(), hit_n)
        hits[key] = hit_n
        # the margin of every pick inside its frame: far over the GPU tests' tolerance, so those compare picks exactly
        free = ~fmo.numpy()[:, :, 1:]
        vals = np.where(free, w.numpy(), -np.inf)
        top2 = -np.partition(-vals, 1, axis=2)[:, :, :2]
        two = free.sum(2) >= 2
        with np.errstate(invalid="ignore"):              # (words with fewer than two unmasked proposals: -inf - -inf, not counted)
            gap = (top2[:, :, 0] - top2[:, :, 1])[two]
        print(f"[ground_gt] {name} seed {seed} {key}: smallest top-2 gap among unmasked proposals {gap.min():.3e} over {two.sum()} words")
        assert gap.min() > 100 * 1e-4
    words = [(int(cls[b, t]), bool(hits["att2_weights"][b, t]), bool(hits["ground_weights"][b, t]))
             for b in range(d.B) for t in range(d.T) if cls[b, t] >= 1 and annotated[b, t]]
    stats = ground_accuracy(words)
    for key, name_ in (("att2_weights", "att"), ("ground_weights", "grd")):
        acc, per_cls, n = FR.ground_accuracy(hits[key], b_np["input_seq"], b_np["box_mask"], d.V)
        assert n == stats["obj_words"] > 0
        assert stats["box_accu_" + name_] == pytest.approx(acc, abs=1e-12) and 0.0 <= acc <= 1.0
        assert stats["box_accu_%s_per_cls" % name_] == pytest.approx(per_cls, abs=1e-12)
    # a word whose proposals are all frame-masked is a miss with pick -1; ties go to the lowest index
    w = torch.zeros(1, 2, 4)
    fm = torch.tensor([[[False, True, True, True, True], [False, True, False, False, True]]])
    lab = torch.ones(1, 2, 4, dtype=torch.bool)
    pick, hit = ground_picks(w, fm, lab)
    assert pick.tolist() == [[-1, 1]] and hit.tolist() == [[False, True]]
    assert ground_accuracy([]) == {"obj_words": 0, "box_accu_att": 0.0, "box_accu_att_per_cls": 0.0, "box_accu_grd": 0.0,
                                   "box_accu_grd_per_cls": 0.0}
    assert ground_accuracy([(1, True, False), (1, False, False), (2, True, True)]) == {
        "obj_words": 3, "box_accu_att": 2 / 3, "box_accu_att_per_cls": 0.75, "box_accu_grd": 1 / 3, "box_accu_grd_per_cls": 0.5}


# ------------------------------------------------------------------ files
def test_grounding_json_layout_and_the_generated_sentences_file_is_unchanged(tmp_path):
    from cvc.trainer import Trainer, write_grounding_json
    o = argparse.Namespace(results_dir=str(tmp_path), val_split="validation", id="x1", num_sampled_frm=2, num_prop_per_frm=3,
                           wtol={"w2": "w2", "w3": "w3", "w4": "w4"}, wtod={"w3": 2}, itow={"2": "w2", "3": "w3", "4": "w4"},
                           itod={2: "cls2"})
    grd = {"v_a": {"0": {"clss": ["cls2"], "idx_in_sent": [1], "bbox_for_all_frames": [[[1.0, 2.0, 3.0, 4.0]] * 2]}}}
    p_gen = write_grounding_json(grd, o)
    want = json.dumps({'results': grd, 'eval_mode': 'gen', 'external_data': {
        'used': True, 'details': 'Object detector pre-trained on Visual Genome on object detection task.'}})
    assert os.path.basename(p_gen) == "attn-gen-sent-results-validation-x1.json" and open(p_gen).read() == want
    p_att = write_grounding_json(grd, o, stem="attn-gt-sent-results", eval_mode="GT")
    p_grd = write_grounding_json(grd, o, stem="grd-gt-sent-results", eval_mode="GT")
    assert os.path.basename(p_att) == "attn-gt-sent-results-validation-x1.json"
    assert os.path.basename(p_grd) == "grd-gt-sent-results-validation-x1.json"
    got = json.load(open(p_grd))
    assert got["eval_mode"] == "GT" and got["results"] == grd and set(got) == {"results", "eval_mode", "external_data"}
    # the box gather that _collect_grounding and ground_gt share: the generated sentences' output as before (restated here)
    tr = object.__new__(Trainer)
    tr.opts = o
    g = torch.Generator().manual_seed(5)
    B, T, N = 2, 3, 6
    ppls, att = torch.rand(B, N, 7, generator=g), torch.rand(B, T, N, generator=g)
    seq = torch.tensor([[3, 2, 3], [4, 3, 0]])
    out = collections.defaultdict(dict)
    tr._collect_grounding(dict(ppls=ppls, seg_id=["v_a_segment_00", "v_b_segment_03"]), seq, att, out)
    ind = torch.max(att.view(B, T, 2, 3), dim=-1)[1]
    boxes = torch.gather(ppls.view(-1, 2, 3, 7).permute(0, 2, 1, 3).contiguous(), 1, ind.unsqueeze(-1).expand(B, T, 2, 7))[..., :4].tolist()
    assert out == {"v_a": {"0": {"clss": ["cls2", "cls2"], "idx_in_sent": [0, 2], "bbox_for_all_frames": [boxes[0][0], boxes[0][2]]}},
                   "v_b": {"3": {"clss": ["cls2"], "idx_in_sent": [1], "bbox_for_all_frames": [boxes[1][1]]}}}
    assert torch.equal(tr._frame_boxes(ppls, att)[..., :4], torch.tensor(boxes))


def test_score_cli_parsing():
    from cvc import score as cvc_score
    from cvc import opts as cvc_opts
    own, rest = cvc_score.parse(["--resume", "True", "--ground_gt", "--id", "r1"])
    assert own.ground_gt is True and rest == ["--resume", "True", "--id", "r1"]
    own, rest = cvc_score.parse(["--resume", "True"])
    assert own.ground_gt is False and rest == ["--resume", "True"]
    # the module's flag is its own: cvc.opts does not know it (tests/golden/opts_namespaces.json pins that namespace)
    assert "ground_gt" not in vars(cvc_opts.build_parser().parse_args([]))
    assert "eval_obj_grounding_gt" in vars(cvc_opts.build_parser().parse_args([]))


# ------------------------------------------------------------------ the block's declarations, the engine's refusals
def test_forced_block_is_declared_as_a_building_block():
    from cvc import hip
    name = "cvc_forced_select_parts"
    blocks_h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cvc_hip_blocks.h")).read(), flags=re.S)
    core_h = open(os.path.join(ROOT, "include", "cvc_hip.h")).read()
    m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, blocks_h)
    assert m and name not in core_h                       # a building block, not an exported symbol
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 11 and params[-1].startswith("cvc_stream_t")
    assert name in hip.BLOCKS and len(hip.SIGNATURES[name]) == 11
    assert hip.SIGNATURES[name][2] is hip._LL and hip.SIGNATURES[name][1] is hip._I
    table = open(os.path.join(ROOT, "cyclical-visual-captioning_amd", "csrc", "blocks.hip")).read()
    assert "CVC_B(%s)" % name in table
    assert os.path.isfile(os.path.join(ROOT, "cyclical-visual-captioning_amd", "csrc", "forced.hip"))


@pytest.mark.parametrize("kw", [dict(beam=2), dict(temperature=0.7), dict(gsk=True), dict(gate_ksplit=True), dict(lang_ksx=True),
                                dict(forced_n=-1), dict(forced_n=1.5), dict(forced_n=2, weights_dtype="bf16"),
                                dict(top_k=3), dict(sample_n=2)])
def test_forced_engine_refusals_come_before_any_tensor_is_touched(kw):
    """weights and features are never looked at: the refusal is raised from the arguments alone"""
    from cvc.decode import DecodeEngine
    kw.setdefault("forced_n", 1)
    with pytest.raises(RuntimeError):
        DecodeEngine(None, None, 4, synth.UNK_IDX, **kw)
