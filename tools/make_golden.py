#!/usr/bin/env python3
"""Generate tests/golden/*.npz by running the REFERENCE itself (imported from
/root/reference, build container only -- the reference never ships to the GPU box).

  python tools/make_golden.py            # writes tests/golden/{g1_tiny,g2_cfg1,g3_shards}.npz

Fixtures are data only: seeded inputs (or the seed that regenerates them through
cvc.synth) and the outputs/gradients the reference produced.  SURVEY.md section 8(c).
"""
from __future__ import annotations

import argparse
import os
import sys
import types
from collections import OrderedDict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/anet-video-captioning"
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "cyclical-visual-captioning_amd"))
sys.path.insert(0, REF)
_tb = types.ModuleType("tensorboardX")
_tb.SummaryWriter = object
sys.modules["tensorboardX"] = _tb

import torch.nn as nn  # noqa: E402
from cvc import synth  # noqa: E402
from model.modules import AdditiveSoftAttention, SoftAttention  # noqa: E402  (reference)
from model.decoder_core import TopDownDecoderCore, AttenedDecoderCore  # noqa: E402
from model.localizer_core import LocalizerNoLSTMCore  # noqa: E402
from model.captioner import DecodeAndGroundCaptionerGVDROI  # noqa: E402

torch.manual_seed(0)
torch.set_num_threads(4)


def make_opts(d: synth.Dims, **over):
    o = argparse.Namespace(
        vocab_size=d.V, itow={str(i): "w%d" % i for i in range(d.V)}, wtoi={"UNK": synth.UNK_IDX},
        seq_length=d.T, seq_per_img=1, rnn_size=d.R, input_encoding_size=d.E, att_hid_size=d.A,
        drop_prob_lm=0.5, softattn_type="additive", softmax_temp=1.0, localizer_softmax_temp=1.0,
        global_img_in_attn_lstm=1, embedding_vocab_plus_1=False, train_decoder_only=False)
    for k, v in over.items():
        setattr(o, k, v)
    return o


class FeatureStub(nn.Module):
    """Stands in for RegionalFeatureExtractorGVD (captioner.py:31-34 allows roi_extractor=):
    returns pre-projected features in the order of backbone.py:350-351."""

    def __init__(self, d, feats):
        super().__init__()
        self.vis_embed = nn.Sequential(nn.Embedding(d.DET + 1, d.G), nn.ReLU(), nn.Dropout(0.5))
        self.vis_classifiers_bias = nn.Parameter(torch.zeros(d.DET + 1))
        self.feats = feats

    def forward(self, *a, **k):
        f = self.feats
        return (f["fc_feats"], f["conv_feats"], f["p_conv_feats"], f["pool_feats"], f["p_pool_feats"],
                f["g_pool_feats"], f["pnt_mask"], None, None, torch.zeros(()))


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def build_reference_model(d, sd_np, feats_t, **opt_over):
    opts = make_opts(d, **opt_over)
    model = DecodeAndGroundCaptionerGVDROI(opts, roi_extractor=FeatureStub(d, feats_t))
    model.device = torch.device("cpu")
    missing, unexpected = model.load_state_dict({k: t(v) for k, v in sd_np.items()}, strict=False)
    assert not unexpected, unexpected
    assert not missing, missing
    model.eval()
    return model


def model_call(model, batch_t, feats_t, lang_eval=False):
    B = feats_t["fc_feats"].size(0)
    segs = torch.zeros(B, 1, 1)
    return model(segs, batch_t["input_seq"], batch_t["gt_seq"], batch_t["num"], batch_t["proposals"],
                 batch_t["gt_bboxs"], batch_t["box_mask"], torch.zeros(B, 1, 1), batch_t["frm_mask"],
                 batch_t["sample_idx"], feats_t["pnt_mask"], lang_eval)


FEAT_GRAD_KEYS = ("fc_feats", "conv_feats", "p_conv_feats", "pool_feats", "p_pool_feats", "g_pool_feats")


def grads_of(model, feats_t, loss):
    for p in model.parameters():
        p.grad = None
    for k in FEAT_GRAD_KEYS:
        feats_t[k].grad = None
    loss.backward()
    g = OrderedDict()
    for n, p in model.named_parameters():
        g["grad." + n] = None if p.grad is None else p.grad.detach().clone().numpy()
    for k in FEAT_GRAD_KEYS:
        gg = feats_t[k].grad
        g["grad.in." + k] = None if gg is None else gg.detach().clone().numpy()
    return g


def feats_to_torch(feats_np, requires_grad):
    ft = {k: t(v) for k, v in feats_np.items()}
    if requires_grad:
        for k in FEAT_GRAD_KEYS:
            ft[k].requires_grad_(True)
    return ft


def put(out, prefix, d):
    for k, v in d.items():
        if v is None:
            out[prefix + k + ".is_none"] = np.asarray(1)
        else:
            out[prefix + k] = v.detach().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def loss_mix(losses, xe=0.5, w_att2=0.0, w_cls=0.0, cons=0.5):
    lm, att2, _g, cls = [x.mean() for x in losses[:4]]
    loss = xe * lm + w_att2 * att2 + w_cls * cls
    if len(losses) > 4:
        loss = loss + cons * losses[4].mean()
    return loss


# ------------------------------------------------------------------------------------ G1
def g1_tiny(path):
    d = synth.CONFIGS["tiny"]
    seed = 1234
    sd = synth.hot_path_state_dict(d, seed)
    feats_np = synth.clip_features(d, seed, full_mask_clip=2)
    batch_np = synth.label_glue_batch(d, seed)
    out = OrderedDict()
    out["meta.seed"] = np.asarray(seed)
    put(out, "sd.", sd)
    put(out, "feats.", feats_np)
    put(out, "batch.", batch_np)

    # ---- module-level vectors (a1, a2, a3, a5, a6) with non-trivial state
    B, N, F, R, A, E = d.B, d.N, d.F, d.R, d.A, d.E
    h = t(synth.normal((B, R), seed, "unit.h") * 0.5)
    emb = t(np.maximum(synth.normal((B, E), seed, "unit.emb"), 0))
    st_h = t(synth.normal((2, B, R), seed, "unit.state_h") * 0.5)
    st_c = t(synth.normal((2, B, R), seed, "unit.state_c") * 0.5)
    fmask = t(synth.uniform((B, N), seed, "unit.fmask") < 0.4)
    put(out, "unit.", dict(h=h, emb=emb, state_h=st_h, state_c=st_c, fmask=fmask))
    ft = feats_to_torch(feats_np, False)
    mask = ft["pnt_mask"][:, 1:]
    opts = make_opts(d)

    add = AdditiveSoftAttention(R, A)
    add.load_state_dict({k.split("soft_attn.")[1]: t(v) for k, v in sd.items() if k.startswith("decoder_core.soft_attn.")})
    ctx, a, fm = add(h, ft["p_pool_feats"], context=ft["pool_feats"], mask=mask, proposal_frame_mask=fmask)
    put(out, "a1.regions.", dict(ctx=ctx, attn=a, fm=fm))
    ctx, a, fm = add(h, ft["p_conv_feats"], context=ft["conv_feats"])
    put(out, "a1.frames.", dict(ctx=ctx, attn=a))
    ctx, a, fm = add(h, ft["p_pool_feats"], mask=mask)  # context=None -> weighted proj_context
    put(out, "a1.noctx.", dict(ctx=ctx, attn=a))

    for temp in (1.0, 2.5):
        dot = SoftAttention(E, A, temp=temp)
        dot.load_state_dict({k.split("soft_attn.")[1]: t(v) for k, v in sd.items() if k.startswith("localizer_core.soft_attn.")})
        ctx, a, fm = dot(emb, ft["p_pool_feats"], context=ft["pool_feats"], mask=mask, proposal_frame_mask=fmask)
        put(out, "a2.temp%g." % temp, dict(ctx=ctx, attn=a, fm=fm))

    core = TopDownDecoderCore(opts)
    core.load_state_dict({k[len("decoder_core."):]: t(v) for k, v in sd.items() if k.startswith("decoder_core.")})
    core.eval()
    o, st, ra, fma, wp = core(emb, ft["fc_feats"], ft["conv_feats"], ft["p_conv_feats"], ft["pool_feats"],
                              ft["p_pool_feats"], mask, (st_h, st_c), proposal_frame_mask=fmask)
    put(out, "a3.", dict(out=o, h=st[0], c=st[1], roi_attn=ra, fm=fma, ctx_r=wp))
    # (global_img_in_attn_lstm=0 cannot run in the reference: the cell is always built with
    #  E+2R inputs, decoder_core.py:14, so the 2-way concat of :48 shape-mismatches.)
    rec = AttenedDecoderCore(opts, core.att_lstm, core.lang_lstm)
    rec.eval()
    lp = t(synth.normal((B, R), seed, "unit.loc_pool"))
    lc = t(synth.normal((B, R), seed, "unit.loc_conv"))
    put(out, "unit.", dict(loc_pool=lp, loc_conv=lc))
    o, st = rec(emb, ft["fc_feats"], lp, lc, (st_h, st_c))
    put(out, "a5.", dict(out=o, h=st[0], c=st[1]))

    loc = LocalizerNoLSTMCore(opts)
    loc.load_state_dict({k[len("localizer_core."):]: t(v) for k, v in sd.items() if k.startswith("localizer_core.")})
    a, b_, c_, _ = loc(emb, ft["fc_feats"], ft["conv_feats"], ft["p_conv_feats"], ft["pool_feats"],
                       ft["p_pool_feats"], mask, None, None, proposal_frame_mask=fmask)
    put(out, "a6.", dict(loc_pool=a, loc_conv=b_, prob=c_))

    # ---- a8 greedy sample, with the per-step log-probs captured by a hook on logit
    ft = feats_to_torch(feats_np, False)
    bt = {k: t(v) for k, v in batch_np.items()}
    model = build_reference_model(d, sd, ft)
    logits = []
    hk = model.logit.register_forward_hook(lambda m, i, o: logits.append(o.detach().clone()))
    with torch.no_grad():
        seq, att2, _ = model_call(model, bt, ft, True)
    hk.remove()
    put(out, "a8.", dict(seq=seq, att2_weights=att2, logp=torch.log_softmax(torch.stack(logits, 1), 2)))

    # ---- a9 cyclical forward + grads (eval mode); a10 ground weights via hook
    for name, over, mix in (("a9.cyc.", dict(), dict()),
                            ("a9.sup.", dict(), dict(w_att2=0.05)),
                            ("a9.dec.", dict(train_decoder_only=True), dict(cons=0.0))):
        ft = feats_to_torch(feats_np, True)
        model = build_reference_model(d, sd, ft, **over)
        grabbed = {}
        orig = model._grounder

        def spy(xt, att_feats, mask, bias=None, min_value=-1e8, _o=orig, _g=grabbed):
            r = _o(xt, att_feats, mask, bias, min_value)
            _g["ground_weights"] = r.detach().clone()
            return r
        model._grounder = spy
        losses = model_call(model, bt, ft, False)
        put(out, name, {"loss%d" % i: l for i, l in enumerate(losses)})
        put(out, name, grabbed)
        loss = loss_mix(losses, **mix)
        put(out, name, dict(total=loss))
        put(out, name, grads_of(model, ft, loss))
    np.savez_compressed(path, **out)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1024))


# ------------------------------------------------------------------------------------ G2
def g2_cfg1(path):
    d = synth.CONFIGS["cfg1"]
    seed = 1235
    sd = synth.hot_path_state_dict(d, seed)
    feats_np = synth.clip_features(d, seed)
    batch_np = synth.label_glue_batch(d, seed)
    out = OrderedDict()
    out["meta.seed"] = np.asarray(seed)
    ft = feats_to_torch(feats_np, False)
    bt = {k: t(v) for k, v in batch_np.items()}
    model = build_reference_model(d, sd, ft)
    logits = []
    hk = model.logit.register_forward_hook(lambda m, i, o: logits.append(o.detach().clone()))
    with torch.no_grad():
        seq, att2, _ = model_call(model, bt, ft, True)
    hk.remove()
    logp = torch.log_softmax(torch.stack(logits, 1), 2)
    top8 = torch.topk(logp, 8, dim=2)
    put(out, "a8.", dict(seq=seq, att2_weights=att2, top8_logp=top8[0], top8_idx=top8[1]))

    ft = feats_to_torch(feats_np, True)
    model = build_reference_model(d, sd, ft)
    losses = model_call(model, bt, ft, False)
    put(out, "a9.cyc.", {"loss%d" % i: l for i, l in enumerate(losses)})
    loss = loss_mix(losses)
    g = grads_of(model, ft, loss)
    for k, v in g.items():
        if v is None:
            out["a9.cyc." + k + ".is_none"] = np.asarray(1)
            continue
        flat = v.reshape(-1)
        idx = synth.randint((16,), seed, "sample." + k, 0, flat.size)
        out["a9.cyc." + k + ".norm"] = np.asarray(np.sqrt((flat.astype(np.float64) ** 2).sum()))
        out["a9.cyc." + k + ".idx"] = idx
        out["a9.cyc." + k + ".val"] = flat[idx]
    np.savez_compressed(path, **out)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1024))


# ------------------------------------------------------------------------------------ G3
def g3_shards(path):
    """Per-shard losses/grads for a 4-clip tiny batch split 2 ways: the mean over shards is what a
    G-way data-parallel step must all-reduce to (DataParallel semantics)."""
    import dataclasses
    d = dataclasses.replace(synth.CONFIGS["tiny"], B=4)
    seed = 1236
    sd = synth.hot_path_state_dict(d, seed)
    feats_np = synth.clip_features(d, seed)
    batch_np = synth.label_glue_batch(d, seed)
    out = OrderedDict()
    out["meta.seed"] = np.asarray(seed)
    shard_grads = []
    for s, sl in enumerate((slice(0, 2), slice(2, 4), slice(0, 4))):
        name = "shard%d." % s if s < 2 else "full."
        ft = feats_to_torch({k: v[sl] for k, v in feats_np.items()}, True)
        bt = {k: t(v[sl]) for k, v in batch_np.items()}
        model = build_reference_model(d, sd, ft)
        losses = model_call(model, bt, ft, False)
        put(out, name, {"loss%d" % i: l for i, l in enumerate(losses)})
        g = grads_of(model, ft, loss_mix(losses))
        g = {k: v for k, v in g.items() if not k.startswith("grad.in.")}
        put(out, name, g)
        if s < 2:
            shard_grads.append(g)
    mean = {k: (None if shard_grads[0][k] is None else (shard_grads[0][k] + shard_grads[1][k]) / 2)
            for k in shard_grads[0]}
    put(out, "mean.", mean)
    np.savez_compressed(path, **out)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1024))


# ------------------------------------------------------------------------------------ G4 (config surface)
def g4_config_surface(path):
    """state_dict key/shape list of the reference model and the routing performed by its stage-2
    warm-start loader (cycle_utils.py:30-101), captured by tagging every checkpoint tensor."""
    import json
    import pickle
    import tempfile
    from cycle_utils import resume_decoder_roiextractor
    d = synth.CONFIGS["tiny"]
    sd = synth.hot_path_state_dict(d, 1)
    ft = feats_to_torch(synth.clip_features(d, 1), False)
    model = build_reference_model(d, sd, ft)
    keys = {k: list(v.shape) for k, v in model.state_dict().items()}
    # tag: every checkpoint tensor is filled with its own ordinal
    ckpt = OrderedDict()
    for i, (k, v) in enumerate(model.state_dict().items()):
        ckpt[k] = torch.full_like(v, float(i + 1)) if v.dtype.is_floating_point else v.clone()
    order = list(ckpt.keys())
    tmp = tempfile.mkdtemp()
    os.makedirs(os.path.join(tmp, "baseline"))
    torch.save(ckpt, os.path.join(tmp, "baseline", "model-best.pth"))
    with open(os.path.join(tmp, "baseline", "infos_-best.pkl"), "wb") as f:
        pickle.dump({"epoch": 7}, f)
    opts = make_opts(d, checkpoint_dir=tmp + "/", id="", resume_embed=1, resume_logit=1, resume_roi_extractor=1)
    decoder = TopDownDecoderCore(opts)
    embed = nn.Sequential(nn.Embedding(d.V, d.E), nn.ReLU(), nn.Dropout(0.5))
    logit = nn.Linear(d.R, d.V)
    roi = FeatureStub(d, ft)
    resume_decoder_roiextractor(opts, "baseline", decoder, embed, logit, roi)
    routing = {}
    for name, mod in (("decoder_core", decoder), ("embed", embed), ("logit", logit), ("roi_feat_extractor", roi)):
        for k, v in mod.state_dict().items():
            routing[name + "." + k] = order[int(round(float(v.reshape(-1)[0]))) - 1]
    json.dump({"state_dict": keys, "warm_start_routing": routing, "start_epoch": opts.start_epoch},
              open(path, "w"), indent=1, sort_keys=True)
    print("wrote", path)


# ------------------------------------------------------------------------------------ G5 (once-per-clip encoder)
def encoder_opts(d, tables, seq_per_img, **over):
    o = make_opts(d, seq_per_img=seq_per_img, test_mode=False, enable_BUTD=False, att_input_mode="both",
                  num_sampled_frm=4, finetune_cnn=False, att_feat_size=d.G, fc_feat_size=synth.SEG_FEAT_DIM,
                  detect_size=d.DET, vis_encoding_size=d.G, t_attn_size=d.F, second_drop_prob=0.3,
                  att_model="topdown", t_attn_mode="bigru", itod={i + 1: "d%d" % i for i in range(d.DET)},
                  vg_cls=["vg%d" % i for i in range(tables["glove_vg_cls"].shape[0])],
                  glove_clss=t(tables["glove_clss"]), glove_vg_cls=t(tables["glove_vg_cls"]))
    for k, v in over.items():
        setattr(o, k, v)
    return o


def build_reference_encoder(d, tables, seed, seq_per_img, **over):
    import pickle
    import tempfile
    from model.backbone import RegionalFeatureExtractorGVD
    tmp = tempfile.mkdtemp()
    os.makedirs(os.path.join(tmp, "data", "detectron_weights"))
    for k in ("fc7_w", "fc7_b", "cls_score_w", "cls_score_b"):
        with open(os.path.join(tmp, "data", "detectron_weights", k + ".pkl"), "wb") as f:
            pickle.dump(tables[k], f)
    cwd = os.getcwd()
    os.chdir(tmp)
    try:
        enc = RegionalFeatureExtractorGVD(encoder_opts(d, tables, seq_per_img, **over))
    finally:
        os.chdir(cwd)
    enc.device = torch.device("cpu")
    ctor = {k: v.detach().clone() for k, v in enc.state_dict().items() if k in synth.ENCODER_CTOR_KEYS}
    sd = {k: (ctor[k] if k in ctor else t(synth.encoder_fill(k, v.shape, seed))) for k, v in enc.state_dict().items()}
    enc.load_state_dict(sd)
    enc.eval()
    return enc, ctor


ENC_OUT = ("fc_feats", "conv_feats", "p_conv_feats", "pool_feats", "p_pool_feats", "g_pool_feats", "pnt_mask",
           "overlaps_expanded")


def encoder_probe_loss(outs):
    fc, conv, pconv, pool, ppool, g = outs[:6]
    return (0.01 * fc.sum() + conv.pow(2).mean() + pconv.mean() + pool.pow(2).mean() + ppool.pow(2).mean()
            + g.pow(2).mean() + outs[9].sum())


def g5_encoder(path):
    import misc.utils as ref_utils
    d = synth.CONFIGS["tiny"]
    seed = 1237
    tables = synth.detectron_tables(d, seed)
    inp = synth.encoder_inputs(d, seed)
    out = OrderedDict()
    out["meta.seed"] = np.asarray(seed)
    bt = {k: t(v) for k, v in inp.items()}
    overlaps = ref_utils.bbox_overlaps(bt["proposals"], bt["gt_bboxs"],
                                       (bt["frm_mask"] | bt["pnt_mask_in"][:, 1:].unsqueeze(-1)))
    out["overlaps"] = overlaps.numpy()
    for name, S, over in (("s2.", 2, {}), ("s1test.", 1, dict(test_mode=True))):
        enc, ctor = build_reference_encoder(d, tables, seed, S, **over)
        put(out, name + "ctor.", ctor)
        res = enc(bt["segs_feat"], bt["proposals"], bt["num"], bt["box_mask"], bt["region_feats"], bt["gt_bboxs"],
                  overlaps, bt["sample_idx"])
        put(out, name + "out.", dict(zip(ENC_OUT, res[:8])))
        out[name + "out.cls_loss"] = res[9].detach().numpy()
        if not over:
            out[name + "out.cls_pred"] = res[8].numpy()
            encoder_probe_loss(res).backward()
            for n, p in enc.named_parameters():
                if p.grad is None:
                    out[name + "grad." + n + ".is_none"] = np.asarray(1)
                else:
                    out[name + "grad." + n + ".norm"] = np.asarray(p.grad.double().norm().item())
    # ---- end to end: the reference captioner on top of the reference encoder (seq_per_img 1)
    sd = synth.hot_path_state_dict(d, seed)
    enc, _ = build_reference_encoder(d, tables, seed, 1)
    model = DecodeAndGroundCaptionerGVDROI(make_opts(d), roi_extractor=enc)
    model.device = torch.device("cpu")
    dec = {k: t(v) for k, v in sd.items() if not k.startswith("roi_feat_extractor.")}
    dec.update({"roi_feat_extractor." + k: v for k, v in enc.state_dict().items()})
    model.load_state_dict(dec)
    model.eval()

    def call(lang_eval):
        return model(bt["segs_feat"], bt["input_seq"], bt["gt_seq"], bt["num"], bt["proposals"], bt["gt_bboxs"],
                     bt["box_mask"], bt["region_feats"], bt["frm_mask"], bt["sample_idx"], bt["pnt_mask_in"], lang_eval)
    with torch.no_grad():
        seq, att2, _ = call(True)
    put(out, "e2e.", dict(seq=seq, att2_weights=att2))
    losses = call(False)
    put(out, "e2e.", {"loss%d" % i: l for i, l in enumerate(losses)})
    loss = loss_mix(losses, w_att2=0.05, w_cls=0.1)
    for p in model.parameters():
        p.grad = None
    loss.backward()
    for n, p in model.named_parameters():
        if p.grad is None:
            out["e2e.grad." + n + ".is_none"] = np.asarray(1)
        else:
            out["e2e.grad." + n + ".norm"] = np.asarray(p.grad.double().norm().item())
    np.savez_compressed(path, **out)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1024))


WIDE = dict(B=5, N=20, F=9, R=256, A=64, E=32, K=3)      # encoder widths at which the HIP forms run (GRU hidden size 128)


def g8_encoder_wide(path):
    """The reference encoder's eval forward at a width the build's HIP kernels take (rnn_size 256 -> GRU hidden size 128: the
    persistent recurrence; frame / region rows on the tile GEMM; the fused class-similarity, layer-norm and frame-embedding
    kernels): outputs only, both test_mode settings.  Inputs and weights come from cvc.synth (same seed) on the test side."""
    import dataclasses
    import misc.utils as ref_utils
    d = dataclasses.replace(synth.CONFIGS["tiny"], **WIDE)
    seed = 1239
    tables = synth.detectron_tables(d, seed)
    inp = synth.encoder_inputs(d, seed)
    out = OrderedDict()
    out["meta.seed"] = np.asarray(seed)
    bt = {k: t(v) for k, v in inp.items()}
    overlaps = ref_utils.bbox_overlaps(bt["proposals"], bt["gt_bboxs"], (bt["frm_mask"] | bt["pnt_mask_in"][:, 1:].unsqueeze(-1)))
    for name, over in (("train.", {}), ("test.", dict(test_mode=True))):
        enc, ctor = build_reference_encoder(d, tables, seed, 1, **over)
        with torch.no_grad():
            res = enc(bt["segs_feat"], bt["proposals"], bt["num"], bt["box_mask"], bt["region_feats"], bt["gt_bboxs"], overlaps,
                      bt["sample_idx"])
        put(out, name + "out.", dict(zip(ENC_OUT, res[:8])))
        out[name + "out.cls_loss"] = res[9].detach().numpy()
    np.savez_compressed(path, **out)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1024))


def g6_dataloader(path):
    """The reference's misc/dataloader_anet.py::DataLoader itself, run over the tiny synthetic dataset of
    cvc.data_fixture (written in the reference's own file formats), with stand-ins ONLY for the third-party modules this
    image lacks: h5py (File -> the two proposal arrays from the .npz twin), torchtext.vocab.GloVe (-> the dataset's GloVe
    table) and torchvision (imported by the reference, never used on this path).  Captures every 12-tuple of two splits,
    the test-mode tuples, and the constructor's GloVe tables."""
    import importlib
    import random
    import tempfile
    from cvc.data_fixture import write_tiny_anet_dataset
    root = tempfile.mkdtemp(prefix="g6_")
    o = write_tiny_anet_dataset(root, seed=7)

    class _H5File(dict):
        def __init__(self, p, mode="r", driver=None):
            with np.load(p) as z:
                super().__init__({k: z[k] for k in z.files})

        def close(self):
            pass
    h5 = types.ModuleType("h5py"); h5.File = _H5File
    tt, ttv = types.ModuleType("torchtext"), types.ModuleType("torchtext.vocab")

    class _GloVe:
        def __init__(self, name=None, dim=300):
            z = np.load(o.glove_path)
            self.stoi = {str(w): i for i, w in enumerate(z["words"])}
            self.vectors = torch.from_numpy(z["vectors"]).float()
    ttv.GloVe = _GloVe; tt.vocab = ttv
    tv, tvd, tvf, tvt = (types.ModuleType(n) for n in ("torchvision", "torchvision.datasets", "torchvision.datasets.folder",
                                                      "torchvision.transforms"))
    tvf.default_loader = None; tvd.folder = tvf; tv.datasets = tvd; tv.transforms = tvt
    sys.modules.update({"h5py": h5, "torchtext": tt, "torchtext.vocab": ttv, "torchvision": tv, "torchvision.datasets": tvd,
                        "torchvision.datasets.folder": tvf, "torchvision.transforms": tvt})
    ref = importlib.import_module("misc.dataloader_anet")
    out = OrderedDict()
    cwd = os.getcwd()
    os.chdir(root)                                   # the reference opens 'data/vg_object_vocab.txt' relative to the CWD
    try:
        for tag, split, test_mode in (("train", "training", False), ("val", "validation", False), ("test", "training", True)):
            ro = argparse.Namespace(**{k: getattr(o, k) for k in (
                "batch_size", "seq_per_img", "seq_length", "att_feat_size", "feature_root", "seg_feature_root", "num_sampled_frm",
                "num_prop_per_frm", "exclude_bgd_det", "prop_thresh", "t_attn_size", "input_dic", "input_json", "grd_reference",
                "proposal_h5")}, test_mode=test_mode)
            np.random.seed(3); random.seed(3)
            ds = ref.DataLoader(ro, split=split, seq_per_img=o.seq_per_img)
            out[tag + ".len"] = np.asarray(len(ds))
            if tag == "train":
                for k in ("glove_vg_cls", "glove_clss", "glove_w"):
                    out["tables." + k] = np.asarray(getattr(ds, k))
                out["tables.vocab_size"], out["tables.detect_size"] = np.asarray(ds.vocab_size), np.asarray(ds.detect_size)
                out["tables.split_ix"] = np.asarray(ds.split_ix)
            for i in range(len(ds)):
                item = ds[i]
                for j, x in enumerate(item):
                    if isinstance(x, str):
                        out["%s.%d.%d" % (tag, i, j)] = np.asarray(x)
                    else:
                        out["%s.%d.%d" % (tag, i, j)] = x.numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    finally:
        os.chdir(cwd)
    np.savez_compressed(path, **out)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1024))


def g7_sentinel(path):
    """with_sentinel=True (model/modules.py:40-41, 53-55, 123-124, 136-138: masked positions filled with -inf instead of -1e8),
    through the two attention modules and the two cores that forward the flag (decoder_core.py:55, localizer_core.py:37).  Same
    tiny inputs as g1 (clip 2 fully masked: its rows are NaN in the reference, which is part of the contract)."""
    d = synth.CONFIGS["tiny"]
    seed = 1234
    sd = synth.hot_path_state_dict(d, seed)
    feats_np = synth.clip_features(d, seed, full_mask_clip=2)
    B, N, R, A, E = d.B, d.N, d.R, d.A, d.E
    h = t(synth.normal((B, R), seed, "unit.h") * 0.5)
    emb = t(np.maximum(synth.normal((B, E), seed, "unit.emb"), 0))
    st_h = t(synth.normal((2, B, R), seed, "unit.state_h") * 0.5)
    st_c = t(synth.normal((2, B, R), seed, "unit.state_c") * 0.5)
    fmask = t(synth.uniform((B, N), seed, "unit.fmask") < 0.4)
    ft = feats_to_torch(feats_np, False)
    mask = ft["pnt_mask"][:, 1:]
    opts = make_opts(d)
    out = OrderedDict()
    out["meta.seed"] = np.asarray(seed)
    add = AdditiveSoftAttention(R, A)
    add.load_state_dict({k.split("soft_attn.")[1]: t(v) for k, v in sd.items() if k.startswith("decoder_core.soft_attn.")})
    ctx, a, fm = add(h, ft["p_pool_feats"], context=ft["pool_feats"], mask=mask, proposal_frame_mask=fmask, with_sentinel=True)
    put(out, "add.", dict(ctx=ctx, attn=a, fm=fm))
    dot = SoftAttention(E, A, temp=2.5)
    dot.load_state_dict({k.split("soft_attn.")[1]: t(v) for k, v in sd.items() if k.startswith("localizer_core.soft_attn.")})
    ctx, a, fm = dot(emb, ft["p_pool_feats"], context=ft["pool_feats"], mask=mask, proposal_frame_mask=fmask, with_sentinel=True)
    put(out, "dot.", dict(ctx=ctx, attn=a, fm=fm))
    core = TopDownDecoderCore(opts)
    core.load_state_dict({k[len("decoder_core."):]: t(v) for k, v in sd.items() if k.startswith("decoder_core.")})
    core.eval()
    o, st, ra, fma, wp = core(emb, ft["fc_feats"], ft["conv_feats"], ft["p_conv_feats"], ft["pool_feats"],
                              ft["p_pool_feats"], mask, (st_h, st_c), proposal_frame_mask=fmask, with_sentinel=True)
    put(out, "core.", dict(out=o, h=st[0], c=st[1], roi_attn=ra, fm=fma, ctx_r=wp))
    loc = LocalizerNoLSTMCore(opts)
    loc.load_state_dict({k[len("localizer_core."):]: t(v) for k, v in sd.items() if k.startswith("localizer_core.")})
    a, b_, c_, _ = loc(emb, ft["fc_feats"], ft["conv_feats"], ft["p_conv_feats"], ft["pool_feats"],
                       ft["p_pool_feats"], mask, None, None, proposal_frame_mask=fmask, with_sentinel=True)
    put(out, "loc.", dict(loc_pool=a, loc_conv=b_, prob=c_))
    np.savez_compressed(path, **out)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1024))


# ------------------------------------------------------------------------------------ G9 (full size, from the reference itself)
def _greedy_ref(d, seed):
    """the reference's own _sample (captioner.py:384-443) on cvc.synth's seeded inputs -> seq, att2_weights, the non-UNK deciding
    margins of every step (best minus second-best log-prob over the words that are not UNK, :415-422)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import fullsize_oracle as FO
    sd, feats_np = synth.hot_path_state_dict(d, seed), synth.clip_features(d, seed)
    batch_np = synth.label_glue_batch(d, seed)
    ft, bt = feats_to_torch(feats_np, False), {k: t(v) for k, v in batch_np.items()}
    model = build_reference_model(d, sd, ft)
    logits = []
    hk = model.logit.register_forward_hook(lambda m, i, o: logits.append(o.detach().clone()))
    with torch.no_grad():
        seq, att2, _ = model_call(model, bt, ft, True)
    hk.remove()
    logp = torch.log_softmax(torch.stack(logits, 1), 2)
    return dict(seq=seq.numpy(), att2_weights=att2.numpy(), gaps=FO.deciding_gaps(logp.numpy()),
                inputs_digest=np.array(FO.inputs_digest(sd, feats_np)))


def g9_fullsize_ref(path):
    """BASELINE's benchmark sizes pinned to the REFERENCE (round-4 review item 3): its greedy sampler at config 2 and config 5,
    its cyclical pass (_forward_3_loops, captioner.py:196-382) at config 3 in eval mode with the objective 0.5 lm + 0.5 lm_recon
    (five losses, ground_weights, per-parameter gradient norms + the elements at tests/fullsize_oracle.py::sample_index).  The
    inputs are cvc.synth's (config, seed) -- the seeds the GPU tests use; a digest of the WHOLE input arrays is stored."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import time
    import fullsize_oracle as FO
    torch.set_num_threads(os.cpu_count() or 8)
    out = OrderedDict()
    for cfg, seed in (("cfg2", 1236), ("cfg5", 1505)):
        t0 = time.time()
        put(out, cfg + ".greedy.", _greedy_ref(synth.CONFIGS[cfg], seed))
        out[cfg + ".greedy.seed"] = np.asarray(seed)
        print(cfg, "greedy: %.0f s" % (time.time() - t0), flush=True)
    d, seed = synth.CONFIGS["cfg3"], 1303
    t0 = time.time()
    sd, feats_np, batch_np = synth.hot_path_state_dict(d, seed), synth.clip_features(d, seed), synth.label_glue_batch(d, seed)
    ft, bt = feats_to_torch(feats_np, False), {k: t(v) for k, v in batch_np.items()}
    model = build_reference_model(d, sd, ft)
    grabbed = {}
    orig = model._grounder

    def spy(xt, att_feats, mask, bias=None, min_value=-1e8):
        r = orig(xt, att_feats, mask, bias, min_value)
        grabbed["ground_weights"] = r.detach().clone()
        return r
    model._grounder = spy
    losses = model_call(model, bt, ft, False)
    loss_mix(losses).backward()
    name = "cfg3.cyclical."
    out[name + "seed"] = np.asarray(seed)
    out[name + "inputs_digest"] = np.array(FO.inputs_digest(sd, feats_np, batch_np))
    out[name + "losses"] = np.array([float(x.detach().mean()) for x in losses], dtype=np.float64)
    out[name + "ground_weights"] = grabbed["ground_weights"].numpy()
    for n, p in model.named_parameters():
        if n.startswith("roi_feat_extractor."):
            continue
        if p.grad is None:
            out[name + "grad_none." + n] = np.asarray(1)
            continue
        g = p.grad.double().reshape(-1)
        out[name + "grad_norm." + n] = np.asarray(float(g.norm()))
        out[name + "grad_at." + n] = g[torch.from_numpy(FO.sample_index(n, g.numel()))].numpy()
    print("cfg3 cyclical: %.0f s" % (time.time() - t0), flush=True)
    np.savez_compressed(path, **out)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1024))


# ------------------------------------------------------------------------------------ G10 (embedding_vocab_plus_1)
def g10_vocab_plus_1(path):
    """opts.embedding_vocab_plus_1 = True (opts.py:197, captioner.py:53-60, 72-76): the embedding table and the vocabulary head
    get V + 1 rows while every vocab_size-relative computation (the grounder's clamp :283, the criterion's range check
    utils.py:134, bbox_target) keeps V.  Tiny dims: greedy sample + per-step log-probs, the cyclical pass's losses and every
    gradient (eval mode)."""
    d = synth.CONFIGS["tiny"]
    seed = 1240
    sd = synth.hot_path_state_dict(d, seed, vocab_plus_1=True)
    feats_np = synth.clip_features(d, seed)
    batch_np = synth.label_glue_batch(d, seed)
    out = OrderedDict()
    out["meta.seed"] = np.asarray(seed)
    ft = feats_to_torch(feats_np, False)
    bt = {k: t(v) for k, v in batch_np.items()}
    model = build_reference_model(d, sd, ft, embedding_vocab_plus_1=True)
    assert model.logit.weight.shape[0] == d.V + 1 and model.embed[0].weight.shape[0] == d.V + 1
    logits = []
    hk = model.logit.register_forward_hook(lambda m, i, o: logits.append(o.detach().clone()))
    with torch.no_grad():
        seq, att2, _ = model_call(model, bt, ft, True)
    hk.remove()
    put(out, "a8.", dict(seq=seq, att2_weights=att2, logp=torch.log_softmax(torch.stack(logits, 1), 2)))
    ft = feats_to_torch(feats_np, True)
    model = build_reference_model(d, sd, ft, embedding_vocab_plus_1=True)
    losses = model_call(model, bt, ft, False)
    put(out, "a9.cyc.", {"loss%d" % i: l for i, l in enumerate(losses)})
    loss = loss_mix(losses)
    put(out, "a9.cyc.", dict(total=loss))
    put(out, "a9.cyc.", grads_of(model, ft, loss))
    np.savez_compressed(path, **out)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1024))


def g11_encoder_bilstm(path):
    """g8_encoder_wide's shape (rnn_size 256 -> hidden size 128: the persistent recurrence's smallest width) with
    t_attn_mode="bilstm" (reference backbone.py:94-106: nn.LSTM instead of nn.GRU), seq_per_img 1, eval mode: the eight encoder
    outputs for both test_mode settings and, for the non-test case, the norm of every parameter gradient of encoder_probe_loss (as
    g5 stores them).  Inputs and weights come from cvc.synth (same seed) on the test side."""
    import dataclasses
    import misc.utils as ref_utils
    d = dataclasses.replace(synth.CONFIGS["tiny"], **WIDE)
    seed = 1241
    tables = synth.detectron_tables(d, seed)
    inp = synth.encoder_inputs(d, seed)
    out = OrderedDict()
    out["meta.seed"] = np.asarray(seed)
    bt = {k: t(v) for k, v in inp.items()}
    overlaps = ref_utils.bbox_overlaps(bt["proposals"], bt["gt_bboxs"], (bt["frm_mask"] | bt["pnt_mask_in"][:, 1:].unsqueeze(-1)))
    for name, over in (("train.", {}), ("test.", dict(test_mode=True))):
        enc, ctor = build_reference_encoder(d, tables, seed, 1, t_attn_mode="bilstm", **over)
        assert isinstance(enc.context_enc, nn.LSTM)
        res = enc(bt["segs_feat"], bt["proposals"], bt["num"], bt["box_mask"], bt["region_feats"], bt["gt_bboxs"], overlaps,
                  bt["sample_idx"])
        put(out, name + "out.", dict(zip(ENC_OUT, res[:8])))
        out[name + "out.cls_loss"] = res[9].detach().numpy()
        if not over:
            encoder_probe_loss(res).backward()
            for n, p in enc.named_parameters():
                if p.grad is None:
                    out[name + "grad." + n + ".is_none"] = np.asarray(1)
                else:
                    out[name + "grad." + n + ".norm"] = np.asarray(p.grad.double().norm().item())
    np.savez_compressed(path, **out)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    gdir = os.path.join(ROOT, "tests", "golden")
    os.makedirs(gdir, exist_ok=True)
    only = sys.argv[1:]
    jobs = {"g1": lambda: g1_tiny(os.path.join(gdir, "g1_tiny.npz")),
            "g2": lambda: g2_cfg1(os.path.join(gdir, "g2_cfg1.npz")),
            "g3": lambda: g3_shards(os.path.join(gdir, "g3_shards.npz")),
            "g4": lambda: g4_config_surface(os.path.join(gdir, "config_surface.json")),
            "g5": lambda: g5_encoder(os.path.join(gdir, "g5_encoder.npz")),
            "g6": lambda: g6_dataloader(os.path.join(gdir, "g6_dataloader.npz")),
            "g7": lambda: g7_sentinel(os.path.join(gdir, "g7_sentinel.npz")),
            "g8": lambda: g8_encoder_wide(os.path.join(gdir, "g8_encoder_wide.npz")),
            "g9": lambda: g9_fullsize_ref(os.path.join(gdir, "g9_fullsize_ref.npz")),      # ~10 min, 30 GB: only when named
            "g10": lambda: g10_vocab_plus_1(os.path.join(gdir, "g10_vocab_plus_1.npz")),
            "g11": lambda: g11_encoder_bilstm(os.path.join(gdir, "g11_encoder_bilstm.npz"))}
    if "--fullsize" in only:
        only = [x for x in only if x != "--fullsize"] + ["g9"]
    for name, job in jobs.items():
        if (not only and name != "g9") or name in only:
            job()
