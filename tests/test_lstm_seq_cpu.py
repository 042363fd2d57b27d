"""The `bilstm` frame encoder, CPU side: the packed W_hh layout the HIP recurrence reads, the fp64 restatement the GPU tests use as
their reference (proven here against nn.LSTM and its autograd), the mirror's encoder in this mode against the reference's own
outputs and gradient norms (tests/golden/g11_encoder_bilstm.npz, tools/make_golden.py g11), and what cvc.lstm_seq refuses."""
import dataclasses

import numpy as np
import pytest
import torch

from cvc import synth
from conftest import Golden
from helpers import make_opts, to_dev
import lstm_ref as R

D = synth.CONFIGS["tiny"]
WIDE = dict(B=5, N=20, F=9, R=256, A=64, E=32, K=3)        # g8 / g11: rnn_size 256 -> hidden size 128
OUT = ("fc_feats", "conv_feats", "p_conv_feats", "pool_feats", "p_pool_feats", "g_pool_feats", "pnt_mask", "overlaps_expanded")


def build_bilstm_encoder(seed, **over):
    """the mirror's encoder at g11's shape with t_attn_mode="bilstm", weights from cvc.synth -> (encoder on the CPU in eval(), Dw)"""
    from cvc.model.backbone import RegionalFeatureExtractorGVD
    Dw = dataclasses.replace(D, **WIDE)
    tables = synth.detectron_tables(Dw, seed)
    o = make_opts(Dw, seq_per_img=1, enable_BUTD=False, att_input_mode="both", num_sampled_frm=4, finetune_cnn=False,
                  att_feat_size=Dw.G, fc_feat_size=synth.SEG_FEAT_DIM, t_attn_size=Dw.F, second_drop_prob=0.3, att_model="topdown",
                  t_attn_mode="bilstm", itod={i + 1: "d%d" % i for i in range(Dw.DET)},
                  vg_cls=["vg%d" % i for i in range(tables["glove_vg_cls"].shape[0])],
                  glove_clss=torch.from_numpy(tables["glove_clss"]), glove_vg_cls=torch.from_numpy(tables["glove_vg_cls"]),
                  detectron_tables=tables, **dict(dict(test_mode=False), **over))
    enc = RegionalFeatureExtractorGVD(o)
    ctor = {k: v.detach().clone() for k, v in enc.state_dict().items() if k in synth.ENCODER_CTOR_KEYS}
    enc.load_state_dict({k: (ctor[k] if k in ctor else torch.from_numpy(np.asarray(synth.encoder_fill(k, v.shape, seed))))
                         for k, v in enc.state_dict().items()})
    return enc.eval(), Dw


def encoder_inputs(Dw, seed, dev):
    from cvc.misc import utils
    inp = to_dev(synth.encoder_inputs(Dw, seed), dev)
    overlaps = utils.bbox_overlaps(inp["proposals"], inp["gt_bboxs"], inp["frm_mask"] | inp["pnt_mask_in"][:, 1:].unsqueeze(-1))
    return inp, overlaps


def run_encoder(enc, inp, overlaps):
    return enc(inp["segs_feat"], inp["proposals"], inp["num"], inp["box_mask"], inp["region_feats"], inp["gt_bboxs"],
               overlaps, inp["sample_idx"])


def probe_loss(outs):
    fc, conv, pconv, pool, ppool, g = outs[:6]
    return (0.01 * fc.sum() + conv.pow(2).mean() + pconv.mean() + pool.pow(2).mean() + ppool.pow(2).mean()
            + g.pow(2).mean() + outs[9].sum())


def check_gradient_norms(enc, want):
    params = dict(enc.named_parameters())
    assert set(k[:-len(".norm")] if k.endswith(".norm") else k for k in want) == set(params)
    for k, v in want.items():
        if v is None:
            assert params[k].grad is None, k
        else:
            got = params[k[:-len(".norm")]].grad.double().norm().item()
            assert got == pytest.approx(float(v), rel=1e-4, abs=1e-7), k


# ---- 1. packed-weight layout
@pytest.mark.parametrize("H", [16, 40, 128])
def test_lstm_weight_pack_layout(H):
    """pack_lstm_weights (pack_weights(w, lstm_R=H) on the k-padded matrix): gate g of hidden unit 8 b + u is row 8 g + u of block b,
    k in quads of 4; columns beyond H are zero."""
    from cvc.lstm_seq import pack_lstm_weights
    w = torch.arange(4 * H * H, dtype=torch.float32).view(4 * H, H) + 1
    p = pack_lstm_weights(w, H)
    Kp = (H + 31) // 32 * 32
    assert p.shape == (H // 8, Kp // 4, 32, 4)
    for b in range(H // 8):
        for g in range(4):
            for u in range(8):
                row = p[b, :, 8 * g + u, :].reshape(-1)
                assert torch.equal(row[:H], w[g * H + 8 * b + u]), (b, g, u)
                assert not row[H:].any()


# ---- 2. the fp64 reference
@pytest.mark.parametrize("B,F,inp,H,layers,bidir", [(3, 5, 32, 16, 2, True), (5, 9, 24, 40, 1, False), (4, 6, 64, 32, 3, True),
                                                    (2, 7, 16, 8, 2, False)])
def test_fp64_restatement_matches_the_library_module_and_its_autograd(B, F, inp, H, layers, bidir):
    lstm = R.make_lstm(inp, H, layers, bidir, 3).double()
    x = torch.randn(B, F, inp, dtype=torch.float64, requires_grad=True)
    probe = torch.randn(B, F, (2 if bidir else 1) * H, dtype=torch.float64)
    want = lstm(x)[0]
    (want * probe).sum().backward()
    params = dict(lstm.named_parameters())
    got, saved = R.lstm_forward(x.detach(), params, layers, bidir)
    assert float((got - want.detach()).abs().max()) < 1e-12
    dx, grads = R.lstm_backward(probe, saved, params, layers, bidir)
    assert float((dx - x.grad).abs().max()) < 1e-12
    assert set(grads) == set(params)
    for k, p in params.items():
        assert float((grads[k] - p.grad).abs().max()) < 1e-12, k


# ---- 3. the mirror's encoder in the LSTM mode against the reference
@pytest.mark.parametrize("case,over", [("train.", {}), ("test.", {"test_mode": True})])
def test_bilstm_encoder_forward_matches_reference(case, over):
    g11 = Golden("g11_encoder_bilstm.npz")
    seed = int(g11["meta.seed"])
    enc, Dw = build_bilstm_encoder(seed, **over)
    assert isinstance(enc.context_enc, torch.nn.LSTM)
    inp, overlaps = encoder_inputs(Dw, seed, "cpu")
    res = run_encoder(enc, inp, overlaps)
    want = g11.sub(case + "out.")
    for k, got in zip(OUT, res[:8]):
        if got.dtype == torch.bool:
            np.testing.assert_array_equal(got.numpy(), want[k], err_msg=k)
        else:
            np.testing.assert_allclose(got.detach().numpy(), want[k], rtol=1e-5, atol=2e-6, err_msg=k)
    np.testing.assert_allclose(res[9].detach().numpy().reshape(-1), want["cls_loss"].reshape(-1), rtol=1e-5, atol=1e-6)


def test_bilstm_encoder_gradients_match_reference():
    g11 = Golden("g11_encoder_bilstm.npz")
    seed = int(g11["meta.seed"])
    enc, Dw = build_bilstm_encoder(seed)
    inp, overlaps = encoder_inputs(Dw, seed, "cpu")
    probe_loss(run_encoder(enc, inp, overlaps)).backward()
    check_gradient_norms(enc, g11.sub("train.grad."))


# ---- 4. what the module refuses; dropout sites
def test_supported_refuses_what_the_kernels_do_not_cover():
    from cvc import lstm_seq as LS

    class FakeCuda:      # `supported` looks at the input's rank, device flag and dtype only (no GPU on this box)
        is_cuda, dtype = True, torch.float32
        def __init__(self, nd=3):
            self._nd = nd
        def dim(self):
            return self._nd
    x = FakeCuda()
    ok = torch.nn.LSTM(32, 16, 2, bidirectional=True, batch_first=True)
    assert LS.supported(ok, x) and LS.supported_train(ok, x)
    assert not LS.supported(torch.nn.LSTM(32, 16, 2, batch_first=True, proj_size=8), x)
    assert not LS.supported(torch.nn.LSTM(32, 16, 2, batch_first=True, bias=False), x)
    assert not LS.supported(torch.nn.LSTM(32, 16, 2, batch_first=False), x)
    assert not LS.supported(torch.nn.LSTM(32, 20, 1, batch_first=True), x)            # H % 8 != 0
    assert not LS.supported(torch.nn.GRU(32, 16, 1, batch_first=True), x)
    assert not LS.supported(ok, torch.zeros(2, 3, 32))                                # a CPU tensor
    assert not LS.supported(ok, FakeCuda(2))


def test_lstm_dropout_sites_have_ids_of_their_own():
    from cvc import dropout
    ids = [dropout.site_id("enc.lstm.%d" % l) for l in range(3)]
    others = [v for k, v in dropout._SITES.items() if not k.startswith("enc.lstm.")]
    others += [dropout.site_id("out_a.%d" % t) for t in range(256)] + [dropout.site_id("out_c.%d" % t) for t in range(256)]
    assert len(set(ids)) == 3 and not set(ids) & set(others)
    assert len(set(dropout._SITES.values())) == len(dropout._SITES)


def test_encoder_reports_the_lstm_recurrence_as_its_own():
    """the wiring of cvc/model/backbone.py: an nn.LSTM frame encoder reports error words and is capturable in deferred mode, as the
    GRU; one with projections (library module) is not"""
    from cvc.model import backbone
    enc, _ = build_bilstm_encoder(5)
    assert enc.reports_error_words()
    assert enc.step_capturable(True) and not enc.step_capturable(False)
    enc.context_enc = torch.nn.LSTM(256, 128, 2, bidirectional=True, batch_first=True, proj_size=64)
    assert not enc.step_capturable(True) and not enc.reports_error_words()
    prev, backbone.HIP_GRU = backbone.HIP_GRU, False
    try:
        enc, _ = build_bilstm_encoder(5)
        assert not enc.step_capturable(True) and not enc.reports_error_words()
    finally:
        backbone.HIP_GRU = prev
