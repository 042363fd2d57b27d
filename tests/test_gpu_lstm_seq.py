"""The `bilstm` frame encoder on the GPU: cvc.lstm_seq (tile-GEMM input projections + the LSTM recurrence of csrc/lstm_seq.hip in its
persistent and its per-step form, inference and autograd) against the fp64 restatement of tests/lstm_ref.py (proven against
nn.LSTM in tests/test_lstm_seq_cpu.py), the building blocks by name, and the encoder in this mode against the reference's own outputs
(tests/golden/g11_encoder_bilstm.npz).

Tolerances are the GRU's (tests/test_encoder.py): 5e-5 max-abs / rtol 1e-4 on outputs, 1e-4 relative norm on gradients; they were
not widened for the LSTM.  Measured on an MI355X: outputs 1.0e-7 .. 1.9e-7 from fp64 at the shapes below (saved gates and c
1.9e-7), the two forms 0 .. 1.8e-7 from each other, 5.5e-7 from fp32 nn.LSTM on the host at config-2 size (F = 480, |y| <= 0.28).

This file is the path as the product runs it, at the workload's sizes, with gradients checked by norm.  The kernels themselves --
every entry point of csrc/lstm_seq.hip by name, isolated from the tile GEMM, every instantiation, strided layouts, poisoned
padding and workspaces, gradients element-wise -- are pinned in tests/test_gpu_lstm_seq_kernels.py."""
import ctypes

import numpy as np
import pytest
import torch

import lstm_ref as R
from conftest import Golden
from test_lstm_seq_cpu import OUT, build_bilstm_encoder, check_gradient_norms, encoder_inputs, probe_loss, run_encoder

pytestmark = pytest.mark.gpu

ATOL, RTOL, GRAD_REL = 5e-5, 1e-4, 1e-4
BADARG = -1


def rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).norm() / (b.double().norm() + 1e-30))


def close(got, want, what=""):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    err = float((got - want).abs().max())
    print("%s max |err| %.3g (max |ref| %.3g)" % (what, err, float(want.abs().max())))
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=RTOL, atol=ATOL, err_msg=what)


def want_form(H):
    return "persistent" if (H % 128 == 0 and H <= 1024) else "steps"


# ---- 5, 6: inference, both forms
# every instantiation of lstm_persistent_kernel<MT, NC, NW>: NC 1..4 at 8 waves (H % 256 == 0), NC 1, 3, 5, 7 at 4 waves, each at
# MT 1 (32 clips) and MT 2 (33 clips)
EVERY_INSTANTIATION = [(B, 3, 16, H, 1, True) for H in range(128, 1025, 128) for B in (32, 33)]


@pytest.mark.parametrize("B,F,inp,H,layers,bidir", [(3, 5, 32, 16, 2, True), (64, 20, 256, 128, 2, True), (70, 7, 48, 128, 2, True),
                                                    (9, 11, 24, 40, 1, False), (33, 11, 100, 72, 2, True), (20, 33, 64, 384, 2, True),
                                                    (64, 17, 96, 256, 1, False), (40, 9, 64, 512, 3, True)] + EVERY_INSTANTIATION)
def test_lstm_hip_vs_fp64(B, F, inp, H, layers, bidir):
    """lstm_forward in the form the shape selects and in the per-step form against the fp64 reference and against each other; more
    than 64 clips run in chunks; a second run of each form gives the same bits (fixed reduction order)."""
    from cvc import lstm_seq as LS
    lstm = R.make_lstm(inp, H, layers, bidir, 5)
    x = torch.randn(B, F, inp)
    want, _ = R.lstm_forward(x, dict(lstm.named_parameters()), layers, bidir)
    ld = lstm.to("cuda:0")
    with torch.no_grad():
        assert LS.supported(ld, x.cuda())
        got = LS.lstm_forward(ld, x.cuda())
        assert LS.last_form == want_form(H)
        again = LS.lstm_forward(ld, x.cuda())
        LS.PERSISTENT = False
        try:
            steps = LS.lstm_forward(ld, x.cuda())
            assert LS.last_form == "steps"
            steps_again = LS.lstm_forward(ld, x.cuda())
        finally:
            LS.PERSISTENT = True
    assert torch.equal(got, again) and torch.equal(steps, steps_again)
    close(got, want, "selected form")
    close(steps, want, "per-step form")
    close(got, steps, "form vs form")


# ---- 7: full size
def test_lstm_hip_full_size_vs_library_cpu():
    """Config-2 encoder size (B=64 clips, F=480 frames, R=2048 -> H=1024, 2 layers, bidirectional): HIP path against nn.LSTM on the
    host CPU (the module the reference calls).  Measured: max |err| 5.5e-7 at max |y| 0.28 (the host's fp32 module is itself 3.5e-7
    from fp64 at this size): c is a 480-step running sum, but the bound of the GRU's test holds with two orders to spare."""
    from cvc import lstm_seq as LS
    lstm = R.make_lstm(2048, 1024, 2, True, 7)
    x = torch.randn(64, 480, 2048)
    with torch.no_grad():
        want = lstm(x)[0]
        got = LS.lstm_forward(lstm.to("cuda:0"), x.cuda()).cpu()
    assert LS.last_form == "persistent"
    err = (got - want).abs().max().item()
    print("full size: max |err| %.3g, max |y| %.3g" % (err, want.abs().max().item()))
    assert err < ATOL, err
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=RTOL, atol=ATOL)


# ---- 8: autograd
@pytest.mark.parametrize("B,F,inp,H,layers,bidir", [(5, 7, 48, 128, 2, True), (64, 12, 96, 256, 1, False), (70, 5, 64, 128, 2, True),
                                                    (37, 9, 80, 256, 3, True), (6, 5, 24, 16, 2, True), (33, 4, 40, 200, 1, True),
                                                    (16, 3, 64, 2048, 1, True)])
def test_lstm_hip_autograd_vs_fp64(B, F, inp, H, layers, bidir):
    """lstm_forward_train (forward keeping gates and c, cvc_lstm_seq_bwd, dense dW / dX products on the tile GEMM) against the fp64
    reference's backward: output, input gradient and every parameter gradient."""
    from cvc import lstm_seq as LS
    lstm = R.make_lstm(inp, H, layers, bidir, 11)
    x = torch.randn(B, F, inp)
    probe = torch.randn(B, F, (2 if bidir else 1) * H)
    params = dict(lstm.named_parameters())
    want_y, saved = R.lstm_forward(x, params, layers, bidir)
    want_dx, want = R.lstm_backward(probe, saved, params, layers, bidir)
    ld = lstm.to("cuda:0")
    xg = x.cuda().requires_grad_(True)
    assert LS.supported_train(ld, xg)
    y = LS.lstm_forward_train(ld, xg)
    assert LS.last_train_form == want_form(H)
    close(y, want_y, "y")
    (y * probe.cuda()).sum().backward()
    assert rel(xg.grad, want_dx) < GRAD_REL, rel(xg.grad, want_dx)
    for k, p in ld.named_parameters():
        assert p.grad is not None and rel(p.grad, want[k]) < GRAD_REL, (k, rel(p.grad, want[k]))


def test_lstm_hip_autograd_full_size_vs_library_cpu():
    """Config-2 encoder width and batch (B=64, R=2048 -> H=1024, 2 layers, both directions) over F=240 frames under autograd against
    torch autograd of nn.LSTM on the host CPU (half of config 2's frames, as the GRU's test: the host's pass is what this waits for)."""
    from cvc import lstm_seq as LS
    lstm = R.make_lstm(2048, 1024, 2, True, 13)
    x = torch.randn(64, 240, 2048)
    probe = torch.randn(64, 240, 2048) / 240 ** 0.5
    xc = x.clone().requires_grad_(True)
    ref_y = lstm(xc)[0]
    (ref_y * probe).sum().backward()
    want = {k: p.grad.clone() for k, p in lstm.named_parameters()}
    want_dx, ref_y = xc.grad.clone(), ref_y.detach()
    for p in lstm.parameters():
        p.grad = None
    ld = lstm.to("cuda:0")
    xg = x.cuda().requires_grad_(True)
    y = LS.lstm_forward_train(ld, xg)
    assert LS.last_train_form == "persistent"
    assert float((y.detach().cpu() - ref_y).abs().max()) < ATOL
    (y * probe.cuda()).sum().backward()
    assert rel(xg.grad, want_dx) < GRAD_REL, rel(xg.grad, want_dx)
    for k, p in ld.named_parameters():
        assert rel(p.grad, want[k]) < GRAD_REL, (k, rel(p.grad, want[k]))


@pytest.mark.parametrize("B,F,inp,H", [(6, 5, 32, 128), (5, 4, 24, 40)])
def test_lstm_hip_train_mode_dropout_uses_the_kernel_mask(B, F, inp, H):
    """train() with dropout 0.2 between the layers: output and gradients equal the fp64 reference under the kernel's own masks (sites
    enc.lstm.<l>), restated on the host through cvc.dropout.host_mask."""
    from cvc import dropout, lstm_seq as LS
    layers = 3
    lstm = R.make_lstm(inp, H, layers, True, 17, dropout=0.2)
    x = torch.randn(B, F, inp)
    probe = torch.randn(B, F, 2 * H)
    ld = lstm.to("cuda:0").train()
    dropout.seed(123)
    xg = x.cuda().requires_grad_(True)
    y = LS.lstm_forward_train(ld, xg)
    (y * probe.cuda()).sum().backward()
    # the masks act on time-major rows (t, clip): [F * B, 2H] -> [B, F, 2H]
    masks = [dropout.host_mask("enc.lstm.%d" % l, (F * B, 2 * H), 0.2, xg.device).view(F, B, 2 * H).transpose(0, 1).double()      # 0 or 1 / (1 - p)
             for l in range(layers - 1)]
    assert all(0 < float((m == 0).double().mean()) < 0.5 for m in masks)
    params = {k: v.detach().cpu() for k, v in ld.named_parameters()}
    want_y, saved = R.lstm_forward(x, params, layers, True, masks)
    want_dx, want = R.lstm_backward(probe, saved, params, layers, True, masks)
    close(y, want_y, "y under dropout")
    assert rel(xg.grad, want_dx) < GRAD_REL
    for k, p in ld.named_parameters():
        assert rel(p.grad, want[k]) < GRAD_REL, k
    with torch.no_grad():                      # eval(): no dropout
        ld.eval()
        close(LS.lstm_forward(ld, x.cuda()), R.lstm_forward(x, params, layers, True)[0], "eval")


# ---- 9: the building blocks by name
def _block(name, restype, argtypes):
    from cvc import hip
    L = hip.lib()
    addr = L.cvc_block(name.encode())
    assert addr, name
    return ctypes.CFUNCTYPE(restype, *argtypes)(addr)


def test_lstm_blocks_by_name_saved_tensors_backward_and_rejected_arguments():
    """cvc_lstm_seq_persistent_train_fwd and cvc_lstm_seq_bwd through cvc_block: y, the saved activated gates and c, and the gate
    gradients dG against fp64; arguments outside the contract return CVC_E_BADARG without launching (outputs untouched)."""
    from cvc import hip
    from cvc.lstm_seq import pack_lstm_weights
    P, LL, I = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int
    fwd = _block("cvc_lstm_seq_persistent_train_fwd", I, [P, P, LL, LL, P, P, I, I, I, I, P, P, LL, LL, P, LL, LL, P, LL, LL, P, P])
    bwd = _block("cvc_lstm_seq_bwd", I, [P, LL, LL, P, LL, LL, P, LL, LL, P, I, I, I, I, P, P, P])
    words = _block("cvc_lstm_persistent_sync_words", I, [])
    work_n = _block("cvc_lstm_seq_bwd_work", I, [I, I, I])
    M, F, inp, H, ndir = 37, 6, 48, 128, 2
    lstm = R.make_lstm(inp, H, 1, True, 23)
    params = dict(lstm.named_parameters())
    x = torch.randn(M, F, inp)
    dy = torch.randn(M, F, ndir * H)
    want_y, saved = R.lstm_forward(x, params, 1, True)
    dev = torch.device("cuda:0")
    sfx = ["", "_reverse"]
    g = lambda n: [params[n + "_l0" + s].detach() for s in sfx]
    w_ih = torch.cat(g("weight_ih"), 0)
    gi = (x.transpose(0, 1).reshape(F * M, inp).double() @ w_ih.double().T).float().to(dev)      # time-major rows (t, clip)
    wp = torch.stack([pack_lstm_weights(w, H) for w in g("weight_hh")]).to(dev)
    w_hh = torch.stack(g("weight_hh")).contiguous().to(dev)
    b_ih, b_hh = torch.stack(g("bias_ih")).to(dev), torch.stack(g("bias_hh")).to(dev)
    mk = lambda *s: torch.full(s, 7.0, device=dev)
    y, c, gates = mk(F * M, ndir * H), mk(F * M, ndir * H), mk(F * M, ndir * 4 * H)
    slots = torch.empty((F + 1) * ndir * H * 64, device=dev)
    sync = torch.zeros(int(words()), dtype=torch.int32, device=dev)
    st = hip._stream()

    def call(M_=M, H_=H, g_ld=ndir * 4 * H, wp_=wp, y_=y, gi_off=0):
        return fwd(wp_.data_ptr() if wp_ is not None else None, gi.data_ptr() + gi_off, ndir * 4 * H, M * ndir * 4 * H, b_ih.data_ptr(),
                   b_hh.data_ptr(), M_, F, H_, ndir, slots.data_ptr(), y_.data_ptr() if y_ is not None else None, ndir * H, M * ndir * H,
                   gates.data_ptr(), g_ld, M * ndir * 4 * H, c.data_ptr(), ndir * H, M * ndir * H, sync.data_ptr(), st)
    # rejected: width outside H % 128 == 0, more than 64 clips, a stride that is not a multiple of 4 floats, a misaligned pointer, nulls
    for kw in (dict(H_=136), dict(M_=65), dict(g_ld=ndir * 4 * H + 2), dict(gi_off=4), dict(wp_=None), dict(y_=None)):
        assert call(**kw) == BADARG, kw
    torch.cuda.synchronize()
    assert float(y.min()) == 7.0 and float(c.min()) == 7.0 and float(gates.min()) == 7.0        # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert int(sync[4]) == 0
    tm = lambda t: t.transpose(0, 1).reshape(F * M, -1)            # [M, F, ..] -> time-major rows
    close(y, tm(want_y), "y")
    for d in range(ndir):
        _, gd, cd = saved[0][1][d]
        close(gates[:, d * 4 * H:(d + 1) * 4 * H], tm(gd.reshape(M, F, 4 * H)), "gates dir %d" % d)
        close(c[:, d * H:(d + 1) * H], tm(cd), "c dir %d" % d)
    # backward from the saved tensors
    dyd = tm(dy).contiguous().to(dev)
    dg = mk(F * M, ndir * 4 * H)
    work = torch.empty(int(work_n(M, H, ndir)), device=dev)

    def callb(M_=M, H_=H, c_ld=ndir * H, dg_=dg):
        return bwd(dyd.data_ptr(), ndir * H, M * ndir * H, gates.data_ptr(), ndir * 4 * H, M * ndir * 4 * H, c.data_ptr(), c_ld,
                   M * ndir * H, w_hh.data_ptr(), M_, F, H_, ndir, dg_.data_ptr() if dg_ is not None else None, work.data_ptr(), st)
    for kw in (dict(H_=132), dict(M_=65), dict(c_ld=ndir * H + 1), dict(dg_=None)):
        assert callb(**kw) == BADARG, kw
    torch.cuda.synchronize()
    assert float(dg.min()) == 7.0
    assert callb() == 0
    torch.cuda.synchronize()
    for d in range(ndir):
        xs, (yd, gd, cd) = saved[0][0], saved[0][1][d]
        dz = R.lstm_layer_backward(dy.double()[:, :, d * H:(d + 1) * H], xs, yd, gd, cd, g("weight_ih")[d].double(),
                                   g("weight_hh")[d].double(), d == 1)[4]
        r = rel(dg[:, d * 4 * H:(d + 1) * 4 * H], tm(dz))
        assert r < GRAD_REL, (d, r)


# ---- 10: the encoder in the bilstm mode
def test_bilstm_encoder_forward_golden_on_the_hip_forms(recwarn):
    """g11 (the reference's eval outputs with t_attn_mode="bilstm" at rnn_size 256) against the mirror on the GPU: the persistent LSTM
    recurrence runs (H = 128), the library module is neither used nor warned about."""
    from cvc import dense, hip, lstm_seq as LS
    g11 = Golden("g11_encoder_bilstm.npz")
    seed = int(g11["meta.seed"])
    dev = torch.device("cuda:0")
    min_rows, dense.MIN_ROWS = dense.MIN_ROWS, 8
    for k in [k for k in hip._warned if k.startswith("gru-library")]:
        hip._warned.discard(k)
    try:
        for name, over in (("train.", {}), ("test.", dict(test_mode=True))):
            enc, Dw = build_bilstm_encoder(seed, **over)
            enc = enc.to(dev).eval()
            inp, overlaps = encoder_inputs(Dw, seed, dev)
            LS.last_form = None
            with torch.no_grad():
                res = run_encoder(enc, inp, overlaps)
            assert LS.last_form == "persistent"
            for k, x in zip(OUT, res[:8]):
                want = g11[name + "out." + k]
                if x.dtype.is_floating_point:
                    np.testing.assert_allclose(x.cpu().numpy(), want, rtol=2e-4, atol=2e-5, err_msg=name + k)
                else:
                    np.testing.assert_array_equal(x.cpu().numpy(), want, err_msg=name + k)
            np.testing.assert_allclose(res[9].cpu().numpy(), g11[name + "out.cls_loss"], rtol=2e-4, atol=1e-6)
    finally:
        dense.MIN_ROWS = min_rows
    assert not [w for w in recwarn.list if "library module" in str(w.message)], [str(w.message) for w in recwarn.list]
    assert not [k for k in hip._warned if k.startswith("gru-library")], hip._warned


def test_bilstm_encoder_gradients_golden_on_the_hip_forms(recwarn):
    """gradient norms of encoder_probe_loss against g11, the frame context on lstm_forward_train (persistent forward + cvc_lstm_seq_bwd)"""
    from cvc import dense, lstm_seq as LS
    g11 = Golden("g11_encoder_bilstm.npz")
    seed = int(g11["meta.seed"])
    dev = torch.device("cuda:0")
    min_rows, dense.MIN_ROWS = dense.MIN_ROWS, 8
    try:
        enc, Dw = build_bilstm_encoder(seed)
        enc = enc.to(dev).eval()
        inp, overlaps = encoder_inputs(Dw, seed, dev)
        LS.last_train_form = None
        probe_loss(run_encoder(enc, inp, overlaps)).backward()
        assert LS.last_train_form == "persistent"
    finally:
        dense.MIN_ROWS = min_rows
    check_gradient_norms(enc, g11.sub("train.grad."))
    assert not [w for w in recwarn.list if "library module" in str(w.message)]


def test_bilstm_raw_feature_training_replays_captured_steps_bit_equal_to_eager(capsys):
    """--t_attn_mode bilstm through Trainer.train(): the encoder is capturable in deferred mode, the step is captured and replayed,
    bit-equal to the same epoch of eager steps (as test_gpu_train.py has it for bigru); small shape (rnn_size 256 -> H = 128)."""
    from cvc import dropout, lstm_seq as LS, opts as cvc_opts, synth
    from cvc.data_synth import SyntheticCaptionDataset, collate
    from cvc.model.create_model import build_model
    from cvc.trainer import Trainer, build_optimizer
    dev = torch.device("cuda:0")
    bs, F, H2, n_clips, seed = 4, 6, 128, 28, 3

    def setup():
        o = cvc_opts.build_parser().parse_args(["--batch_size", str(bs), "--num_prop_per_frm", "7", "--t_attn_size", str(F), "--rnn_size",
                                                str(2 * H2), "--att_hid_size", "64", "--input_encoding_size", "32", "--seq_length", "4",
                                                "--vis_encoding_size", "24", "--att_feat_size", "24", "--learning_rate", "0.001",
                                                "--t_attn_mode", "bilstm"])
        o.test_mode = False
        dims = synth.Dims(B=bs, N=7, F=F, R=2 * H2, A=64, E=32, T=4, G=24, K=7)
        full = SyntheticCaptionDataset(dims, n_clips, seed, "training", raw=True)
        o.vocab_size, o.itow, o.wtoi, o.itod, o.detect_size = full.vocab_size, full.itow, full.wtoi, full.itod, dims.DET
        o.glove_clss, o.glove_vg_cls = torch.from_numpy(full.glove_clss), torch.from_numpy(full.glove_vg_cls)
        o.vg_cls, o.detectron_tables = full.vg_cls, full.tables
        o.disp_interval, o.hip_graph = 3, 1
        torch.manual_seed(seed)
        model = build_model(o, dev)
        return o, model, [collate([full[i] for i in range(j, j + bs)]) for j in range(0, n_clips, bs)]
    finals, shown, stats = [], [], []
    for graphed in (False, True):
        o, model, batches = setup()
        assert isinstance(model.roi_feat_extractor.context_enc, torch.nn.LSTM)
        tr = Trainer(o, None, model, build_optimizer(model, o), batches, None)
        assert tr.graph_capable() and model.reports_error_words() and model.step_capturable(deferred_errors=True)
        assert not model.step_capturable(deferred_errors=False)
        tr._graph_broken = not graphed
        dropout.seed(99)
        LS.last_train_form = None
        tr.train(0)
        torch.cuda.synchronize()
        assert LS.last_train_form == "persistent"
        finals.append({k: v.detach().clone() for k, v in model.state_dict().items()})
        shown.append([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Epoch")])
        stats.append(dict(tr.graph_stats))
        assert tr.deferred_stats == dict(void_steps=0, rerun_steps=0)
    assert stats[0] == dict(eager=6, replayed=0, captured=0) and stats[1] == dict(eager=2, replayed=4, captured=1), stats
    strip = lambda ln: ln.split("LM Loss")[1]
    assert len(shown[0]) == 2 and [strip(x) for x in shown[0]] == [strip(x) for x in shown[1]], (shown[0], shown[1])
    for k in finals[0]:
        assert torch.equal(finals[0][k], finals[1][k]), k
