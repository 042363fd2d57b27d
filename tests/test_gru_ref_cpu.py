"""The fp64 restatement of the GRU recurrence the GPU tests use as their reference (tests/gru_ref.py), proven here against
nn.GRU(...).double() and its autograd: forward, input gradient and every parameter gradient to 1e-12 max-abs, the saved (r, z, n, hn)
tensor and the pre-activation gradients dgi / dgh against their definitions, and the inter-layer `masks` path against single-layer
modules with the masks applied by hand between them."""
import pytest
import torch

import gru_ref as R

TOL = 1e-12


def err(a, b):
    return float((a - b).abs().max())


SHAPES = [(3, 5, 12, 16, 1, False), (3, 5, 12, 16, 1, True), (5, 9, 24, 40, 2, False), (3, 5, 32, 16, 2, True), (4, 6, 64, 32, 3, True),
          (2, 7, 16, 8, 3, False), (4, 1, 16, 8, 1, True), (3, 1, 24, 16, 2, True), (1, 2, 8, 8, 3, True)]


@pytest.mark.parametrize("B,F,inp,H,layers,bidir", SHAPES)
def test_fp64_restatement_matches_the_library_module_and_its_autograd(B, F, inp, H, layers, bidir):
    gru = R.make_gru(inp, H, layers, bidir, 3).double()
    gen = torch.Generator().manual_seed(B * 1000 + F * 100 + H)
    x = torch.randn(B, F, inp, dtype=torch.float64, generator=gen).requires_grad_(True)
    probe = torch.randn(B, F, (2 if bidir else 1) * H, dtype=torch.float64, generator=gen)
    want = gru(x)[0]
    (want * probe).sum().backward()
    params = dict(gru.named_parameters())
    got, saved = R.gru_forward(x.detach(), params, layers, bidir)
    assert err(got, want.detach()) < TOL
    dx, grads = R.gru_backward(probe, saved, params, layers, bidir)
    assert err(dx, x.grad) < TOL
    assert set(grads) == set(params)
    for k, p in params.items():
        assert grads[k].shape == p.shape and err(grads[k], p.grad) < TOL, k


@pytest.mark.parametrize("B,F,inp,H,reverse", [(3, 5, 12, 16, False), (3, 5, 12, 16, True), (2, 1, 8, 8, False), (4, 2, 8, 24, True)])
def test_saved_gates_and_preactivation_gradients_are_what_they_are_named(B, F, inp, H, reverse):
    """gates = (r, z, n, hn) with hn = W_hn h + b_hn and h' = (1 - z) n + z h; dgi / dgh are the gradients with respect to the
    pre-activations x W_ih^T + b_ih and h W_hh^T + b_hh of every step (autograd through a forward that takes them as inputs)"""
    gru = R.make_gru(inp, H, 1, False, 7).double()
    w_ih, w_hh, b_ih, b_hh = [p.detach() for p in (gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0)]
    gen = torch.Generator().manual_seed(11 + F)
    x = torch.randn(B, F, inp, dtype=torch.float64, generator=gen)
    dy = torch.randn(B, F, H, dtype=torch.float64, generator=gen)
    y, gates = R.gru_layer_forward(x, w_ih, w_hh, b_ih, b_hh, reverse)
    # the same recurrence with a zero offset added to each step's two pre-activation vectors: its gradient is dgi / dgh
    oi = torch.zeros(B, F, 3 * H, dtype=torch.float64, requires_grad=True)
    oh = torch.zeros(B, F, 3 * H, dtype=torch.float64, requires_grad=True)
    h = x.new_zeros(B, H)
    ys = [None] * F
    for s in range(F):
        t = F - 1 - s if reverse else s
        gi = (x[:, t] @ w_ih.T + b_ih + oi[:, t]).view(B, 3, H)
        gh = (h @ w_hh.T + b_hh + oh[:, t]).view(B, 3, H)
        r, z = torch.sigmoid(gi[:, 0] + gh[:, 0]), torch.sigmoid(gi[:, 1] + gh[:, 1])
        n = torch.tanh(gi[:, 2] + r * gh[:, 2])
        assert err(torch.stack((r, z, n, gh[:, 2]), 1).detach(), gates[:, t]) < TOL
        h = (1 - z) * n + z * h
        ys[t] = h
    yy = torch.stack(ys, 1)
    assert err(yy.detach(), y) < TOL
    (yy * dy).sum().backward()
    dgi, dgh = R.gru_layer_backward(dy, x, y, gates, w_ih, w_hh, reverse)[5:]
    assert err(dgi, oi.grad) < TOL and err(dgh, oh.grad) < TOL
    assert err(dgh[:, :, 2 * H:], dgi[:, :, 2 * H:] * gates[:, :, 0]) < TOL            # dn * r against dn
    assert torch.equal(dgh[:, :, :2 * H], dgi[:, :, :2 * H])


@pytest.mark.parametrize("B,F,inp,H,layers,bidir", [(3, 5, 12, 16, 3, True), (4, 1, 8, 8, 2, True), (2, 4, 8, 24, 2, False)])
def test_masks_path_matches_single_layer_modules_with_the_masks_applied_by_hand(B, F, inp, H, layers, bidir):
    ndir = 2 if bidir else 1
    gru = R.make_gru(inp, H, layers, bidir, 5, dropout=0.2).double().eval()
    params = dict(gru.named_parameters())
    gen = torch.Generator().manual_seed(17 * layers + F)
    x = torch.randn(B, F, inp, dtype=torch.float64, generator=gen).requires_grad_(True)
    probe = torch.randn(B, F, ndir * H, dtype=torch.float64, generator=gen)
    masks = [(torch.rand(B, F, ndir * H, generator=gen) > 0.2).double() / 0.8 for _ in range(layers - 1)]
    assert all(0 < float((m == 0).double().mean()) < 0.5 for m in masks)
    # one single-layer module per layer, sharing the stacked module's parameters
    cur = x
    for l in range(layers):
        one = torch.nn.GRU(inp if l == 0 else ndir * H, H, 1, bidirectional=bidir, batch_first=True).double().eval()
        for k in list(one._parameters):
            setattr(one, k, params[k.replace("_l0", "_l%d" % l)])          # (RNNBase.__setattr__ refreshes its flat-weight list)
        cur = one(cur)[0]
        if l + 1 < layers:
            cur = cur * masks[l]
    (cur * probe).sum().backward()
    got, saved = R.gru_forward(x.detach(), params, layers, bidir, masks)
    assert err(got, cur.detach()) < TOL
    dx, grads = R.gru_backward(probe, saved, params, layers, bidir, masks)
    assert err(dx, x.grad) < TOL
    for k, p in params.items():
        assert err(grads[k], p.grad) < TOL, k
    # without masks the stacked module in eval() is the reference
    assert err(R.gru_forward(x.detach(), params, layers, bidir)[0], gru(x.detach())[0].detach()) < TOL


def test_make_gru_scales_the_default_initialisation():
    torch.manual_seed(9)
    plain = torch.nn.GRU(8, 8, 2, bidirectional=True, batch_first=True)
    scaled = R.make_gru(8, 8, 2, True, 9)
    for (k, a), (_, b) in zip(plain.named_parameters(), scaled.named_parameters()):
        assert torch.equal(a * 1.5, b), k
    assert R.make_gru(8, 8, 2, True, 9, dropout=0.2).dropout == 0.2
