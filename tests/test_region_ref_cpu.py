"""tests/region_ref.py proven on the CPU (no GPU here): every fp64 reference equals the torch formulation of the reference model in
float64; every float32 restatement of a kernel's arithmetic stays within 1.0 of its bound WITHOUT the constant K on every case of
every table (the worst ratio per entry point is printed); every wrong restatement leaves K x bound on a committed case (its
distance is printed)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import region_ref as RR
from region_ref import K, ratio

T64 = torch.float64


def t64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


# ------------------------------------------------------------------------------------------------ the references against torch
@pytest.mark.parametrize("case", RR.SOFTMAX_CASES, ids=str)
def test_softmax_reference_is_torch_softmax_after_masked_fill(case):
    x, bias, pad = RR.softmax_values(case)
    p, _b = RR.softmax_fp64(x, bias, pad, case.C)
    logits = t64(np.nan_to_num(x[:, :case.C].astype(np.float64), nan=0.0, neginf=-np.inf))
    if bias is not None:
        logits = logits + t64(bias)
    if pad is not None:
        logits = logits.masked_fill(torch.from_numpy(pad)[:, None], RR.MIN_VALUE)
    np.testing.assert_allclose(p, torch.softmax(logits, dim=1).numpy(), rtol=1e-12, atol=0)
    if pad is not None and pad.any():
        assert (p[pad] == 1.0 / case.C).all()
    assert np.isfinite(p).all() and ((x[:, :case.C] == -np.inf) <= (p == 0)).all()


@pytest.mark.parametrize("case", RR.LN_CASES, ids=str)
def test_layernorm_reference_is_torch_layer_norm_plus_cat(case):
    xs = RR.ln_values(case)
    out, _b = RR.ln_fp64(xs, case.eps)
    want = torch.cat([Fn.layer_norm(t64(x), [x.shape[1]], eps=float(np.float32(case.eps))) for x in xs], dim=1)
    np.testing.assert_allclose(out, want.numpy(), rtol=1e-9, atol=1e-12)


def bn_module(C, seed):
    """an eval-mode BatchNorm1d in float64 with non-trivial running statistics, negative and zero gamma channels"""
    rng = np.random.default_rng(seed)
    bn = torch.nn.BatchNorm1d(C).double().eval()
    with torch.no_grad():
        bn.weight.copy_(t64(rng.standard_normal(C)))
        bn.weight[::3] = 0.0
        bn.bias.copy_(t64(rng.standard_normal(C)))
        bn.running_mean.copy_(t64(rng.standard_normal(C) * 0.3))
        bn.running_var.copy_(t64(rng.uniform(0.2, 3.0, C)))
    return bn


@pytest.mark.parametrize("case", RR.FE_CASES, ids=str)
def test_frame_embed_reference_is_relu_batchnorm_eval_relu(case):
    y0, b0, y1, b1, _scale, _shift = RR.fe_values(case)
    bn = bn_module(case[1] + case[2], 3)
    scale = (bn.weight / torch.sqrt(bn.running_var + bn.eps)).detach()
    shift = (bn.bias - bn.running_mean * scale).detach()
    out, z, _b = RR.fe_fp64(y0, b0, y1, b1, scale.numpy(), shift.numpy())
    with torch.no_grad():
        want = torch.relu(bn(torch.cat([torch.relu(t64(y0) + t64(b0)), torch.relu(t64(y1) + t64(b1))], dim=1)))
    np.testing.assert_allclose(out, want.numpy(), rtol=1e-12, atol=1e-14)
    assert (z < 0).any() and (z > 0).any() and np.array_equal(out, np.maximum(z, 0))


@pytest.mark.parametrize("case", RR.NLL_CASES, ids=str)
def test_attn_nll_reference_is_autograd_of_the_masked_log_softmax_loss(case):
    x, tg = RR.nll_values(case)
    g = np.array([0.7, -1.3])
    ref = RR.nll_fp64(x, tg)
    d, _b = RR.nll_bwd_fp64(x, tg, g, ref)
    xt = t64(x).requires_grad_(True)
    target = torch.from_numpy(tg).to(T64)
    losses = [-(torch.log_softmax(xt[w], dim=2) * target).sum() / target.sum().clamp(min=1) for w in range(2)]
    (losses[0] * g[0] + losses[1] * g[1]).backward()
    np.testing.assert_allclose(ref.loss, [float(v.detach()) for v in losses], rtol=1e-12)
    assert ref.count == max(int(tg.sum()), 1) and np.array_equal(ref.cnt, tg.reshape(-1, case[2]).sum(axis=1))
    np.testing.assert_allclose(d.reshape(x.shape), xt.grad.numpy(), rtol=1e-9, atol=1e-15)
    np.testing.assert_allclose(ref.lse.reshape(x.shape[:3]), torch.logsumexp(xt.detach(), dim=3).numpy(), rtol=1e-13)


def test_attn_nll_reference_without_a_target():
    x, tg = RR.nll_values((2, 3, 7))
    ref = RR.nll_fp64(x, np.zeros_like(tg))
    d, b = RR.nll_bwd_fp64(x, np.zeros_like(tg), [1.0, 1.0], ref)
    assert (ref.loss == 0).all() and ref.count == 1 and not d.any() and not b.any()


@pytest.mark.parametrize("case", RR.GR_CASES, ids=str)
def test_grounder_reference_is_autograd_of_the_masked_einsum(case):
    xt, feats, bias, mask, d = RR.gr_values(case)
    a, f = t64(xt).requires_grad_(True), t64(feats).requires_grad_(True)
    out = (torch.einsum("btg,bng->btn", a, f) + t64(bias)).masked_fill(torch.from_numpy(mask), RR.MIN_VALUE)
    got, _b = RR.gr_fwd_fp64(xt, feats, bias, mask)
    np.testing.assert_allclose(got, out.detach().numpy(), rtol=1e-12, atol=1e-13)
    # the kernel's backward takes the gradient of the UNMASKED product (the caller zeroes d on masked slots)
    torch.einsum("btg,bng->btn", a, f).backward(t64(d))
    d_xt, _e, d_f, _e2 = RR.gr_bwd_fp64(d, xt, feats)
    np.testing.assert_allclose(d_xt, a.grad.numpy(), rtol=1e-11, atol=1e-12)
    np.testing.assert_allclose(d_f, f.grad.numpy(), rtol=1e-11, atol=1e-12)


@pytest.mark.parametrize("case", RR.EMBED_CASES, ids=str)
def test_embed_reference_is_relu_of_the_embedding(case):
    table, idx, drop = RR.embed_values(case)
    want = torch.relu(Fn.embedding(torch.from_numpy(idx), torch.from_numpy(table)))
    assert np.array_equal(RR.embed_ref(table, idx, None), want.numpy()) and np.isfinite(want.numpy()).all()
    assert np.array_equal(RR.embed_ref(table, idx, drop), (want * torch.from_numpy(drop)).numpy())
    assert (idx == case[1] - 1).any() and (len(set(idx.tolist())) < len(idx) or case[0] < 3)
    assert np.isnan(table).any() or case[1] <= case[0]


# ------------------------------------------------------------------------------------------------ restatements and mutants
def softmax_ratio(case, variant=None):
    x, bias, pad = RR.softmax_values(case)
    want, bound = RR.softmax_fp64(x, bias, pad, case.C)
    return _ratio(RR.softmax_f32(x, bias, pad, case.C, variant), want, bound)


def ln_ratio(case, variant=None):
    xs = RR.ln_values(case)
    want, bound = RR.ln_fp64(xs, case.eps)
    return _ratio(RR.ln_f32(xs, case.eps, variant), want, bound)


def fe_ratio(case, variant=None):
    v = RR.fe_values(case)
    want, _z, bound = RR.fe_fp64(*v)
    return _ratio(RR.fe_f32(*v, variant=variant), want, bound)


NLL_G = (0.7, -1.3)


def nll_fwd_ratio(case, variant=None):
    return max(_nll_fwd_ratio(case, variant, low) for low in (True, False))


def _nll_fwd_ratio(case, variant, low):
    x, tg = RR.nll_values(case, low)
    ref = RR.nll_fp64(x, tg)
    loss, count, lse, part, cnt = RR.nll_fwd_f32(x, tg, variant)
    if variant is None:
        assert count == ref.count and np.array_equal(cnt, ref.cnt)
    return max(_ratio(loss, ref.loss, ref.e_loss), _ratio(lse, ref.lse, ref.e_lse), _ratio(part, ref.part, ref.e_part))


def nll_bwd_ratio(case, variant=None):
    return max(_nll_bwd_ratio(case, variant, low) for low in (True, False))


def _nll_bwd_ratio(case, variant, low):
    x, tg = RR.nll_values(case, low)
    want, bound = RR.nll_bwd_fp64(x, tg, NLL_G)
    return _ratio(RR.nll_bwd_f32(x, tg, NLL_G, variant), want, bound)


def gr_fwd_ratio(case, variant=None):
    xt, feats, bias, mask, _d = RR.gr_values(case)
    want, bound = RR.gr_fwd_fp64(xt, feats, bias, mask)
    return _ratio(RR.gr_fwd_f32(xt, feats, bias, mask, variant), want, bound)


def gr_bwd_ratio(case, variant=None):
    xt, feats, _bias, _mask, d = RR.gr_values(case)
    d_xt, e_xt, d_f, e_f = RR.gr_bwd_fp64(d, xt, feats)
    g_xt, g_f = RR.gr_bwd_f32(d, xt, feats, variant)
    return max(_ratio(g_xt, d_xt, e_xt), _ratio(g_f, d_f, e_f))


def _ratio(got, want, bound):
    """region_ref.ratio, with a NaN or an infinity where the reference is finite counted as infinitely far"""
    got = np.asarray(got, dtype=np.float64)
    if not np.isfinite(got[np.isfinite(np.asarray(want, dtype=np.float64))]).all():
        return float("inf")
    return ratio(got, want, bound)[0]


ENTRY_POINTS = {
    "cvc_class_softmax_fwd": (softmax_ratio, RR.SOFTMAX_CASES, RR.SOFTMAX_MUTANTS),
    "cvc_layernorm_cat_fwd": (ln_ratio, RR.LN_CASES, RR.LN_MUTANTS),
    "cvc_frame_embed_fwd": (fe_ratio, RR.FE_CASES, RR.FE_MUTANTS),
    "cvc_attn_nll_fwd": (nll_fwd_ratio, RR.NLL_CASES, RR.NLL_FWD_MUTANTS),
    "cvc_attn_nll_bwd": (nll_bwd_ratio, RR.NLL_CASES, RR.NLL_BWD_MUTANTS),
    "cvc_grounder_fwd": (gr_fwd_ratio, RR.GR_CASES, RR.GR_FWD_MUTANTS),
    "cvc_grounder_bwd": (gr_bwd_ratio, RR.GR_CASES, RR.GR_BWD_MUTANTS),
}


@pytest.mark.parametrize("entry", list(ENTRY_POINTS))
def test_restatement_stays_within_the_bound_without_k(entry):
    fn, cases, _m = ENTRY_POINTS[entry]
    rs = [fn(c) for c in cases]
    worst = int(np.argmax(rs))
    print("%s: float32 restatement, worst |err| / bound over %d cases = %.3f (x 1 / K = %.3f) at %s" % (entry, len(cases), rs[worst], rs[worst] / K, cases[worst]))
    assert max(rs) <= 1.0, (entry, cases[worst], rs[worst])


@pytest.mark.parametrize("entry,variant", [(e, v) for e, (_f, _c, ms) in ENTRY_POINTS.items() for v in ms])
def test_bounds_notice_a_wrong_kernel(entry, variant):
    fn, cases, mutants = ENTRY_POINTS[entry]
    assert len(mutants) >= 3
    rs = [fn(c, variant) / K for c in cases]
    worst = int(np.argmax(rs))
    print("%s / %s: %d of %d cases outside K x bound, the farthest %.3g x (K x bound) at %s" % (entry, variant, sum(r > 1 for r in rs), len(cases), rs[worst], cases[worst]))
    assert rs[worst] > 1.0, (entry, variant, rs[worst])


@pytest.mark.parametrize("variant", RR.EMBED_MUTANTS)
def test_exact_embedding_notices_a_wrong_kernel(variant):
    assert len(RR.EMBED_MUTANTS) >= 3
    hit = 0
    for case in RR.EMBED_CASES:
        table, idx, drop = RR.embed_values(case)
        want, got = RR.embed_ref(table, idx, drop), RR.embed_ref(table, idx, drop, variant)
        hit += not np.array_equal(want.view(np.uint32), got.view(np.uint32))
    assert hit >= 1


# ------------------------------------------------------------------------------------------------ the tables say what the issue asks
def test_case_tables_cover_the_edges():
    shapes = {tuple(c[:4]) for c in RR.SOFTMAX_CASES}
    assert shapes == set(RR.SOFTMAX_SHAPES)
    for shape in ((2, 15, 7, 7), (2, 17, 65, 72)):                    # the full cross of bias / pad / out_rows
        assert len({(c.bias, c.pad, c.rows) for c in RR.SOFTMAX_CASES if tuple(c[:4]) == shape}) == 8
    for c in RR.SOFTMAX_CASES:
        if c.pad and c.B >= 2:
            pad = RR.pad_mask(c.B, c.N, tuple(c))
            assert pad[0].all() and not pad[1].any()
    assert {c.widths for c in RR.LN_CASES} == set(RR.LN_WIDTHS) and {c.rows for c in RR.LN_CASES} == {1, 5}
    for case in RR.FE_CASES:
        _y0, _b0, _y1, _b1, scale, shift = RR.fe_values(case)
        c0 = case[1]
        for side in (scale[:c0], scale[c0:]):
            assert (side < 0).any() and (side == 0).any() and (side > 0).any()
        assert (shift < 0).any() and (shift > 0).any()
    for case in RR.NLL_CASES:
        x, tg = RR.nll_values(case)
        rows = tg.reshape(-1, case[2])
        if len(rows) >= 2:
            assert rows.all(axis=1).any() and ((x[0].reshape(rows.shape) == RR.MIN_VALUE) & rows).any()
        if len(rows) >= 3:
            assert not rows[0].any()
    assert sorted({-(-c[2] // 4) for c in RR.GR_CASES}) == [1, 2, 5, 16, 17, 33] and {c[3] for c in RR.GR_CASES} >= {252, 256, 260}
