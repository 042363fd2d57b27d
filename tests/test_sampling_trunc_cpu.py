"""Top-k / nucleus truncated sampling without a GPU: properties of the fp64 reference (tests/sample_trunc_ref.py), the new building
block in the library's block table, its host-side argument checks, the engine's refusals and the CLI's flags."""
import os
import re

import numpy as np
import pytest
import torch

from cvc import synth
from oracle import ref_cpu as O
import sample_oracle as S
import sample_trunc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNK = synth.UNK_IDX


def logits(rows=12, V=50, seed=7, scale=1.5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(rows, V, generator=g) * scale


def kept_sets(z, tau, k, p, tol=0.0):
    orders, j_lo, j_hi = R.truncate(z, tau, UNK, k, p, tol=tol)
    assert (j_lo == j_hi).all() or tol > 0
    return [set(o[:j].tolist()) for o, j in zip(orders, j_lo)], orders, j_lo


def test_top_k_1_is_the_arg_max_without_unk():
    z = logits()
    z[::2, UNK] = 9.0                                        # UNK leads half of the rows: it counts neither towards k nor is kept
    noise = S.gumbel_noise(3, 1, 0, z.shape[0], z.shape[1])
    orders, j_lo, j_hi = R.truncate(z, 1.0, UNK, 1, 1.0)
    assert (j_lo == 1).all() and (j_hi == 1).all()
    w, _ = R.select(z, noise, 1.0, UNK, orders, j_lo)
    zz = z.clone()
    zz[:, UNK] = -float("inf")
    assert np.array_equal(w, zz.argmax(1).numpy())


def test_no_truncation_is_the_plain_reference_sampler():
    z = logits()
    V = z.shape[1]
    noise = S.gumbel_noise(5, 2, 1, z.shape[0], V)
    w0, s0, _ = S.select(z, noise, 0.7, UNK)
    for k in (0, V - 1, V + 7):
        orders, j_lo, j_hi = R.truncate(z, 0.7, UNK, k, 1.0)
        assert (j_lo == V - 1).all() and (j_hi == V - 1).all()
        w, s = R.select(z, noise, 0.7, UNK, orders, j_lo)
        assert np.array_equal(w, w0)
    # the reference's scores are the product with the fp32 1 / tau the block is handed, S.select's the quotient: |z / tau| * 2^-24
    np.testing.assert_allclose(s[np.isfinite(s)], s0[np.isfinite(s0)], rtol=0, atol=1e-6)


def test_ties_with_the_kth_value_are_all_kept():
    z = logits(rows=4)
    for r in range(4):
        zz = z[r].clone()
        zz[UNK] = -float("inf")
        o = torch.argsort(zz, descending=True)
        z[r, o[5]] = z[r, o[4]]                              # the 6th word duplicates the 5th value
    _, _, j = kept_sets(z, 1.0, 5, 1.0)
    assert (j == 6).all()
    _, _, j4 = kept_sets(z, 1.0, 4, 1.0)
    assert (j4 == 4).all()


def test_kept_sets_are_nested_in_k_and_in_p():
    z = logits(rows=16, V=200)
    prev = None
    for k in (1, 2, 5, 17, 60, 150, 0):                      # 0 = off = everything
        sets, _, _ = kept_sets(z, 0.8, k, 1.0)
        if prev is not None:
            assert all(a <= b for a, b in zip(prev, sets)), k
        prev = sets
    prev = None
    for p in (1e-6, 0.1, 0.5, 0.9, 0.99, 1.0):
        sets, _, _ = kept_sets(z, 0.8, 0, p)
        if prev is not None:
            assert all(a <= b for a, b in zip(prev, sets)), p
        prev = sets
    for p in (0.3, 0.9):                                     # top-p after top-k: inside the top-k set, and inside the band's other end
        inner, _, _ = kept_sets(z, 0.8, 17, p)
        outer, _, _ = kept_sets(z, 0.8, 17, 1.0)
        assert all(a <= b for a, b in zip(inner, outer))
        orders, j_lo, j_hi = R.truncate(z, 0.8, UNK, 17, p)
        assert (j_lo <= j_hi).all() and (j_lo >= 1).all() and (j_hi <= 17).all()
    # the kept mass reaches p, and without its last value it does not
    orders, j_lo, _ = R.truncate(z, 0.8, UNK, 0, 0.9, tol=0.0)
    for r in range(z.shape[0]):
        e = np.exp(z[r, torch.from_numpy(orders[r])].double().numpy() * float(np.float32(1 / 0.8)))
        assert e[:j_lo[r]].sum() >= 0.9 * e.sum() > e[:j_lo[r] - 1].sum()


def test_one_step_distribution_of_the_truncated_reference():
    """4 000 rows per clip see the same logits and differ through the noise: counts against softmax(z / tau) renormalised over C2,
    and not one draw outside C2 (fixed seed: deterministic)."""
    d = synth.CONFIGS["tiny"]
    P, f = O.to_torch(synth.hot_path_state_dict(d, 99)), O.to_torch(synth.clip_features(d, 99))
    n, tau, k, p = 4000, 1.3, 20, 0.8
    with torch.no_grad():
        out, _, _, _, _ = O.decoder_step(P, O.embed(P, torch.zeros(d.B, dtype=torch.long)), f["fc_feats"], f["conv_feats"],
                                         f["p_conv_feats"], f["pool_feats"], f["p_pool_feats"], f["pnt_mask"][:, 1:],
                                         O.init_hidden(d.B, d.R))
        z = torch.nn.functional.linear(out, P["logit.weight"], P["logit.bias"])
    orders, j_lo, j_hi = R.truncate(z, tau, UNK, k, p)
    assert (j_lo == j_hi).all() and (j_lo < k).all()
    zr = z.repeat_interleave(n, 0)
    rep = lambda xs: [x for x in xs for _ in range(n)]
    word, _ = R.select(zr, S.gumbel_noise(2024, 1, 0, d.B * n, d.V), tau, UNK, rep(orders), np.repeat(j_lo, n))
    for b in range(d.B):
        c2 = orders[b][:j_lo[b]]
        counts = np.bincount(word[b * n:(b + 1) * n], minlength=d.V)
        assert counts[np.setdiff1d(np.arange(d.V), c2)].sum() == 0
        prob = np.zeros(d.V)
        prob[c2] = torch.softmax(z[b, torch.from_numpy(c2)].double() / tau, 0).numpy()
        stat, df = S.chi_square(counts, prob)
        assert stat < S.chi_square_critical(df), (b, stat, df)


def test_reference_sampler_flags_ambiguous_cutoffs_only_with_a_tolerance():
    d = synth.CONFIGS["tiny"]
    P, f = O.to_torch(synth.hot_path_state_dict(d, 99)), O.to_torch(synth.clip_features(d, 99))
    with torch.no_grad():
        seq, att, lp, scores, info = R.sample(P, f, d.T, UNK, 3, 0.8, 5, 1, top_k=10, top_p=0.9, tol=0.0)
        seq1, *_ = R.sample(P, f, d.T, UNK, 3, 0.8, 5, 1, top_k=1)
        seq_g, _, _, _ = O.greedy_sample(P, f, d.T, UNK, return_logprobs=True)
    assert info["unambiguous"].all() and (info["j_lo"] == info["j_hi"]).all() and (info["j_hi"] <= 10).all()
    assert seq.shape == (d.B * 3, d.T) and not (seq == UNK).any()
    assert np.isfinite(scores).sum(-1).max() <= 10
    assert torch.equal(seq1, seq_g.repeat_interleave(3, 0))                       # top_k = 1: the greedy decode, whatever the noise


def test_a_logit_tolerance_widens_the_band_only_where_values_are_that_close():
    z = torch.tensor([[5.0, 4.0, 3.0, 2.0, 1.0, 0.0, -1.0, -2.0]])
    unk = 7
    # well separated values: the band stays one point whatever the (small) tolerances
    for k, p in ((3, 1.0), (3, 0.9), (0, 0.9)):
        _, lo0, hi0 = R.truncate(z, 1.0, unk, k, p)
        _, lo1, hi1 = R.truncate(z, 1.0, unk, k, p, tol=3e-4, ztol=1e-4)
        assert lo0 == hi0 == lo1 == hi1, (k, p, lo0, hi0, lo1, hi1)
    # the 4th value within 2 ztol of the 3rd: in or out at k = 3; the 3rd itself may fall out too (band [2, 4])
    z[0, 3] = 3.0 - 1.5e-4
    _, lo, hi = R.truncate(z, 1.0, unk, 3, 1.0, ztol=1e-4)
    assert (int(lo[0]), int(hi[0])) == (2, 4)
    _, lo, hi = R.truncate(z, 1.0, unk, 3, 1.0)
    assert (int(lo[0]), int(hi[0])) == (3, 3)


def test_trunc_block_is_in_the_block_table_and_not_exported():
    """cvc_sample_select_trunc_parts: declared in include/cvc_hip_blocks.h, bound through cvc_block(), absent from the dynamic symbol
    table (the exported ABI stays include/cvc_hip.h); its host-side argument checks launch nothing."""
    import ctypes
    import subprocess
    import build_hip
    from cvc import hip
    so = build_hip.build(verbose=False)
    name = "cvc_sample_select_trunc_parts"
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cvc_hip_blocks.h")).read(), flags=re.S)
    lib = ctypes.CDLL(so)
    lib.cvc_block.restype = ctypes.c_void_p
    lib.cvc_block.argtypes = [ctypes.c_char_p]
    exported = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    assert re.search(r"\bint\s+" + name + r"\s*\(", src)
    assert lib.cvc_block(name.encode())
    assert name in hip.BLOCKS and name in hip.SIGNATURES
    assert len(hip.SIGNATURES[name]) == len(hip.SIGNATURES["cvc_sample_select_parts"]) + 4
    assert not re.search(r"\b" + name + r"\b", exported)
    fn = hip.lib().cvc_sample_select_trunc_parts
    fake = ctypes.c_void_p(16)
    call = lambda parts=fake, nparts=1, stride=0, V=50, inv_tau=1.0, k=0, p=1.0, state=fake, word=fake: fn(
        parts, nparts, stride, None, 4, V, 1, inv_tau, k, p, state, 0, word, 1, None, None, None, None)
    # the checks of cvc_sample_select_parts ...
    assert call(parts=None) == -1 and call(state=None) == -1 and call(word=None) == -1
    assert call(inv_tau=0.0) == -1 and call(inv_tau=float("inf")) == -1
    assert call(V=9000) == -2
    assert call(nparts=2, stride=10) == -1
    # ... and the truncation's own
    assert call(k=-1) == -1
    for p in (0.0, -0.5, 1.5, float("nan"), float("inf")):
        assert call(p=p) == -1, p
    assert call(k=3, p=float("nan")) == -1 and call(k=-1, p=0.5) == -1


def test_engine_refuses_bad_truncation_before_touching_the_gpu():
    from cvc.decode import DecodeEngine
    new = lambda **kw: DecodeEngine.__init__(object.__new__(DecodeEngine), None, {}, 4, 1, **kw)
    with pytest.raises(RuntimeError, match="top_k"):
        new(temperature=1.0, top_k=-1)
    with pytest.raises(RuntimeError, match="top_k"):
        new(temperature=1.0, top_k=2.5)
    with pytest.raises(RuntimeError, match="top_p"):
        new(temperature=1.0, top_p=0)
    with pytest.raises(RuntimeError, match="top_p"):
        new(temperature=1.0, top_p=1.5)
    with pytest.raises(RuntimeError, match="top_p"):
        new(temperature=1.0, top_p=float("nan"))
    with pytest.raises(RuntimeError, match="temperature"):
        new(top_k=5)
    with pytest.raises(RuntimeError, match="temperature"):
        new(top_p=0.9)
    with pytest.raises(RuntimeError, match="beam"):          # the sampling checks still come first for what they cover
        new(temperature=1.0, top_k=5, beam=3)


def test_cli_parses_the_truncation_flags():
    from cvc import sample as cvc_sample
    own, rest = cvc_sample.parse(["--temperature", "0.8", "--top_k", "40", "--top_p", "0.9", "--id", "x"])
    assert (own.temperature, own.top_k, own.top_p, own.sample_n, own.sample_seed) == (0.8, 40, 0.9, 5, 0) and rest == ["--id", "x"]
    own, rest = cvc_sample.parse(["--sample_n", "2"])
    assert (own.top_k, own.top_p) == (0, 1.0) and rest == []
    for bad in (["--top_k", "-1"], ["--top_p", "0"], ["--top_p", "1.5"]):
        with pytest.raises(SystemExit):
            cvc_sample.parse(bad)
    # the options of cvc.main know nothing of them: they are this module's own
    from cvc import opts
    import inspect
    assert "top_k" not in inspect.getsource(opts) and "top_p" not in inspect.getsource(opts)
