"""Self-critical training without replacement, everything that needs no GPU: the fp64 restatement of the rule (tests/wor_ref.py) on
the stochastic-beam toy of tests/sbs_ref.py -- the estimator's two expectations, with and without the root-key correction --, its
algebraic limits, and the surface of the block, the wrapper, the flag, the trainer's refusals and the documentation."""
import ctypes
import os
import subprocess
import types

import numpy as np
import pytest
import torch

import sbs_ref as S
import wor_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z_OK, Z_OFF = 4.5, 10.0


# ------------------------------------------------------------------ the estimator on the toy
@pytest.mark.parametrize("name", list(W.TOY_CASES))
def test_toy_statistics_need_the_root_key_correction(name):
    """V = 4, T = 3, beam 4 (S = 3), 50 000 clips: the unnormalised sum wgt f within 4.5 of its own standard errors of E f, sum adv h
    within 4.5 of sum p f h - (sum p f)(sum p h) (exact enumeration); with the threshold as the engine leaves it (lambda = -G_S) both
    are more than 10 standard errors off."""
    c = W.toy_case(name)
    assert c["hist"].shape == (W.TOY_TRIALS, 4, 3) and c["live"].all()
    z = {}
    for corrected in (True, False):
        est, gh = W.toy_statistics(c["hist"], c["logq"], c["G"], c["a"], c["seqs"], c["f"], c["h"], corrected=corrected)
        z[corrected] = (W.z_score(est, c["Ef"]), W.z_score(gh, c["cov"]))
    print(f"[wor toy] {name}: {len(c['seqs'])} captions, E f = {c['Ef']:.4f}, gradient term = {c['cov']:.4f}; standard errors off: "
          f"corrected {z[True][0]:+.2f} / {z[True][1]:+.2f}, uncorrected {z[False][0]:+.2f} / {z[False][1]:+.2f}")
    assert abs(z[True][0]) <= Z_OK and abs(z[True][1]) <= Z_OK
    assert abs(z[False][0]) > Z_OFF and abs(z[False][1]) > Z_OFF


def test_a_is_a_unit_exponential_and_differs_per_clip_and_call():
    a = W.root_from_seed(12, 1, 50000)
    assert (a > 0).all() and abs(a.mean() - 1.0) < 5 / np.sqrt(50000) and abs((a > 1).mean() - np.exp(-1)) < 5 * 0.5 / np.sqrt(50000)
    assert not np.array_equal(a, W.root_from_seed(12, 2, 50000)) and not np.array_equal(a, W.root_from_seed(13, 1, 50000))
    for h in (0, 0xFFFFFFFF):                                  # the extreme hash values: a stays finite and > 0, in fp32 too
        for dt in (np.float64, np.float32):
            v = W.root_exponential(np.array([h], dtype=np.uint32), dt)[0]
            assert np.isfinite(v) and v > 0 and v - dt(1) > -1


def test_a_toy_the_beam_exhausts():
    """V = 2, T = 2: three captions, S = 3, beam 4 -- slot S is dead in every trial, the weights are the probabilities, and the
    estimator is exact per trial in both forms (the normalised adv carries the factor n_live = 3, taken out here)."""
    trials = 400
    table = S.toy_table(2, 2, 9)
    hist, live, G, logq, _ = S.toy_run(table, trials, 4, 1.0, 21, call=1)
    seqs, probs = S.toy_sequences(table, 1.0)
    assert len(seqs) == 3 and live[:, :3].all() and not live[:, 3].any()
    rng = np.random.default_rng(3)
    f, h = rng.random(3) * 10, rng.normal(size=3)
    Ef, cov = W.exact_values(probs, f, h)
    index = {s: i for i, s in enumerate(seqs)}
    idx = np.array([[index[tuple(int(w) for w in hist[n, i])] for i in range(3)] for n in range(trials)])
    a = W.root_from_seed(21, 1, trials)
    for normalize in (False, True):
        r = W.weights(f[idx], logq, G, a, normalize=normalize)
        assert np.isinf(r["lam"]).all() and (r["n_live"] == 3).all()
        np.testing.assert_allclose(r["wgt"], probs[idx], rtol=0, atol=1e-12)
        np.testing.assert_allclose(r["est"], Ef, rtol=0, atol=1e-12)
        gh = (r["adv"] * h[idx]).sum(1) / (3 if normalize else 1)
        np.testing.assert_allclose(gh, cov, rtol=0, atol=1e-12)


# ------------------------------------------------------------------ algebraic limits
def _clip(S_, logq, kt=-3.0, seed=0):
    rng = np.random.default_rng(seed)
    f = rng.random((4, S_)) * 10
    lq = np.full((4, S_ + 1), float(logq))
    G = np.sort(lq + rng.gumbel(size=lq.shape), 1)[:, ::-1].copy()
    G[:, S_] = kt
    return f, lq, G, rng.exponential(size=4)


@pytest.mark.parametrize("S_", [2, 5, 7])
def test_tiny_probabilities_give_the_leave_one_out_advantage(S_):
    f, lq, G, a = _clip(S_, -60.0)
    r = W.weights(f, lq, G, a, normalize=True)
    np.testing.assert_allclose(r["adv"], W.leave_one_out(f), rtol=0, atol=1e-9)
    np.testing.assert_allclose(r["wgt"], 1.0 / S_, rtol=0, atol=1e-9)
    np.testing.assert_allclose(r["est"], f.mean(1), rtol=0, atol=1e-9)


def test_probabilities_that_underflow_stay_finite_in_the_normalised_form():
    f, lq, G, a = _clip(5, -150.0, kt=-120.0)
    lq[:, 1] = -140.0
    r = W.weights(f, lq, G, a, normalize=True)
    for k in ("adv", "wgt", "est"):
        assert np.isfinite(r[k]).all(), k
    np.testing.assert_allclose(r["wgt"].sum(1), 1.0, rtol=0, atol=1e-12)
    np.testing.assert_allclose(r["est"], (r["wgt"] * f).sum(1), rtol=0, atol=1e-12)
    assert (r["wgt"] > 0).all()
    u = W.weights(f, lq, G, a, normalize=False)                   # the unnormalised weights may be anything down to 0, never NaN
    assert np.isfinite(u["wgt"]).all() and np.isfinite(u["adv"]).all() and (u["wgt"] >= 0).all()


def test_one_live_row_has_no_advantage_and_dead_rows_weigh_nothing():
    f, lq, G, a = _clip(3, -2.0)
    G[:, 1:] = -np.inf                                            # rows 1, 2 and the threshold slot are dead
    r = W.weights(f, lq, G, a, normalize=True)
    assert (r["adv"] == 0).all() and (r["wgt"][:, 0] == 1).all() and (r["wgt"][:, 1:] == 0).all() and (r["n_live"] == 1).all()
    np.testing.assert_array_equal(r["est"], f[:, 0])
    lq[:, 0] = 0.0                                                # the clip's only caption has probability 1
    u = W.weights(f, lq, G, a, normalize=False)
    assert (u["adv"] == 0).all() and (u["wgt"][:, 0] == 1).all()
    G[:, 0] = -np.inf
    z = W.weights(f, lq, G, a, normalize=True)
    assert not z["adv"].any() and not z["wgt"].any() and not z["est"].any()


def test_threshold_limits_and_the_inclusion_branches():
    a = np.array([0.3, 1.0, 2.5])
    np.testing.assert_allclose(W.threshold(np.zeros(3), a), np.log(a), rtol=0, atol=1e-15)       # kt = 0: lambda = log a
    np.testing.assert_array_equal(W.threshold(np.full(3, -np.inf), a), np.inf)
    np.testing.assert_allclose(W.threshold(np.full(3, -4.0), np.ones(3)), 4.0)                    # a = 1: the engine's own root key
    kt = np.array([-0.5, -3.0, -40.0])
    np.testing.assert_allclose(np.exp(W.threshold(kt, a)), a - 1 + np.exp(-kt), rtol=1e-13)       # exp(-kappa) = a - 1 + exp(-kt)
    d = np.array([-800.0, -50.0, -1e-9, 0.0, 1e-9, 3.0, 800.0, np.inf])
    got = W.log_inclusion(d)
    assert got[0] == -800.0 and got[-1] == 0 and got[-2] == 0 and np.isfinite(got).all()
    mid = d[1:6]
    np.testing.assert_allclose(got[1:6], np.log(-np.expm1(-np.exp(mid))), rtol=1e-13)
    cand = np.array([[3, 0, 5], [4, 4, 4], [0, 0, 1]])
    adv = np.array([1.5, -2.0, 0.25], dtype=np.float32)
    np.testing.assert_array_equal(W.token_weights(adv, cand), np.array([[1.5, 1.5, 0], [-2, -2, -2], [0.25, 0, 0]], dtype=np.float32))
    np.testing.assert_array_equal(W.token_weights(adv, cand, t_major=True), W.token_weights(adv, cand).T)


# ------------------------------------------------------------------ surface
def test_block_declared_listed_bound_and_not_exported():
    import re
    import build_hip
    from cvc import hip
    from test_cabi import declared_functions, BLOCKS_H
    n = "cvc_scst_weights_wor"
    lib = hip.lib()
    lib.cvc_block.restype = ctypes.c_void_p
    out = subprocess.check_output(["nm", "-D", "--defined-only", build_hip.build(verbose=False)], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert n in declared_functions(BLOCKS_H) and n in hip.BLOCKS and n in hip.SIGNATURES and len(hip.SIGNATURES[n]) == 15
    assert lib.cvc_block(n.encode()) and n not in exported
    header = open(os.path.join(ROOT, "include", "cvc_hip_blocks.h")).read()
    sites = {k: int(v, 16) for k, v in re.findall(r"#define (CVC_\w+_SITE) (0x[0-9A-Fa-f]+)u", header)}
    assert sites["CVC_WOR_SITE"] == W.WOR_SITE
    from cvc import dropout
    taken = set(dropout._SITES.values())
    for t in range(256):
        taken |= {dropout.site_id("out_a.%d" % t), dropout.site_id("out_c.%d" % t)}
    taken |= {s + 64 * g for s in list(taken) for g in range(64)}
    for k, v in sites.items():
        if k != "CVC_WOR_SITE":
            taken |= {v + t for t in range(65)}
    assert W.WOR_SITE not in taken
    for word in ("exp(-kappa) = a - 1 + exp(-kt)", "log1p((a - 1) * exp(kt))", "n_live", "THIS COMMENT IS THE DEFINITION"):
        assert word in header, word


def test_bad_arguments_return_badarg_before_any_launch():
    from cvc import hip
    lib = hip.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)                    # non-null; never dereferenced: every call below is refused on the host

    def wor(reward=p, logq=p, G=p, state=p, rows=6, per=3, cand=p, T=5, adv=p, wgt=p, est=p, w=p):
        return lib.cvc_scst_weights_wor(reward, logq, G, state, rows, per, cand, T, 0, 1, adv, wgt, est, w, None)
    for name in ("reward", "logq", "G", "state", "cand", "adv", "wgt", "est", "w"):
        assert wor(**{name: None}) == -1, name
    assert wor(per=1, rows=6) == -1 and wor(per=0) == -1 and wor(per=8, rows=16) == -1
    assert wor(rows=7) == -1 and wor(rows=0) == -1 and wor(T=0) == -1
    assert bytes(buf) == b"\0" * 64


def test_wrapper_refuses_shapes_that_do_not_fit_and_cpu_tensors():
    from cvc import hip
    B, S_, T = 2, 3, 4
    ok = dict(reward=torch.zeros(B * S_), logq=torch.zeros(B, S_ + 1), G=torch.zeros(B, S_ + 1), state=torch.zeros(4, dtype=torch.int32),
              cand=torch.zeros(B * S_, T, dtype=torch.int64))
    call = lambda kw: hip.scst_weights_wor(kw["reward"], kw["logq"], kw["G"], kw["state"], S_, kw["cand"])
    for bad in (dict(reward=torch.zeros(5)), dict(logq=torch.zeros(B, S_)), dict(G=torch.zeros(B, S_)), dict(state=torch.zeros(3, dtype=torch.int32)),
                dict(cand=torch.zeros(B * S_ + 1, T, dtype=torch.int64)), dict(cand=torch.zeros(B * S_ * T, dtype=torch.int64))):
        with pytest.raises(RuntimeError, match="do not fit"):
            call({**ok, **bad})
    with pytest.raises(RuntimeError, match="GPU"):                       # no CPU fallback
        call(ok)


def test_flag_lives_in_main_not_in_opts():
    from cvc import main as cvc_main
    from cvc import opts as cvc_opts
    assert cvc_main.build_parser().parse_args(["--scst_wor"]).scst_wor is True
    assert cvc_main.build_parser().parse_args([]).scst_wor is False
    assert "scst_wor" not in vars(cvc_opts.build_parser().parse_args([]))
    with pytest.raises(SystemExit):
        cvc_opts.build_parser().parse_args(["--scst_wor"])


@pytest.mark.parametrize("S_,ok", [(1, False), (2, True), (7, True), (8, False)])
def test_trainer_refuses_sample_counts_the_estimator_cannot_take(S_, ok):
    from cvc import trainer as tr
    opts = types.SimpleNamespace(att_model="cyclical", batch_size=2, seq_per_img=1, disp_interval=1, hip_graph=0, scst_after=0,
                                 scst_wor=True, scst_samples=S_)
    if ok:
        assert tr.Trainer(opts, None, torch.nn.Linear(1, 1), None, [], None).scst_wor
        return
    with pytest.raises(RuntimeError, match="scst_samples"):
        tr.Trainer(opts, None, torch.nn.Linear(1, 1), None, [], None)
    opts.scst_wor = False                                            # without the flag the count is no concern of the trainer's
    t = tr.Trainer(opts, None, torch.nn.Linear(1, 1), None, [], None)
    t.scst_wor = True                                                # switched on later: the step itself refuses, before any work
    with pytest.raises(RuntimeError, match="scst_samples"):
        t.scst_step_prepared({})


def test_design_has_the_section_and_names_the_correction():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### Self-critical training without replacement" in text
    sec = text.split("### Self-critical training without replacement")[1].split("\n### ")[0]
    for word in ("root key", "exp(−κ) = a − 1 + exp(−κ̃)", "biased", "Rao-Blackwell", "cvc_scst_weights_wor", "q_τ", "--scst_wor"):
        assert word in sec, word
    assert "scst_wor" in open(os.path.join(ROOT, "README.md")).read()
