"""cvc_cider_d and cvc_scst_weights (csrc/cider.hip) against the fp64 restatement of CIDEr-D (tests/cider_ref.py).

Tolerance of the reward: the reference is cider_ref in fp64; the yardstick is the SAME helper evaluated in fp32 on the CPU, in this
test; the kernel's largest error may be 4 x the yardstick's largest error (another summation order, a few ulp in sqrtf / expf), with a
floor of 2^-20 (one fp32 ulp of the largest reward, 10).  Every test prints its figures before it asserts."""
import numpy as np
import pytest
import torch

import cider_ref as R

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -20
CASES = [(1, 1, 1, 1, 5), (5, 5, 4, 1, 7), (7, 1, 20, 3, 23), (6, 3, 63, 2, 23), (320, 5, 20, 1, 997)]      # (rows, S, T, Rmax, V)
_CACHE = {}


def _caption(rng, T, V, garbage):
    """n words drawn from a Zipf-like law over 1 .. V - 1, then the end mark if it fits; behind it zeros or (garbage) more words"""
    p = 1.0 / np.arange(1, V, dtype=np.float64)
    n = int(rng.integers(0, T + 1))
    c = rng.choice(np.arange(1, V), size=T, p=p / p.sum()).astype(np.int64)
    if n < T:
        c[n] = 0
        if not garbage:
            c[n + 1:] = 0
    return c


def _case(rows, S, T, Rmax, V):
    """-> dict(cand, refs, nref, table, df, n_doc, ref64 (scores, parts), ref32): built once per case, shared and left unchanged"""
    key = (rows, S, T, Rmax, V)
    if key in _CACHE:
        return _CACHE[key]
    from cvc.cider import CiderD
    rng = np.random.default_rng(rows * 1000 + T)
    clips = rows // S
    train = [_caption(rng, T, V, False) for _ in range(200 if V < 100 else 2000)]
    refs = np.stack([np.stack([_caption(rng, T, V, bool(rng.integers(0, 2))) for _ in range(Rmax)]) for _ in range(clips)])
    nref = rng.integers(1, Rmax + 1, clips).astype(np.int32)
    cand = np.stack([_caption(rng, T, V, True) for _ in range(rows)])
    for r in range(rows):
        if r % 3 == 2:                                   # a third: one of the clip's references with one word changed
            c = r // S
            cand[r] = refs[c, int(rng.integers(0, nref[c]))]
            cand[r, int(rng.integers(0, T))] = int(rng.integers(0, V))
    df, n_doc = R.doc_freq(train)
    out = dict(cand=cand, refs=refs, nref=nref, table=CiderD.from_captions(train), df=df, n_doc=n_doc,
               ref64=R.score_batch(cand, refs, nref, df, n_doc), ref32=R.score_batch(cand, refs, nref, df, n_doc, dt=np.float32))
    _CACHE[key] = out
    return out


def _score(table, cand, refs, nref, dev, **kw):
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)
    return table.score(t(cand, torch.int64), t(refs, torch.int64), t(nref, torch.int32), **kw)


def _check(label, got, parts, ref64, ref32):
    err = float(np.abs(got - ref64[0]).max())
    err_p = float(np.abs(parts - ref64[1]).max())
    yard, yard_p = float(np.abs(ref32[0] - ref64[0]).max()), float(np.abs(ref32[1] - ref64[1]).max())
    bound, bound_p = max(4.0 * yard, FLOOR), max(4.0 * yard_p, FLOOR)          # (the per-order parts: the same rule on their own yardstick)
    print(f"[cider] {label}: kernel max |err| reward {err:.3e} (fp32 yardstick {yard:.3e}, bound {bound:.3e}), per-order {err_p:.3e} "
          f"(yardstick {yard_p:.3e}, bound {bound_p:.3e}); mean reward {ref64[0].mean():.4f}, non-zero rows "
          f"{np.count_nonzero(ref64[0])}/{len(got)}")
    assert err <= bound and err_p <= bound_p, (label, err, err_p, yard, yard_p)


@pytest.mark.parametrize("rows,S,T,Rmax,V", CASES)
def test_cider_d_random_cases_vs_fp64(rows, S, T, Rmax, V):
    dev = torch.device("cuda:0")
    c = _case(rows, S, T, Rmax, V)
    # not vacuous: at least 90 % of the rows have a non-zero reference reward
    assert np.count_nonzero(c["ref64"][0]) >= 0.9 * rows, (np.count_nonzero(c["ref64"][0]), rows)
    got, parts = _score(c["table"], c["cand"], c["refs"], c["nref"], dev, per_order=True)
    got, parts = got.cpu().double().numpy(), parts.cpu().double().numpy()
    _check(str((rows, S, T, Rmax, V)), got, parts, c["ref64"], c["ref32"])
    np.testing.assert_array_equal(got.astype(np.float32), (0.25 * ((parts[:, 0].astype(np.float32) + parts[:, 1].astype(np.float32)) +
                                                                  (parts[:, 2].astype(np.float32) + parts[:, 3].astype(np.float32)))))


def test_cider_d_hand_made_rows():
    """one candidate per clip (T = 8, V = 23, Rmax = 3): the edge cases of the definition, each against fp64 and some exactly"""
    from cvc.cider import CiderD
    dev = torch.device("cuda:0")
    T, V, Rmax = 8, 23, 3
    rng = np.random.default_rng(7)
    train = [_caption(rng, T, 20, False) for _ in range(200)]           # words 20, 21, 22 never occur: n-grams absent from the table
    df, n_doc = R.doc_freq(train)
    Z = [0] * T
    full = [3, 4, 5, 6, 7, 8, 9, 10]
    rows = [
        ("first word EOS", [0, 5, 6, 7, 0, 0, 0, 0], [[2, 3, 0] + [0] * 5], 1),
        ("first word EOS, reference too", [0, 5, 6, 7, 0, 0, 0, 0], [Z], 1),
        ("no EOS in T steps", [2, 3, 4, 5, 2, 3, 4, 5], [[2, 3, 4, 5, 0, 0, 0, 0]], 1),
        ("identical, full length", full, [full], 1),
        ("identical, L = 2", [4, 0] + [0] * 6, [[4, 0] + [9] * 6], 1),
        ("one word T times vs a reference holding it once", [6] * T, [[2, 6, 3, 0] + [0] * 4], 1),
        ("nref = 0", full, [full], 0),
        ("n-grams absent from the table", [20, 21, 22, 20, 0, 0, 0, 0], [[20, 21, 22, 21, 0, 0, 0, 0]], 1),
        ("references of other lengths", [2, 3, 4, 0] + [0] * 4, [[2, 3, 4, 5, 6, 7, 8, 0], [2, 0] + [0] * 6, [2, 3, 4, 0] + [0] * 4], 3),
        ("nref = 2 of 3", [2, 3, 4, 0] + [0] * 4, [[2, 3, 4, 5, 6, 7, 8, 0], [2, 0] + [0] * 6, [2, 3, 4, 0] + [0] * 4], 2),
    ]
    cand = np.array([r[1] for r in rows], dtype=np.int64)
    refs = np.zeros((len(rows), Rmax, T), dtype=np.int64)
    for i, r in enumerate(rows):
        refs[i, :len(r[2])] = np.array(r[2], dtype=np.int64)
    nref = np.array([r[3] for r in rows], dtype=np.int32)
    table = CiderD.from_captions(train)
    ref64, ref32 = R.score_batch(cand, refs, nref, df, n_doc), R.score_batch(cand, refs, nref, df, n_doc, dt=np.float32)
    got, parts = _score(table, cand, refs, nref, dev, per_order=True)
    got, parts = got.cpu().double().numpy(), parts.cpu().double().numpy()
    for i, r in enumerate(rows):
        print(f"[cider] hand-made {r[0]!r}: kernel {got[i]:.7f}, fp64 {ref64[0][i]:.7f}")
    _check("hand-made", got, parts, ref64, ref32)
    name = [r[0] for r in rows]
    assert got[name.index("nref = 0")] == 0.0 and not parts[name.index("nref = 0")].any()
    assert abs(ref64[0][name.index("identical, full length")] - 10.0) < 1e-12 and abs(got[name.index("identical, full length")] - 10.0) <= 4 * FLOOR
    assert abs(ref64[0][name.index("identical, L = 2")] - 5.0) < 1e-12 and abs(got[name.index("identical, L = 2")] - 5.0) <= 4 * FLOOR
    assert parts[name.index("identical, L = 2"), 2:].max() == 0.0
    # the Gaussian term and the clipping bite: below the identical pair's 10, above 0
    for n_ in ("one word T times vs a reference holding it once", "references of other lengths", "no EOS in T steps",
               "n-grams absent from the table"):
        assert 0.0 < got[name.index(n_)] < 10.0, n_
    assert got[name.index("nref = 2 of 3")] != got[name.index("references of other lengths")]


def test_cider_d_deterministic_and_independent_of_the_other_rows():
    dev = torch.device("cuda:0")
    rows, S, T, Rmax, V = CASES[-1]
    c = _case(rows, S, T, Rmax, V)
    a, pa = _score(c["table"], c["cand"], c["refs"], c["nref"], dev, per_order=True)
    b, pb = _score(c["table"], c["cand"], c["refs"], c["nref"], dev, per_order=True)
    assert torch.equal(a, b) and torch.equal(pa, pb)
    for r in (0, 1, 77, 163, 319):
        clip = r // S
        one = _score(c["table"], c["cand"][r:r + 1], c["refs"][clip:clip + 1], c["nref"][clip:clip + 1], dev)
        assert torch.equal(one, a[r:r + 1]), r


def test_both_launches_replay_from_a_graph_bit_for_bit():
    from cvc import hip
    dev = torch.device("cuda:0")
    rows, S, T, Rmax, V = CASES[-1]
    c = _case(rows, S, T, Rmax, V)
    table = c["table"].to(dev)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)
    cand, refs, nref = t(c["cand"], torch.int64), t(c["refs"], torch.int64), t(c["nref"], torch.int32)
    rng = np.random.default_rng(5)
    other = t(np.stack([_caption(rng, T, V, True) for _ in range(rows)]), torch.int64)

    def both(x):
        reward = hip.cider_d(x, refs, nref, table.keys, table.idf, table.idf_unseen, table.sigma)
        adv, w = hip.scst_weights(reward, None, S, x, t_major=True)
        return reward, adv, w
    static = cand.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        both(static)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = both(static)
    for x in (other, cand):
        static.copy_(x)
        g.replay()
        for got, want in zip(out, both(x)):
            assert torch.equal(got, want)
    assert not torch.equal(both(other)[0], both(cand)[0])


@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("t_major", [False, True])
def test_scst_weights(S, t_major):
    """adv against fp64 within (S + 2) 2^-24 sum |r| over the terms of the row's clip (its samples' rewards; with S = 1 the reward and
    the baseline it is compared with); w == adv x the text mask, exactly"""
    from cvc import hip
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(10 * S + t_major)
    T, clips = 7, 27
    rows = clips * S                              # 27 and 135 rows: less than one block of threads, and more than two
    cand = np.stack([_caption(rng, T, 13, True) for _ in range(rows)])
    cand[0] = [0, 4, 5, 0, 6, 7, 8]               # EOS first: one live step
    cand[1] = [3, 4, 5, 6, 7, 8, 9]               # no EOS: all T steps
    reward = (rng.random(rows) * 10).astype(np.float32)
    reward[rows // 2] = 0.0
    base = (rng.random(clips) * 10).astype(np.float32) if S == 1 else None
    adv, w = hip.scst_weights(torch.from_numpy(reward).to(dev), None if base is None else torch.from_numpy(base).to(dev), S,
                              torch.from_numpy(cand).to(dev), t_major=t_major)
    want, mag = R.advantages(reward, S, base)
    err = np.abs(adv.cpu().double().numpy() - want)
    bound = (S + 2) * 2.0 ** -24 * mag
    print(f"[scst_weights] S={S} t_major={t_major}: max |adv err| {err.max():.3e}, smallest slack {(bound - err).min():.3e}")
    assert (err <= bound).all()
    mask = torch.from_numpy(R.text_mask(cand)).to(dev)
    assert mask[0].sum() == 1 and mask[1].all()
    want_w = adv[:, None] * mask.to(adv.dtype)
    assert w.shape == ((T, rows) if t_major else (rows, T))
    assert torch.equal(w.t() if t_major else w, want_w)
