"""cvc_caption_overlap (csrc/overlap.hip; cvc.metrics.overlap) against the restatement of BLEU and ROUGE-L (tests/overlap_ref.py).

The integers (the ten BLEU statistics, the LCS lengths) must EQUAL the restatement's.  Tolerance of bleu and rouge, by the convention of
tests/test_gpu_cider.py: the reference is the restatement in fp64; the yardstick is the SAME helper evaluated in fp32 on the CPU; the
kernel's largest error may be 4 x the yardstick's largest error, with a floor of 2^-23 (one fp32 ulp at the scores' maximum, 1).
Every test prints its figures before it asserts."""
import ctypes

import numpy as np
import pytest
import torch

import overlap_ref as R

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -23
BADARG = -1                  # CVC_E_BADARG (include/cvc_hip.h)
CASES = [(1, 1, 1, 1, 5), (5, 5, 4, 1, 7), (7, 1, 20, 3, 23), (6, 3, 63, 2, 23), (320, 5, 20, 1, 997)]      # (rows, S, T, Rmax, V)
# the generator's seed per case: chosen (from the restatement alone) so that every case with T >= 4 holds a row with correct_4 > 0,
# a row where clipping bites and a row with Lc < ref_len -- test_random_cases asserts that before it looks at the kernel
SEEDS = {(1, 1, 1, 1, 5): 1001, (5, 5, 4, 1, 7): 5012, (7, 1, 20, 3, 23): 7020, (6, 3, 63, 2, 23): 6063, (320, 5, 20, 1, 997): 320020}
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


def _generate(rows, S, T, Rmax, V, seed):
    rng = np.random.default_rng(seed)
    clips = rows // S
    refs = np.stack([np.stack([_caption(rng, T, V, bool(rng.integers(0, 2))) for _ in range(Rmax)]) for _ in range(clips)])
    nref = rng.integers(1, Rmax + 1, clips).astype(np.int32)
    cand = np.stack([_caption(rng, T, V, True) for _ in range(rows)])
    for r in range(rows):
        if r % 3 == 2:                                   # a third: one of the clip's references with one word changed
            c = r // S
            cand[r] = refs[c, int(rng.integers(0, nref[c]))]
            cand[r, int(rng.integers(0, T))] = int(rng.integers(0, V))
    return cand, refs, nref


def _case(rows, S, T, Rmax, V):
    """-> dict(cand, refs, nref, ref64, ref32): built once per case, shared and left unchanged"""
    key = (rows, S, T, Rmax, V)
    if key not in _CACHE:
        cand, refs, nref = _generate(rows, S, T, Rmax, V, SEEDS[key])
        _CACHE[key] = dict(cand=cand, refs=refs, nref=nref, ref64=R.score_batch(cand, refs, nref),
                           ref32=R.score_batch(cand, refs, nref, dt=np.float32))
    return _CACHE[key]


def _t(a, dev, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)


def _run(cand, refs, nref, dev, **kw):
    from cvc import metrics
    return metrics.overlap(_t(cand, dev, torch.int64), _t(refs, dev, torch.int64), _t(nref, dev, torch.int32), want_lcs=True, **kw)


def _check(label, out, ref64, ref32):
    np.testing.assert_array_equal(out["stats"].cpu().numpy().astype(np.int64), ref64["stats"], err_msg=label)
    np.testing.assert_array_equal(out["lcs"].cpu().numpy().astype(np.int64), ref64["lcs"], err_msg=label)
    assert out["stats"].dtype == torch.int32 and out["lcs"].dtype == torch.int32
    for k in ("bleu", "rouge"):
        got = out[k].cpu().double().numpy()
        err = float(np.abs(got - ref64[k]).max())
        yard = float(np.abs(ref32[k] - ref64[k]).max())
        bound = max(4.0 * yard, FLOOR)
        print(f"[overlap] {label}: {k} kernel max |err| {err:.3e} (fp32 yardstick {yard:.3e}, bound {bound:.3e}); mean {ref64[k].mean():.4f}, "
              f"non-zero {np.count_nonzero(ref64[k])}/{ref64[k].size}")
        assert err <= bound, (label, k, err, yard)


@pytest.mark.parametrize("rows,S,T,Rmax,V", CASES)
def test_random_cases(rows, S, T, Rmax, V):
    dev = torch.device("cuda:0")
    c = _case(rows, S, T, Rmax, V)
    st = c["ref64"]["stats"]
    kinds = (int((st[:, 3] > 0).sum()), int(c["ref64"]["clip"].sum()), int((st[:, 8] < st[:, 9]).sum()))
    print(f"[overlap] {(rows, S, T, Rmax, V)}: rows with correct_4 > 0: {kinds[0]}, where clipping bites: {kinds[1]}, with Lc < ref_len: {kinds[2]}")
    if T >= 4:
        assert min(kinds) >= 1, kinds
    _check(str((rows, S, T, Rmax, V)), _run(c["cand"], c["refs"], c["nref"], dev), c["ref64"], c["ref32"])


def test_hand_made_rows():
    """one candidate per clip, T = 63, Rmax = 2: the edge cases of the definition"""
    dev = torch.device("cuda:0")
    T, Rmax = 63, 2
    pad = lambda w, fill=0: list(w) + [fill] * (T - len(w))
    perm = list(range(101, 101 + T))
    sent = [5, 6, 7, 8, 9, 6, 7, 0]
    rows = [
        ("Lc = 0", pad([0, 4, 5, 6]), [pad([4, 5, 6, 0])], 1),
        ("no end mark at T = 63", perm, [pad(perm[:40] + [0])], 1),
        ("identical to its reference", pad(sent, 9), [pad(sent, 3)], 1),
        ("one word 63 times against 63", [7] * T, [[7] * T], 1),
        ("reversed permutation of 63 distinct words", perm, [perm[::-1]], 1),
        ("nref = 0", pad(sent), [pad(sent)], 0),
        ("a reference with Lr = 0 beside a real one", pad([4, 5, 6, 7, 0]), [pad([0, 4, 5, 6, 7]), pad([4, 5, 9, 7, 0])], 2),
        ("length tie: Lc 5, references of 6 and 4 words", pad([1, 2, 3, 4, 5, 0]), [pad([1, 2, 3, 4, 5, 6, 0]), pad([1, 2, 3, 4, 0])], 2),
        ("ids 1, 257, 513, 65534 together", pad([1, 257, 513, 65534, 1, 257, 0]), [pad([257, 1, 513, 65534, 1, 0]), pad([1, 1, 513, 0])], 2),
        ("nref > Rmax is clamped", pad([4, 5, 6, 0]), [pad([4, 5, 0]), pad([4, 5, 6, 7, 0])], 5),
    ]
    name = [r[0] for r in rows]
    cand = np.array([r[1] for r in rows], dtype=np.int64)
    refs = np.zeros((len(rows), Rmax, T), dtype=np.int64)
    for i, r in enumerate(rows):
        refs[i, :len(r[2])] = np.array(r[2], dtype=np.int64)
    nref = np.array([r[3] for r in rows], dtype=np.int32)
    ref64, ref32 = R.score_batch(cand, refs, nref), R.score_batch(cand, refs, nref, dt=np.float32)
    out = _run(cand, refs, nref, dev)
    st, lcs, bleu, rouge = (out[k].cpu().numpy() for k in ("stats", "lcs", "bleu", "rouge"))
    for i, n_ in enumerate(name):
        print(f"[overlap] hand-made {n_!r}: stats {st[i].tolist()} lcs {lcs[i].tolist()} bleu {bleu[i].tolist()} rouge {rouge[i]:.7f}; "
              f"fp64 bleu {ref64['bleu'][i].tolist()} rouge {ref64['rouge'][i]:.7f}")
    _check("hand-made", out, ref64, ref32)
    i = name.index("Lc = 0")
    assert st[i].tolist() == [0] * 9 + [3] and not bleu[i].any() and rouge[i] == 0.0 and lcs[i].tolist() == [0, -1]
    i = name.index("no end mark at T = 63")
    assert st[i, 8] == 63 and st[i, 9] == 40 and st[i, :4].tolist() == [40, 39, 38, 37] and lcs[i, 0] == 40
    i = name.index("identical to its reference")
    assert st[i].tolist() == [7, 6, 5, 4, 7, 6, 5, 4, 7, 7] and lcs[i, 0] == 7
    assert np.abs(bleu[i] - 1.0).max() <= 4 * FLOOR and abs(rouge[i] - 1.0) <= 4 * FLOOR
    i = name.index("one word 63 times against 63")
    assert lcs[i, 0] == 63 and st[i, :4].tolist() == [63, 62, 61, 60]
    i = name.index("reversed permutation of 63 distinct words")
    assert lcs[i, 0] == 1 and st[i, :4].tolist() == [63, 0, 0, 0]
    i = name.index("nref = 0")
    assert st[i].tolist() == [0, 0, 0, 0, 7, 6, 5, 4, 7, 0] and not bleu[i].any() and rouge[i] == 0.0 and lcs[i].tolist() == [-1, -1]
    i = name.index("a reference with Lr = 0 beside a real one")
    assert lcs[i].tolist() == [0, 3] and st[i, 9] == 4 and st[i, :4].tolist() == [3, 1, 0, 0] and 0.0 < rouge[i] < 1.0
    i = name.index("length tie: Lc 5, references of 6 and 4 words")
    assert st[i, 8] == 5 and st[i, 9] == 4 and lcs[i].tolist() == [5, 4]
    i = name.index("ids 1, 257, 513, 65534 together")
    assert st[i, :8].tolist() == [5, 2, 1, 0, 6, 5, 4, 3] and lcs[i].tolist() == [4, 2]
    i = name.index("nref > Rmax is clamped")
    assert st[i, 9] == 2 and lcs[i].tolist() == [2, 3]


def test_deterministic_independent_of_other_rows_and_of_what_follows_the_end_mark():
    dev = torch.device("cuda:0")
    rows, S, T, Rmax, V = CASES[-1]
    c = _case(rows, S, T, Rmax, V)
    a, b = _run(c["cand"], c["refs"], c["nref"], dev), _run(c["cand"], c["refs"], c["nref"], dev)
    for k in ("stats", "lcs", "bleu", "rouge"):
        assert torch.equal(a[k], b[k]), k
    for r in (0, 1, 77, 163, 319):
        clip = r // S
        one = _run(c["cand"][r:r + 1], c["refs"][clip:clip + 1], c["nref"][clip:clip + 1], dev)
        for k in ("stats", "lcs", "bleu", "rouge"):
            assert torch.equal(one[k], a[k][r:r + 1]), (k, r)
    # what stands behind the first end mark, in candidates and references alike, changes no bit
    rng = np.random.default_rng(3)
    cand, refs = c["cand"].copy(), c["refs"].copy()
    changed = 0
    for arr in (cand.reshape(-1, T), refs.reshape(-1, T)):
        for row in arr:
            z = np.flatnonzero(row == 0)
            if z.size and z[0] + 1 < T:
                row[z[0] + 1:] = rng.integers(0, V, T - z[0] - 1)
                changed += 1
    assert changed >= rows // 2 and not np.array_equal(cand, c["cand"])
    g = _run(cand, refs, c["nref"], dev)
    for k in ("stats", "lcs", "bleu", "rouge"):
        assert torch.equal(g[k], a[k]), k


def test_replays_from_a_graph_bit_for_bit():
    from cvc import metrics
    dev = torch.device("cuda:0")
    rows, S, T, Rmax, V = CASES[-1]
    c = _case(rows, S, T, Rmax, V)
    cand, refs, nref = _t(c["cand"], dev, torch.int64), _t(c["refs"], dev, torch.int64), _t(c["nref"], dev, torch.int32)
    rng = np.random.default_rng(5)
    other = _t(np.stack([_caption(rng, T, V, True) for _ in range(rows)]), dev, torch.int64)
    run = lambda x: metrics.overlap(x, refs, nref, want_lcs=True)
    static = cand.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(static)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = run(static)
    for x in (other, cand):
        static.copy_(x)
        g.replay()
        want = run(x)
        for k in ("stats", "lcs", "bleu", "rouge"):
            assert torch.equal(out[k], want[k]), k
    assert not torch.equal(run(other)["stats"], run(cand)["stats"])


def test_bad_arguments():
    from cvc import hip
    dev = torch.device("cuda:0")
    fn = hip.lib().cvc_caption_overlap
    T, Rmax = 64, 1
    cand, refs, nref = torch.zeros(6, T, dtype=torch.int64, device=dev), torch.zeros(6, Rmax, T, dtype=torch.int64, device=dev), \
        torch.ones(6, dtype=torch.int32, device=dev)
    stats, lcs = torch.zeros(6, 10, dtype=torch.int32, device=dev), torch.zeros(6, Rmax, dtype=torch.int32, device=dev)
    bleu, rouge = torch.zeros(6, 4, device=dev), torch.zeros(6, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    call = lambda rows, T_, per, st, bl, ro: fn(p(cand), p(refs), p(nref), rows, T_, per, Rmax, st, p(lcs), bl, ro, None)
    rcs = dict(T64=call(6, 64, 1, p(stats), p(bleu), p(rouge)), per_clip=call(6, 20, 4, p(stats), p(bleu), p(rouge)),
               null_stats=call(6, 20, 1, None, p(bleu), p(rouge)), null_bleu=call(6, 20, 1, p(stats), None, p(rouge)),
               null_rouge=call(6, 20, 1, p(stats), p(bleu), None), rows0=call(0, 20, 1, p(stats), p(bleu), p(rouge)))
    print(f"[overlap] bad arguments -> {rcs}")
    assert all(rc == BADARG for rc in rcs.values()), rcs
    assert call(6, 20, 1, p(stats), p(bleu), p(rouge)) == 0 and call(6, 20, 3, p(stats), p(bleu), p(rouge)) == 0
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        from cvc import metrics
        metrics.overlap(cand, refs, nref)                                    # T = 64 through the Python surface
