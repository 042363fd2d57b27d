"""cvc_consensus_cider (csrc/consensus.hip) against the fp64 restatement of consensus selection (tests/consensus_ref.py, on
tests/cider_ref.py) and, bit for bit, against cvc_cider_d on gathered references.

Tolerance of the utilities, the project's rule: the reference is the restatement in fp64, the yardstick the SAME restatement in fp32
on the CPU; the kernel's largest error may be 4 x the yardstick's largest error, with a floor of 2^-20 (one fp32 ulp of the largest
CIDEr-D, 10).  pick is checked exactly against the kernel's own utilities, and against fp64 through the utility of the picked row
(within 2 x bound of the clip's fp64 maximum: duplicates among the candidates make near-ties the norm, an index comparison would be
wrong).  Every test prints its figures before it asserts."""
import numpy as np
import pytest
import torch

import cider_ref as R
import consensus_ref as C

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -20
_TABLES = {}


def _dev():
    return torch.device("cuda:0")


def _t(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev(), dt)


def _table(key, train):
    from cvc.cider import CiderD
    if key not in _TABLES:
        _TABLES[key] = CiderD.from_captions(train, _dev())
    return _TABLES[key]


def _run(table, cand, n, live):
    u, p, b = table.consensus(_t(cand, torch.int64), n, live=None if live is None else _t(live, torch.int32))
    return u, p, b


def _gathered(table, cand, n, live):
    """the route without the block: every row against its clip's other live rows, gathered -> cvc_cider_d with per_clip = 1"""
    rows, T = cand.shape
    live = np.ones(rows, dtype=bool) if live is None else np.asarray(live).astype(bool)
    Rmax = max(n - 1, 1)
    refs, nref = np.zeros((rows, Rmax, T), dtype=np.int64), np.zeros(rows, dtype=np.int32)
    for i in range(rows):
        if not live[i]:
            continue
        c0 = i // n * n
        others = [r for r in range(c0, c0 + n) if r != i and live[r]]
        refs[i, :len(others)] = cand[others]
        nref[i] = len(others)
    return table.score(_t(cand, torch.int64), _t(refs, torch.int64), _t(nref, torch.int32))


def _check(label, cand, n, live, got, u64, u32):
    """the three outputs of one launch against fp64 -> bound"""
    u, pick, best = (x.cpu().numpy() for x in got)
    rows = cand.shape[0]
    lv = np.ones(rows, dtype=bool) if live is None else np.asarray(live).astype(bool)
    err, yard = float(np.abs(u.astype(np.float64) - u64).max()), float(np.abs(u32 - u64).max())
    bound = max(4.0 * yard, FLOOR)
    m64 = np.where(lv, u64, -np.inf).reshape(-1, n)
    has = lv.reshape(-1, n).any(1)
    picked64 = u64.reshape(-1, n)[np.arange(rows // n), pick]
    gap = float((m64.max(1) - picked64)[has].max()) if has.any() else 0.0
    print(f"[consensus] {label}: kernel max |err| {err:.3e} (fp32 yardstick {yard:.3e}, bound {bound:.3e}); live rows {int(lv.sum())}/{rows}, "
          f"non-zero fp64 utilities {np.count_nonzero(u64[lv])}; largest fp64 shortfall of a picked row {gap:.3e} (allowed {2 * bound:.3e})")
    assert err <= bound, (label, err, yard)
    assert not u[~lv].any()                                               # a dead row's utility is 0
    assert np.array_equal(pick, C.picks(u, live, n)), label               # exact: the first live arg-max of the kernel's own utilities
    assert lv.reshape(-1, n)[np.arange(rows // n), pick][has].all()       # a dead row is never picked
    assert gap <= 2 * bound, (label, gap)
    assert np.array_equal(best, cand.reshape(-1, n, cand.shape[1])[np.arange(rows // n), pick]), label
    return bound


@pytest.mark.parametrize("clips,n,T,V", C.CASES)
def test_random_cases_vs_fp64(clips, n, T, V):
    c = C.case(clips, n, T, V)
    lv = np.ones(clips * n, dtype=bool) if c["live"] is None else c["live"]
    if T >= 4:                                   # not vacuous (T = 1: idf 0, all zeros by construction, kept for the edge)
        assert np.count_nonzero(c["u64"][lv]) >= 0.9 * lv.sum(), (np.count_nonzero(c["u64"][lv]), lv.sum())
    table = _table((clips, n, T, V), c["train"])
    _check(str((clips, n, T, V)), c["cand"], n, c["live"], _run(table, c["cand"], n, c["live"]), c["u64"], c["u32"])


@pytest.mark.parametrize("clips,n,T,V", C.CASES)
def test_utilities_have_the_bits_of_cider_d_on_gathered_references(clips, n, T, V):
    c = C.case(clips, n, T, V)
    table = _table((clips, n, T, V), c["train"])
    for live in ([c["live"], None] if c["live"] is not None else [None]):
        u = _run(table, c["cand"], n, live)[0]
        want = _gathered(table, c["cand"], n, live)
        same = int((u == want).sum())
        print(f"[consensus] {(clips, n, T, V)} live {'given' if live is not None else 'all'}: {same}/{u.numel()} utilities bit-equal to "
              f"cvc_cider_d, max |diff| {float((u - want).abs().max()):.3e}")
        assert torch.equal(u, want)


def _hand_table():
    rng = np.random.default_rng(7)
    train = [C.clip_candidates(rng, 1, 8, 20, garbage=False)[0] for _ in range(200)]       # words 20, 21, 22: absent from the table
    return train, R.doc_freq(train)


def test_hand_made_clips():
    """T = 8, V = 23: the edges of the definition, each against fp64 and some exactly"""
    T = 8
    train, (df, n_doc) = _hand_table()
    table = _table("hand", train)
    A, U, Z = [2, 3, 4, 5, 6, 0, 0, 0], [9, 10, 11, 0, 0, 0, 0, 0], [0] * T
    full = [3, 4, 5, 6, 7, 8, 9, 10]
    clips = {
        "n = 1": ([A], None),
        "all rows dead": ([U, A, A], [0, 0, 0]),
        "one live row among dead ones": ([A, U, A], [0, 1, 0]),
        "two identical and one unrelated": ([A, A, U], None),
        "the end mark alone": ([Z, A, [2, 3, 0, 0, 0, 0, 0, 0]], None),
        "no end mark": ([full, [3, 4, 5, 6, 0, 0, 0, 0], full[:7] + [0]], None),
        "asymmetric pair": ([[6] * T, [2, 6, 3, 0, 0, 0, 0, 0]], None),
        "n-grams absent from the table": ([[20, 21, 22, 20, 0, 0, 0, 0], [20, 21, 22, 21, 0, 0, 0, 0], A], None),
    }
    out = {}
    for name, (rows, live) in clips.items():
        cand, n = np.array(rows, dtype=np.int64), len(rows)
        live = None if live is None else np.array(live, dtype=bool)
        u64, u32 = C.utilities(cand, n, live, df, n_doc), C.utilities(cand, n, live, df, n_doc, dt=np.float32)
        got = _run(table, cand, n, live)
        bound = _check(name, cand, n, live, got, u64, u32)
        out[name] = (got[0].cpu().numpy(), int(got[1][0]), got[2].cpu().numpy()[0], u64, bound)
        print(f"[consensus] hand-made {name!r}: kernel {out[name][0].tolist()}, fp64 {u64.tolist()}, pick {out[name][1]}")
    u, p, b, _, _ = out["n = 1"]
    assert u.tolist() == [0.0] and p == 0 and b.tolist() == A
    u, p, b, _, _ = out["all rows dead"]
    assert not u.any() and p == 0 and b.tolist() == U                      # best = the clip's first row
    u, p, b, _, _ = out["one live row among dead ones"]
    assert not u.any() and p == 1 and b.tolist() == U
    u, p, b, _, _ = out["two identical and one unrelated"]
    assert p == 0 and u[0] == u[1] and u[2] < u[0] and u[2] == u.min()
    u, p, b, u64, _ = out["the end mark alone"]
    assert p != 0 and u64[0] == 0.0 and u[0] == 0.0                         # "0" alone: idf 0 (every caption ends), nothing in common
    u, p, b, u64, _ = out["no end mark"]
    assert 0.0 < u[0] < 10.0
    u, p, b, u64, bound = out["asymmetric pair"]
    a_, b_ = clips["asymmetric pair"][0]
    s_ab, s_ba = float(R.score(a_, [b_], df, n_doc)[0]), float(R.score(b_, [a_], df, n_doc)[0])
    print(f"[consensus] asymmetric pair: score(a | b) {s_ab:.7f}, score(b | a) {s_ba:.7f}, kernel {u.tolist()}")
    assert abs(s_ab - s_ba) > 100 * bound                                   # the directions differ by far more than the tolerance
    assert abs(u[0] - s_ab) <= bound and abs(u[1] - s_ba) <= bound
    assert abs(u[0] - s_ba) > bound and abs(u[1] - s_ab) > bound            # ... and each row has ITS direction, not the other


def test_words_behind_the_end_mark_change_no_output_bit():
    T, n = 8, 5
    train, _ = _hand_table()
    table = _table("hand", train)
    rng = np.random.default_rng(11)
    cand = np.concatenate([C.clip_candidates(rng, n, T, 20, garbage=False) for _ in range(6)])
    other = cand.copy()
    for r in range(other.shape[0]):
        L = len(R.words(other[r]))
        other[r, L:] = rng.integers(0, 23, T - L)                          # zeros included: a second end mark changes nothing either
    assert not np.array_equal(cand, other)
    live = rng.random(cand.shape[0]) >= 0.15
    a, b = _run(table, cand, n, live), _run(table, other, n, live)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    idx = torch.arange(6, device=_dev()) * n + b[1]
    assert torch.equal(b[2], _t(other, torch.int64)[idx]) and torch.equal(a[2], _t(cand, torch.int64)[idx])


def test_deterministic_and_independent_of_the_other_clips():
    clips, n, T, V = C.CASES[-1]
    c = C.case(clips, n, T, V)
    table = _table((clips, n, T, V), c["train"])
    a, b = _run(table, c["cand"], n, c["live"]), _run(table, c["cand"], n, c["live"])
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    rng = np.random.default_rng(5)
    for clip in (0, 1, 31, 63):
        sl = slice(clip * n, (clip + 1) * n)
        one = _run(table, c["cand"][sl], n, c["live"][sl])                  # alone in its launch
        other = np.concatenate([C.clip_candidates(rng, n, T, V) for _ in range(clips)])
        other[sl] = c["cand"][sl]
        olive = rng.random(clips * n) >= 0.3
        olive[sl] = c["live"][sl]
        mixed = _run(table, other, n, olive)                                # among other clips
        for full, single, mix, per in zip(a, one, mixed, (n, 1, 1)):
            assert torch.equal(full[clip * per:(clip + 1) * per], single), clip
            assert torch.equal(full[clip * per:(clip + 1) * per], mix[clip * per:(clip + 1) * per]), clip


def test_replays_from_a_graph_bit_for_bit():
    from cvc import hip
    clips, n, T, V = C.CASES[-1]
    c = C.case(clips, n, T, V)
    table = _table((clips, n, T, V), c["train"])
    cand, live = _t(c["cand"], torch.int64), _t(c["live"], torch.int32)
    rng = np.random.default_rng(6)
    other = _t(np.concatenate([C.clip_candidates(rng, n, T, V) for _ in range(clips)]), torch.int64)
    olive = _t(rng.random(clips * n) >= 0.5, torch.int32)

    def run(x, l):
        return hip.consensus_cider(x, n, table.keys, table.idf, table.idf_unseen, table.sigma, live=l)
    s_cand, s_live = cand.clone(), live.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(s_cand, s_live)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = run(s_cand, s_live)
    for x, l in ((other, olive), (cand, live)):
        s_cand.copy_(x)
        s_live.copy_(l)
        g.replay()
        for got, want in zip(out, run(x, l)):
            assert torch.equal(got, want)
    assert not torch.equal(run(other, olive)[0], run(cand, live)[0])


def test_bad_arguments_surface_as_runtime_errors():
    from cvc import hip
    train, _ = _hand_table()
    table = _table("hand", train)

    def call(rows, T, per):
        return hip.consensus_cider(torch.zeros(rows, T, dtype=torch.int64, device=_dev()), per, table.keys, table.idf, table.idf_unseen)
    with pytest.raises(RuntimeError, match="cvc_consensus_cider failed: bad argument"):
        call(33, 8, 33)
    with pytest.raises(RuntimeError, match="cvc_consensus_cider failed: bad argument"):
        call(4, 64, 2)
    with pytest.raises(RuntimeError):
        call(7, 8, 2)
    with pytest.raises(RuntimeError, match="bad argument"):                 # the block itself, past the wrapper's own check
        z = torch.zeros(7, 8, dtype=torch.int64, device=_dev())
        hip._check(hip.lib().cvc_consensus_cider(z.data_ptr(), None, 7, 8, 2, table.keys.data_ptr(), table.idf.data_ptr(), len(table),
                                                 table.idf_unseen, 6.0, z.data_ptr(), z.data_ptr(), z.data_ptr(), None), "cvc_consensus_cider")
    u, p, b = call(4, 8, 2)                                                 # the same call within the limits runs
    assert u.shape == (4,) and p.tolist() == [0, 0] and not b.any()
