"""cvc_grounding_f1 (csrc/grounding.hip; cvc.metrics.grounding / GroundingScorer) against the numpy restatement of the grounding
scores (tests/grounding_ref.py).

pick, counts and the per-class table must EQUAL the restatement's, bit for bit: they are integers, and the hit test's fp32 products are
exact on the cases' integer coordinates below 2048.  f1 is compared with the fp64 restatement to 1e-6 absolute: values in [0, 1] built
by a handful of correctly rounded fp32 operations (each within 2^-24 relative) stay far below that.  tests/test_grounding_cpu.py checks,
from the restatement alone, that the case list holds hits and misses and every special input named there.
Every test prints its figures before it asserts."""
import numpy as np
import pytest
import torch

import grounding_ref as R

pytestmark = pytest.mark.gpu

F1_TOL = 1e-6


def _dev():
    return torch.device("cuda:0")


def _tensors(inp, rows=slice(None), clips=slice(None)):
    d = _dev()
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(d, dt)
    return dict(seq=t(inp["seq"][rows], torch.int64), att=t(inp["att"][rows], torch.float32), ppls=t(inp["ppls"][clips], torch.float32),
                gt_bboxs=t(inp["gt_bboxs"][clips], torch.float32), nbox=t(inp["nbox"][clips], torch.int32),
                word_cls=t(inp["word_cls"], torch.int32))


def _run(inp, table=None, **sel):
    from cvc import metrics
    if table is None:
        table = torch.zeros(inp["n_classes"] + 1, 6, dtype=torch.int32, device=_dev())
    return metrics.grounding(**_tensors(inp, **sel), frames=inp["frames"], per_clip=inp["per_clip"], table=table,
                             props_per_frame=inp["n_per"])


def _check(label, out, ref, table=None):
    for k in ("pick", "counts", "table"):
        assert out[k].dtype == torch.int32, k
    got = {k: out[k].cpu().numpy().astype(np.int64) for k in ("pick", "counts", "table")}
    f1 = out["f1"].cpu().double().numpy()
    err = float(np.abs(f1 - ref["f1"]).max())
    want_table = ref["table"] if table is None else table
    print(f"[grounding] {label}: object words {int((ref['pick'][:, :, 0] >= 0).sum())}, table column sums kernel "
          f"{got['table'].sum(0).tolist()} restatement {want_table.sum(0).tolist()}; f1 max |err| {err:.3e} (bound {F1_TOL:.0e}), "
          f"mean f1 {ref['f1'].mean():.4f}, non-zero {np.count_nonzero(ref['f1'])}/{ref['f1'].size}")
    np.testing.assert_array_equal(got["pick"], ref["pick"], err_msg=label)
    np.testing.assert_array_equal(got["counts"], ref["counts"], err_msg=label)
    np.testing.assert_array_equal(got["table"], want_table, err_msg=label)
    assert out["f1"].dtype == torch.float32 and err <= F1_TOL, (label, err)


@pytest.mark.parametrize("key", R.CASES, ids=lambda k: "r%d_s%d_T%d_F%d_Np%d_P%d_K%d" % k[:7])
def test_cases_equal_the_restatement(key):
    inp, ref = R.case(key)
    _check(str(key), _run(inp), ref)


def test_hand_worked_clip():
    from test_grounding_cpu import hand_worked_clip
    inp = hand_worked_clip()
    ref = R.score_batch(**inp)
    out = _run(inp)
    print(f"[grounding] hand-worked clip: pick {out['pick'][0].tolist()} counts {out['counts'][0].tolist()} f1 {float(out['f1'][0]):.7f}")
    _check("hand-worked clip", out, ref)
    assert out["counts"][0].tolist() == [5, 3, 2, 3, 2, 1] and out["table"][1].tolist() == [2, 2, 2, 1, 1, 1]
    assert abs(float(out["f1"][0]) - 4.0 / 11.0) <= F1_TOL


def test_nan_weights_follow_the_sequential_search():
    """a NaN in front keeps the search at j = 0; a NaN further back is never picked"""
    from test_grounding_cpu import hand_worked_clip
    inp = hand_worked_clip()
    inp["att"][0, 1, 0] = np.nan                     # man, frame 0: slot 0 stays
    inp["att"][0, 2, 4] = np.nan                     # dog, frame 1: slot 5 as before
    inp["att"][0, 3, 3:6] = np.nan                   # men, frame 1: all NaN -> slot 3
    ref = R.score_batch(**inp)
    assert ref["pick"][0, 1].tolist() == [0, 4] and ref["pick"][0, 2].tolist() == [1, 5] and ref["pick"][0, 3].tolist() == [2, 3]
    _check("NaN weights", _run(inp), ref)


def test_the_table_is_added_to_and_two_calls_equal_one():
    key = R.CASES[-1]
    inp, ref = R.case(key)
    rows = key[0]
    table = torch.zeros(inp["n_classes"] + 1, 6, dtype=torch.int32, device=_dev())
    a = _run(inp, table, rows=slice(0, 23), clips=slice(0, 23))
    first = table.clone()
    b = _run(inp, table, rows=slice(23, rows), clips=slice(23, rows))
    assert a["table"] is table and b["table"] is table
    print(f"[grounding] two calls: column sums after the first {first.sum(0).tolist()}, after the second {table.sum(0).tolist()}, "
          f"one call {ref['table'].sum(0).tolist()}")
    np.testing.assert_array_equal(table.cpu().numpy(), ref["table"])
    assert 0 < int(first.sum()) < int(table.sum())
    for k in ("pick", "counts"):
        np.testing.assert_array_equal(torch.cat([a[k], b[k]]).cpu().numpy(), ref[k])
    # a table that is not zero: the kernel adds
    seeded = torch.full_like(table, 7)
    _run(inp, seeded)
    np.testing.assert_array_equal(seeded.cpu().numpy(), ref["table"] + 7)


def test_two_runs_are_identical_and_rows_do_not_depend_on_each_other():
    key = R.CASES[2]                                  # per_clip = 3, T = 63
    inp, ref = R.case(key)
    a, b = _run(inp), _run(inp)
    for k in ("pick", "counts", "f1", "table"):
        assert torch.equal(a[k], b[k]), k
    one = _run(inp, rows=slice(3, 6), clips=slice(1, 2))
    for k in ("pick", "counts", "f1"):
        assert torch.equal(one[k], a[k][3:6]), k


def test_scorer_accumulates_without_a_host_read_and_reads_once():
    from cvc import metrics
    key = R.CASES[1]
    inp, ref = R.case(key)
    t = _tensors(inp)
    s = metrics.GroundingScorer(t["word_cls"].cpu(), inp["n_classes"], inp["frames"], inp["n_per"])
    for _ in range(2):
        out = s.add(t["seq"], t["att"], t["ppls"], t["gt_bboxs"], t["nbox"].long())
    np.testing.assert_array_equal(out["pick"].cpu().numpy(), ref["pick"])
    np.testing.assert_array_equal(s.sums(), 2 * ref["table"])
    s.add_sums(ref["table"])
    want = R.result(3 * ref["table"])
    got = s.result()
    print(f"[grounding] scorer: {got}")
    assert set(got) == set(R.KEYS)
    for k in R.KEYS:
        assert got[k] == pytest.approx(want[k], abs=1e-12), k


def test_replays_from_a_graph_add_every_time():
    key = R.CASES[1]
    inp, ref = R.case(key)
    from cvc import metrics
    t = _tensors(inp)
    table = torch.zeros(inp["n_classes"] + 1, 6, dtype=torch.int32, device=_dev())
    run = lambda: metrics.grounding(**t, frames=inp["frames"], per_clip=inp["per_clip"], table=table, props_per_frame=inp["n_per"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    table.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                        # one kernel node: no parallel branches
        out = run()
    table.zero_()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    print(f"[grounding] three replays: column sums {table.sum(0).tolist()}, one call {ref['table'].sum(0).tolist()}")
    np.testing.assert_array_equal(table.cpu().numpy(), 3 * ref["table"])
    np.testing.assert_array_equal(out["pick"].cpu().numpy(), ref["pick"])
    np.testing.assert_array_equal(out["counts"].cpu().numpy(), ref["counts"])


def test_bad_shapes_raise():
    from cvc import hip, metrics
    inp, _ = R.case(R.CASES[0])
    t = _tensors(inp)
    C = inp["n_classes"]
    table = torch.zeros(C + 1, 6, dtype=torch.int32, device=_dev())
    ok = dict(frames=inp["frames"], per_clip=1, table=table, props_per_frame=inp["n_per"])
    metrics.grounding(**t, **ok)
    with pytest.raises(RuntimeError):                # T = 64
        d = _dev()
        metrics.grounding(torch.zeros(1, 64, dtype=torch.int64, device=d), torch.zeros(1, 64, 10, device=d), t["ppls"], t["gt_bboxs"],
                          t["nbox"], t["word_cls"], **ok)
    with pytest.raises(RuntimeError, match="cvc_grounding_f1 failed: bad argument"):       # T = 64 past the Python checks
        d = _dev()
        hip.grounding_f1(torch.zeros(1, 64, dtype=torch.int64, device=d), torch.zeros(1, 64, 10, device=d), t["ppls"], t["gt_bboxs"],
                         t["nbox"], t["word_cls"], inp["frames"], table)
    for kw in (dict(table=table[:1]), dict(table=table[:, :5].contiguous()), dict(table=table.long())):       # a table that is too small
        with pytest.raises(RuntimeError):
            metrics.grounding(**t, **{**ok, **kw})
    with pytest.raises(RuntimeError):
        metrics.grounding(**{**t, "att": t["att"][:, :, :9].contiguous()}, **ok)
    with pytest.raises(RuntimeError):
        metrics.grounding(**{**t, "ppls": t["ppls"][:, :, :6].contiguous()}, **ok)
    with pytest.raises(RuntimeError):
        metrics.grounding(**{**t, "gt_bboxs": t["gt_bboxs"][:, :, :5].contiguous()}, **ok)
    with pytest.raises(RuntimeError):
        metrics.grounding(**t, **{**ok, "props_per_frame": 4})               # 10 slots in 2 frames of 4
    with pytest.raises(RuntimeError, match="dimension not covered"):        # picks of 63 x 200 (word, frame) pairs: more than the LDS
        d = _dev()
        hip.grounding_f1(torch.zeros(1, 63, dtype=torch.int64, device=d), torch.zeros(1, 63, 200, device=d),
                         torch.zeros(1, 200, 7, device=d), t["gt_bboxs"], t["nbox"], t["word_cls"], 200, table)
    torch.cuda.synchronize()
    assert int(table.sum()) == int(R.case(R.CASES[0])[1]["table"].sum())     # the refused calls launched nothing
