"""CPU tests of what tests/test_gpu_nn_gemm.py relies on (no GPU): the constants of csrc/gemm_nn.hip, the K-loop sweep against
them for all three kernels, the K-slice rule, the slice restatement against the full product, the plane layout, the host-built quad
layout and the mixed-magnitude operands -- and every refusal of the four entry points, whose argument checks all precede the
launch (the library loads without a GPU, as tests/test_cabi.py has it)."""
import pytest
import torch

import nn_gemm_cases as N


# ------------------------------------------------------------------ the constants and the sweep
def test_source_constants_are_what_the_gpu_file_states():
    assert N.source_constants() == dict(NN_MAX_SEG=6, CVC_NN_DEPTH=3, CVC_NNS_DEPTH=4, CVC_NN128_DEPTH=3, NW_FP32=4, NW_SPLIT=4, NW_SPLIT128=4)
    assert N.MAXSEG == 6 and len(N.SIX_WIDTHS) == 6


def test_k_sweep_reaches_every_branch_of_all_three_kernels():
    """with the depths and wave counts READ FROM THE SOURCE: a changed ring depth moves the thresholds, and the sweep then misses a
    branch of this list (checked with each of the three depths changed in a copy of the source)"""
    cs = N.source_constants()
    counts = {G: N.wave_counts(G, 4) for G in N.SWEEP_GROUPS}
    assert counts[1] == [1, 0, 0, 0] and all(counts[8 * n + 6] == [2 * n + 2, 2 * n + 2, 2 * n + 1, 2 * n + 1] for n in range(12))
    assert {n for c in counts.values() for n in c} == set(range(25))
    seen, want = N.sweep_branches(cs), N.wanted_branches()
    for kern in ("fp32", "split", "split128"):
        assert want[kern] <= seen[kern], (kern, sorted(want[kern] - seen[kern]))
    # the thresholds as the source has them: the simple loop below the depth, a first steady pass at 2 depth - 1 steps, tails of
    # depth - 1 .. 2 depth - 2 steps behind a pass
    for d in (3, 4):
        assert [N.ring_branch(n, d)[0] for n in range(d + 1)] == ["simple"] * d + ["ring"]
        assert N.ring_branch(2 * d - 2, d) == ("ring", 0, 2 * d - 2) and N.ring_branch(2 * d - 1, d) == ("ring", 1, d - 1)
        assert all(d - 1 <= N.ring_branch(n, d)[2] <= 2 * d - 2 for n in range(2 * d - 1, 60))
    # the 128-row kernel's tail runs at most 2 D - 2 = 4 steps, D - 1 = 2 of them requested before it: the rests the sweep reaches
    assert {b[0][2] for b in seen["split128"] if b[0][0] == "ring"} == {2, 3, 4}
    # ... and what the existing tests reach of the split kernel at their shapes (n2 in {0, 2, 32}): none of the tails of 3 behind a pass
    assert N.ring_branch(32, 4) == ("ring", 7, 4)


@pytest.mark.parametrize("name,depth", [("CVC_NN_DEPTH", 2), ("CVC_NN_DEPTH", 4), ("CVC_NNS_DEPTH", 3), ("CVC_NNS_DEPTH", 5),
                                        ("CVC_NN128_DEPTH", 2), ("CVC_NN128_DEPTH", 4)])
def test_a_changed_ring_depth_fails_the_coverage_check(tmp_path, name, depth):
    """the sweep cannot silently stop covering a ring: with one depth changed in a copy of the source, the coverage comparison of
    the test above misses branches of that kernel"""
    import re
    src = open(N.source_path()).read()
    changed, n = re.subn(r"(#define\s+" + name + r"\s+)\d+", r"\g<1>%d" % depth, src)
    assert n == 1
    p = tmp_path / "gemm_nn.hip"
    p.write_text(changed)
    cs = N.source_constants(str(p))
    assert cs[name] == depth
    seen, want = N.sweep_branches(cs), N.wanted_branches()
    kern = {"CVC_NN_DEPTH": "fp32", "CVC_NNS_DEPTH": "split", "CVC_NN128_DEPTH": "split128"}[name]
    assert want[kern] - seen[kern]
    assert all(want[k] <= seen[k] for k in want if k != kern)


# ------------------------------------------------------------------ the K slices
def test_slice_rule_partitions_the_groups_exactly_once():
    """G = K / 8 in 1 .. 100, ksplit in 1 .. G: consecutive, disjoint, non-empty, covering [0, G); a larger request is clamped to G"""
    for G in range(1, 101):
        for ksplit in range(1, G + 1):
            b = N.slice_groups(G, ksplit)
            assert len(b) == ksplit and b[0][0] == 0 and b[-1][1] == G, (G, ksplit)
            assert all(lo < hi for lo, hi in b) and all(b[s][1] == b[s + 1][0] for s in range(ksplit - 1)), (G, ksplit)
        assert N.slice_groups(G, G + 1) == N.slice_groups(G, G) == [(g, g + 1) for g in range(G)]
        assert N.slice_groups(G, 64 * G) == N.slice_groups(G, G)
    # the cases of the GPU file
    assert N.slice_groups(3, 64) == [(0, 1), (1, 2), (2, 3)]
    assert N.slice_groups(11, 3) == [(0, 3), (3, 7), (7, 11)] and N.slice_groups(47, 2) == [(0, 23), (23, 47)]
    assert N.slice_groups(23, 4) == [(0, 5), (5, 11), (11, 17), (17, 23)]
    assert [len(N.slice_groups(G, ks)) for G, ks in N.SLICE_CASES] == [5, 3, 4, 2, 3, 3]


@pytest.mark.parametrize("G,ksplit", N.SLICE_CASES)
def test_slice_references_sum_to_the_full_reference(G, ksplit):
    c = N.nn_case(7000 + G + ksplit, 33, 8 * G, sum(N.SLICE_WIDTHS))
    refs = N.slice_refs(c["dy"], c["w"], ksplit)
    assert len(refs) == min(ksplit, G)
    torch.testing.assert_close(sum(refs), N.nn_ref(c["dy"], c["w"]), rtol=1e-12, atol=1e-12)
    lo, hi = N.slice_groups(G, ksplit)[1]
    torch.testing.assert_close(refs[1], c["dy"][:, 8 * lo:8 * hi].double() @ c["w"][8 * lo:8 * hi].double(), rtol=0, atol=0)
    # unit scale at every K: a skipped or doubled 8-row group moves an output by about sqrt(8 / K) >= 0.1
    assert 0.8 < float(N.nn_ref(c["dy"], c["w"]).std()) < 1.2 and (8 / 752) ** 0.5 > 0.1


def test_plane_layout_pads_every_segment_to_whole_slabs():
    ntot, starts = N.plane_layout(N.SIX_WIDTHS)
    assert N.SIX_WIDTHS == (4, 128, 132, 256, 36, 260)
    assert ntot == 128 * (1 + 1 + 2 + 2 + 1 + 3) == 1280 and starts == [0, 128, 256, 512, 768, 896]
    assert N.plane_layout((132, 36)) == (384, [0, 256]) and N.plane_layout((4,)) == (128, [0]) and N.plane_layout((128,)) == (128, [0])
    for widths in ((4,), (128, 132), N.SIX_WIDTHS):
        ntot, starts = N.plane_layout(widths)
        ends = starts[1:] + [ntot]
        assert all(s % 128 == 0 and 0 <= e - s - n < 128 for s, e, n in zip(starts, ends, widths))


# ------------------------------------------------------------------ operands
def test_host_quad_is_the_layout_the_kernels_read():
    """[K/4][64][4]: element (q, m, e) = x[m, 4 q + e], rows >= M exactly +0.0"""
    x = torch.arange(1, 3 * 8 + 1, dtype=torch.float32).view(3, 8)
    q = N.host_quad(x)
    assert q.shape == (2, 64, 4) and q[1, 2].tolist() == [21.0, 22.0, 23.0, 24.0] and q[0, 1].tolist() == [9.0, 10.0, 11.0, 12.0]
    assert torch.equal(q.permute(1, 0, 2).reshape(64, 8)[:3], x)
    assert not bool(q[:, 3:].view(torch.int32).any())                           # +0.0 bits, not -0.0


def test_mixed_magnitude_case_keeps_its_stripes_on_the_k_index():
    c = N.mixed_nn_case(17, 376, 96)
    assert c["dy"].shape == (17, 376) and c["w"].shape == (376, 96) and c["w"].is_contiguous()
    assert c["dy"][0, :4].tolist() == [0.0, -0.0, 1.0, -2.0 ** -100] and str(float(c["dy"][0, 1])) == "-0.0"
    assert float(c["dy"][1:, 5::13].abs().max()) > 1e17 and float(c["w"][5::13].abs().max()) < 1e-17
    assert float(c["w"][6::13].abs().max()) > 1e-3
    ref = N.nn_ref(c["dy"], c["w"])
    assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) < 1e3
    # both K of the GPU test give some waves an odd number of groups (the fp32-MFMA step inside the split kernels)
    assert N.wave_counts(752 // 8, 4) == [24, 24, 23, 23] and N.wave_counts(376 // 8, 4) == [12, 12, 12, 11]


# ------------------------------------------------------------------ refusals (argument checks precede every launch)
A, B, W, D, WS = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000        # fake addresses, 16-byte aligned: nothing is dereferenced


def _segs(hip, n=1, **bad):
    """n valid segments (w, dst, ldw = 16, ncols = 8, ld_dst = 12); `bad` overrides fields of the LAST one"""
    arr = (hip.NNSeg * max(n, 1))()
    for s in range(max(n, 1)):
        f = dict(w=W + 64 * s, dst=D + 4096 * s, ldw=16, ncols=8, ld_dst=12)
        if s == max(n, 1) - 1:
            f.update(bad)
        arr[s] = hip.NNSeg(f["w"], f["dst"], f["ldw"], f["ncols"], f["ld_dst"])
    return arr


SEG_REFUSALS = [dict(w=None), dict(dst=None), dict(ncols=0), dict(ncols=2), dict(ncols=6), dict(ldw=18), dict(ld_dst=14),
                dict(ldw=4), dict(ld_dst=4), dict(w=W + 4), dict(dst=D + 4)]
CALL_REFUSALS = [dict(dy_q=None), dict(segs=None), dict(nsegs=0), dict(nsegs=7), dict(M=0), dict(M=65), dict(K=0), dict(K=4),
                 dict(K=12), dict(ksplit=0), dict(ksplit=2, ws=None)]


def _call(hip, entry, nseg_alloc=1, seg=None, **bad):
    a = dict(dy_q=A, dy_q2=B, K=64, M=8, M2=8, segs=_segs(hip, nseg_alloc, **(seg or {})), nsegs=nseg_alloc, ksplit=1, ws=WS, reduce=1)
    a.update(bad)
    L = hip.lib()
    if entry == "planes2":
        return L.cvc_linear_nn_planes2_fwd(a["dy_q"], a["dy_q2"], a["K"], a["M"], a["M2"], a["segs"], a["nsegs"], a["ksplit"], a["ws"],
                                           a["reduce"], None)
    fn = L.cvc_linear_nn_fwd if entry == "fwd" else L.cvc_linear_nn_planes_fwd
    return fn(a["dy_q"], a["K"], a["M"], a["segs"], a["nsegs"], a["ksplit"], a["ws"], None)


@pytest.mark.parametrize("entry", ["fwd", "planes", "planes2"])
def test_product_entry_points_refuse_one_bad_argument_at_a_time(entry):
    from cvc import hip
    assert len(SEG_REFUSALS) == 11 and len(CALL_REFUSALS) == 11
    for mode in ((0, 1, 2) if entry != "planes2" else (1, 2)):
        with N.split_mode(hip, mode):
            for bad in CALL_REFUSALS:
                alloc = 7 if bad.get("nsegs") == 7 else 1
                assert _call(hip, entry, nseg_alloc=alloc, **bad) == N.E_BADARG, (entry, mode, bad)
            for seg in SEG_REFUSALS:
                for nseg in (1, 3):                    # the bad segment alone, and last of three
                    assert _call(hip, entry, nseg_alloc=nseg, seg=seg) == N.E_BADARG, (entry, mode, seg, nseg)
            if entry == "planes2":
                for bad in (dict(M2=0), dict(M2=65), dict(dy_q2=None), dict(dy_q=A + 4), dict(dy_q2=B + 4)):
                    assert _call(hip, entry, **bad) == N.E_BADARG, (entry, mode, bad)
    if entry == "planes2":
        with N.split_mode(hip, 0):                     # split-product arithmetic only: an otherwise valid call
            assert _call(hip, entry) == N.E_BADARG
            assert _call(hip, entry, ksplit=2) == N.E_BADARG


def test_pack_quad_refuses_one_bad_argument_at_a_time():
    from cvc import hip
    L = hip.lib()
    for x, ldx, M, K, xq in ((A, 16, 0, 16, B), (A, 16, 65, 16, B), (A, 16, 8, 0, B), (A, 16, 8, 6, B), (A, 18, 8, 16, B), (A, 17, 8, 16, B),
                             (A + 4, 16, 8, 16, B), (A + 8, 16, 8, 16, B), (None, 16, 8, 16, B), (A, 16, 8, 16, None)):
        assert L.cvc_pack_quad(x, ldx, M, K, xq, None) == N.E_BADARG, (x, ldx, M, K, xq)
