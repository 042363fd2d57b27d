"""CPU tests of what tests/test_gpu_skinny_gemm.py relies on (no GPU): the K-loop sweep against the constants of
csrc/gemm_skinny.hip for both of its kernels, the two K-slice rules of the split-K form, the slice restatement against the full
product, the margins of the random merge cases and the planted orders of the exact and last-column cases."""
import pytest
import torch

import packed_gemm_cases as P
import skinny_gemm_cases as S


# ------------------------------------------------------------------ the sweep reaches every branch of both K loops
def test_k_sweep_reaches_every_branch_of_both_kernels():
    """ring kernel (NW = 4, RING = 3): a wave skips a segment (n_my = 0), runs the drain alone with 1, 2 and 3 chunks, one pass of
    the steady loop followed by a drain of 2 and of 3, and two passes followed by both; direct-load kernel (NW = 8): n_my = 0 .. 4,
    both exits of its two-step loop"""
    cs = S.source_constants()
    assert cs == dict(KC=32, RK=32, RING=3, NW_RING=4, NW_DIRECT=8)              # what the comments of the GPU file state
    ring = {n: P.wave_counts(n, cs["NW_RING"]) for n in S.SWEEP_CHUNKS}
    assert ring == {1: [1, 0, 0, 0], 3: [1, 1, 1, 0], 6: [2, 2, 1, 1], 11: [3, 3, 3, 2], 14: [4, 4, 3, 3], 18: [5, 5, 4, 4],
                    23: [6, 6, 6, 5], 27: [7, 7, 7, 6]}
    seen = {S.ring_branch(n) for counts in ring.values() for n in counts}
    want = {("skip",), ("drain", 1), ("drain", 2), ("drain", 3), ("steady", 1, 2), ("steady", 1, 3), ("steady", 2, 2), ("steady", 2, 3)}
    assert want <= seen, sorted(want - seen)
    # the thresholds as the source has them: the drain handles at most RING chunks, the steady loop starts at RING + 1
    assert [S.ring_branch(n)[0] for n in range(0, 9)] == ["skip"] + ["drain"] * cs["RING"] + ["steady"] * 5
    assert all(S.ring_branch(n)[2] in (2, 3) and S.ring_branch(n)[2] % 2 == n % 2 for n in range(4, 40))
    assert S.ring_branch(6)[1] == 2 and S.ring_branch(8)[1] == 3
    direct = {S.direct_branch(n) for nch in S.SWEEP_CHUNKS for n in P.wave_counts(nch, cs["NW_DIRECT"])}
    assert direct == {("none",), ("middle", 1), ("head", 2), ("middle", 3), ("head", 4)}
    assert P.wave_counts(27, cs["NW_DIRECT"]) == [4, 4, 4, 3, 3, 3, 3, 3]
    # four segments with chunk counts (1, 6, 3, 11): the ring pipeline restarts with another branch in every segment
    per_seg = [P.wave_counts(n, cs["NW_RING"]) for n in (1, 6, 3, 11)]
    assert [c[0] for c in per_seg] == [1, 2, 1, 3] and [c[3] for c in per_seg] == [0, 1, 0, 2]


# ------------------------------------------------------------------ the K slices
def test_both_slice_rules_partition_every_segment_exactly_once():
    """for nch = 1 .. 30 chunks and ksplit = 1 .. 64: the slices of a segment are consecutive, disjoint and cover [0, k) -- in the
    ring kernel's rule (nch = k / 32) and in the direct-load kernel's (nch = ceil(k / 32), tail clamped), there also at the ragged
    widths k = 32 nch - 28 .. 32 nch - 4"""
    cs = S.source_constants()
    for nch in range(1, 31):
        for ksplit in range(1, 65):
            widths = {"ring": [nch * 32], "direct": [nch * 32] + [nch * 32 - r for r in range(4, 32, 4)]}
            for kern, ks in widths.items():
                for k in ks:
                    b = S.slice_bounds(k, ksplit, kern, cs)
                    assert len(b) == ksplit and b[0][0] == 0 and b[-1][1] == k, (kern, k, ksplit)
                    assert all(lo <= hi for lo, hi in b) and all(b[s][1] == b[s + 1][0] for s in range(ksplit - 1)), (kern, k, ksplit)
                    assert all(lo % 32 == 0 for lo, _ in b) and all(hi % 32 == 0 or hi == k for _, hi in b)
    # on whole chunks the two rules are one
    assert all(S.slice_bounds(n * 32, s, "ring") == S.slice_bounds(n * 32, s, "direct") for n in range(1, 31) for s in (1, 2, 3, 8, 64))
    # the cases the GPU file names
    assert S.slice_bounds(32, 8, "ring") == [(0, 0)] * 7 + [(0, 32)]
    assert [s for s, (lo, hi) in enumerate(S.slice_bounds(96, 64, "ring")) if hi > lo] == [21, 42, 63]
    assert S.slice_bounds(100, 3, "direct") == [(0, 32), (32, 64), (64, 100)]


@pytest.mark.parametrize("ks,ksplit,kern", [((352,), 8, "ring"), ((96, 160), 3, "ring"), ((96, 160), 64, "direct"), ((100,), 3, "direct"), ((32,), 8, "ring")])
def test_slice_references_sum_to_the_full_reference(ks, ksplit, kern):
    c = P.linear_case(7000 + sum(ks) + ksplit, 33, 72, sum(ks))
    segs, x_eff = S.split_segments(c, ks)
    assert torch.equal(x_eff, c["x"])
    refs, empty = S.slice_refs(c, segs, x_eff, ksplit, kern)
    torch.testing.assert_close(sum(refs), P.linear_ref(c["x"], c["w"], c["b"]), rtol=1e-12, atol=1e-12)
    for s in range(ksplit):
        if empty[s]:
            assert torch.equal(refs[s], (c["b"].double() if s == 0 else torch.zeros(72, dtype=torch.float64)).expand(33, 72))
    if len(ks) == 2 and ksplit == 3:
        # slice 1 of (96, 160): chunk [1, 2) of segment 0 and [1, 3) of segment 1, not a contiguous range of the concatenation
        want = c["x"][:, 32:64].double() @ c["w"][:, 32:64].double().t() + c["x"][:, 96 + 32:96 + 96].double() @ c["w"][:, 96 + 32:96 + 96].double().t()
        torch.testing.assert_close(refs[1], want, rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------ segments
def test_gather_segments_enter_the_reference_through_the_relu():
    c = P.lstm_case(5, 33, 40, 192)
    segs, x_eff = S.split_segments(c, (64, 96, 32), (0, 2))
    assert [("table" in s) for s in segs] == [True, False, True] and [s["k0"] for s in segs] == [0, 64, 160]
    for s in (segs[0], segs[2]):
        assert s["table"].shape == (50, s["k"]) and int(s["idx"][0]) == 0 and int(s["idx"][-1]) == 49
        assert bool((s["table"][s["idx"]] < 0).any())
        assert torch.equal(x_eff[:, s["k0"]:s["k0"] + s["k"]], torch.relu(s["table"][s["idx"]]))
    assert torch.equal(x_eff[:, 64:160], c["x"][:, 64:160]) and bool((x_eff[:, :64] >= 0).all())


# ------------------------------------------------------------------ records
@pytest.mark.parametrize("V,seed", P.MERGE_CASES)
def test_random_merge_cases_have_a_deciding_margin_on_every_row(V, seed):
    """what test_merged_word_and_logprob_on_random_rows asserts first, without a GPU: no row is left out there"""
    c, unk = P.merge_case(V, seed)
    _, _, margin = P.select_ref(P.linear_ref(c["x"], c["w"], c["b"]), unk)
    assert float(margin.min()) >= 1e-3


@pytest.mark.parametrize("V,seed", S.NEGATIVE_VOCAB_CASES)
def test_negative_vocabulary_cases_have_a_deciding_margin_on_every_row(V, seed):
    """what test_vocabulary_ending_inside_a_block_keeps_the_padding_out asserts first, without a GPU"""
    c = P.negative_vocab_case(seed, 37, V)
    ref = P.linear_ref(c["x"], c["w"], c["b"])
    assert float(ref.max()) < -1.0
    assert float(P.select_ref(ref, -1)[2].min()) >= 1e-3


def test_second_bias_differs_from_the_first_and_from_zero_on_every_column():
    """a dropped bias2, a doubled bias or the two swapped for one another moves every column by at least 1e-2"""
    cases = [P.linear_case(4000 + n, 64, 300, 32 * n) for n in S.SWEEP_CHUNKS]                       # the K-loop sweep's
    cases += [P.linear_case(9600 + M, M, 72, 192) for M in (65, 129)] + [P.linear_case(9100, 37, 300, 96)]
    for c in cases:
        V, b2 = c["V"], S.second_bias(c)
        assert b2.shape == (V,) and float(b2.abs().min()) >= 1e-2 and float((b2 - c["b"]).abs().min()) >= 1e-2


@pytest.mark.parametrize("place,V,K,pair", P.TIE_PLACES)
def test_planted_orders_of_the_exact_cases_hold(place, V, K, pair):
    """the integer cases are exact in fp32, their planted scenarios give the stated top two, and with four waves of eight columns
    the three places are one wave's scan, two waves of one block and two blocks"""
    c = P.exact_case(77, 8, V, K, pair)
    y = P.linear_ref(c["x"], c["w"], c["b"])
    assert torch.equal((c["x"] @ c["w"].t() + c["b"]).double(), y) and float(y.abs().max()) < 2 ** 24
    order = torch.sort(y, dim=1, descending=True, stable=True).indices
    assert torch.equal(order[:, 0], c["top1"]) and torch.equal(order[:, 1], c["top2"])
    _, _, i1, i2 = P.merge_records(P.block_records(y.float()), -1)
    assert torch.equal(i1, c["top1"]) and torch.equal(i2, c["top2"])
    a, b = pair
    wave = lambda n: (n // 32, (n % 32) // 8)
    want = {"one_wave": wave(a) == wave(b), "two_waves": wave(a)[0] == wave(b)[0] and wave(a)[1] != wave(b)[1],
            "two_blocks": wave(a)[0] != wave(b)[0], "thread_stride": wave(a)[0] != wave(b)[0]}
    assert want[place]


@pytest.mark.parametrize("M", [1, 33, 64])
def test_last_column_case_has_column_299_on_top_of_the_even_rows_only(M):
    c = S.last_column_case(8500 + M, M)
    y = P.linear_ref(c["x"], c["w"], c["b"])
    assert bool((y[0::2].argmax(1) == 299).all()) and bool((y[1::2].argmax(1) != 299).all())
    assert float((y[0::2, 299] - y[0::2, :299].max(1).values).min()) > 10.0


def test_offset_bound_case_tells_the_wrapped_row_from_the_right_one():
    """row 32 of the 4 GiB-strided weight view wraps to row 0 in 32-bit byte offsets: the two columns' products differ by far more
    than OP_TOL on every row, so the wrong row cannot pass"""
    c = P.linear_case(3232, 4, 33, 32)
    ref = P.linear_ref(c["x"], c["w"], c["b"])
    assert float((ref[:, 32] - ref[:, 0]).abs().min()) > 1e-2
    assert 32 * (1 << 25) * 4 == 1 << 32 and (1 << 30) + 32 == 32 * (1 << 25) + 32     # row 32 starts at 2^32 bytes; the buffer ends with it
    # the activation side: row 16 of the ldx = 2^26 view starts at 2^32 bytes and ends with the same buffer
    cx = P.linear_case(S.OFFSET_X_SEED, S.OFFSET_X_ROWS, 40, 32)
    refx = P.linear_ref(cx["x"], cx["w"], cx["b"])
    assert S.OFFSET_X_ROWS == 17 and float((refx[16] - refx[0]).abs().min()) > 1e-2
    assert 16 * (1 << 26) * 4 == 1 << 32 and 16 * (1 << 26) + 32 == (1 << 30) + 32


def test_mixed_magnitude_case_is_the_parity_tests_operands():
    c = S.mixed_magnitude_case(17, 256, 96)
    assert c["x"][0, :4].tolist() == [0.0, -0.0, 1.0, -2.0 ** -100] and str(float(c["x"][0, 1])) == "-0.0"
    assert float(c["x"][:, 5::13].abs().max()) > 1e17 and float(c["w"][:, 5::13].abs().max()) < 1e-17
