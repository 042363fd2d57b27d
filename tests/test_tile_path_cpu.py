"""CPU tests of what tests/test_gpu_tile_path.py relies on (no GPU): the host restatements of tests/tile_path_cases.py (fragment
layout, census reference, LSTM finish, beam scan, back-track) against independent formulations, the gap condition of every beam
case, the constants the tables are built on against the sources, and that the tables reach every branch they claim."""
import math

import pytest
import torch

import tile_path_cases as T


# ------------------------------------------------------------------ constants and fragments
def test_constants_are_the_sources():
    """BEAM_MAX, ROW_CACHE (csrc/beam.hip), WG (csrc/row_block.h), FRAG and the form switch (csrc/gemm_tile.hip): a changed constant fails here until
    the case tables follow"""
    assert T.source_constants() == dict(BEAM_MAX=T.BEAM_MAX, ROW_CACHE=T.ROW_CACHE, WG=T.WG, FRAG=T.FRAG, WIDE_KSTEPS=T.WIDE_KSTEPS)
    assert T.KSTEP == 3 * T.FRAG and T.WG * T.ROW_CACHE == 8192 and T.BEAM_MAX == 8


def test_fragment_restatement_is_to_frag_per_plane():
    from cvc.decode import from_frag, to_frag
    x = torch.randn(70, 48, generator=T.gen(1)) * torch.exp2(torch.randint(-20, 20, (70, 1), generator=T.gen(2)).float())
    planes = torch.zeros(3, 96, 48, dtype=torch.int16)
    planes[:, :70] = T.split3(x)
    xb = T.planes_to_frag(planes)
    assert torch.equal(xb, to_frag(x, 96)) and torch.equal(T.frag_to_planes(xb), planes)
    assert torch.equal(from_frag(xb, 70), x)                      # hi + mid + lo is the fp32 value
    # integers in [-7, 7] are one bf16 term: bf16_bits is their exact pattern
    v = torch.arange(-7, 8).float()
    assert torch.equal((T.bf16_bits(v).to(torch.int32) << 16).view(torch.float32), v)
    assert torch.equal(T.split3(v)[1:], torch.zeros(2, 15, dtype=torch.int16))


def test_rows_alloc_restatement_is_the_library():
    from cvc import hip
    for M in [m for m, *_ in T.CENSUS] + [m for m, *_ in T.REAL] + [321, 1000, 2560]:
        assert hip.lib().cvc_tile_rows_alloc(M) == T.rows_alloc(M), M


# ------------------------------------------------------------------ 1. the census
@pytest.mark.parametrize("M,N,K,ksplit", [(33, 50, 48, 2), (5, 130, 176, 3)])
def test_census_reference_is_all_nine_products_minus_the_three_dropped(M, N, K, ksplit):
    """from_frag of the fragments (a second statement of the layout) gives sum_p X_p and sum_q W_q: their fp64 product per K slice,
    less the pairs with p + q > 2, is the census reference; and fp32 accumulation of it is exact"""
    from cvc.decode import from_frag
    X, W = T.census_case(9, M, N, K)
    xb, wb = T.census_frags(X, W)
    assert xb.shape[0] * 32 == T.rows_alloc(M) and bool((T.frag_to_planes(xb)[:, M:] == T.FILL16).all())
    assert torch.isnan((T.frag_to_planes(xb)[:, M:].to(torch.int32) << 16).view(torch.float32)).all()
    xs, ws = from_frag(xb, M).double(), from_frag(wb, N).double()
    assert torch.equal(xs, X.sum(0).double()) and float(from_frag(wb, wb.shape[0] * 32)[N:].abs().max() if wb.shape[0] * 32 > N else 0.0) == 0.0
    ref = T.census_ref(X, W, ksplit)
    for s in range(ksplit):
        a, b = (16 * v for v in T.slice_range(K // 16, s, ksplit))
        full = xs[:, a:b] @ ws[:, a:b].t()
        dropped = sum(X[p][:, a:b].double() @ W[q][:, a:b].double().t() for p, q in ((1, 2), (2, 1), (2, 2)))
        assert torch.equal(ref[s], full - dropped)
    assert float(ref.abs().max()) < 2 ** 24 and 6 * 2048 * 49 < 2 ** 24


def test_census_table_reaches_every_branch():
    small = [c for c in T.CENSUS if c[0] <= 320]
    assert {T.chunk_mh(M) for M, *_ in small if (M + 31) // 32 < 10} == {1, 2, 3, 4, 5}
    assert {M for M, *_ in T.CENSUS} >= {1, 33, 64, 65, 129, 161, 200, 250, 257, 320, 352, 640}
    assert T.chunk_mh(250) == 4 and T.chunk_mh(200) == 4 and T.chunk_mh(257) == 5 and T.chunk_mh(320) == 5 and T.chunk_mh(352) is None
    assert {N for _, N, *_ in T.CENSUS} >= {1, 50, 128, 130, 384}
    lengths = [T.slice_lengths(K, ks) for _, _, K, ks in T.CENSUS]
    assert {l for ls in lengths for l in ls} >= {1, 2, 3, 4, 5, 7}
    assert [12, 13] in lengths and [3, 4, 4] in lengths
    taken = {(ks, N) for _, N, K, ks in T.CENSUS if T.xcd_remap(N, ks)}
    not_taken = {(ks, N) for _, N, K, ks in T.CENSUS if ks > 1 and not T.xcd_remap(N, ks)}
    assert (2, 512) in taken and (4, 256) in taken and {ks for ks, _ in taken} == {2, 4, 8}
    assert {ks for ks, _ in not_taken} >= {2, 3, 4, 5, 6, 16} and (2, 50) in not_taken
    wide = {(K, ks) for _, _, K, ks in T.CENSUS if T.wide_form(K, ks)}
    assert wide == {(1024, 1), (2048, 2)} and not T.wide_form(1008, 1) and (1008, 1) in {(K, ks) for _, _, K, ks in T.CENSUS}
    assert any(T.big_form(M, N) for M, N, *_ in T.CENSUS)
    assert all(K <= 2048 and M <= 640 and N <= 512 and K % 16 == 0 and ks <= K // 16 for M, N, K, ks in T.CENSUS + T.REAL)
    # M > 320: every chunk height the device may pick (3, 4, 5 accumulator tiles) leaves dead row blocks at 11 blocks; at 20 blocks
    # heights 3 and 4 do, and a grid of at most one round of workgroups takes 3 (csrc/gemm_tile.hip::tile_rows_per_chunk)
    assert all((11 + 2 * mh - 1) // (2 * mh) * 2 * mh > 11 for mh in (3, 4, 5))
    assert all((20 + 2 * mh - 1) // (2 * mh) * 2 * mh > 20 for mh in (3, 4))


# ------------------------------------------------------------------ 2. finishers
def test_finisher_tables_reach_every_template():
    lc = T.linear_cases()
    assert {c["nparts"] for c in lc} == set(T.LIN_NPARTS) >= {1, 2, 4, 6, 8, 16, 3, 17}
    for key, want in (("N", {1, 255, 256, 257, 513}), ("M", {1, 321}), ("bias", {False, True}), ("bias2", {False, True})):
        assert {c[key] for c in lc} == want
    assert any(c["ld"] > c["N"] for c in lc) and any(c["ldy"] > c["N"] for c in lc) and any(c["ld"] == c["N"] for c in lc)
    assert {n for n, *_ in T.LSTM_CASES} == {1, 2, 4, 8, 3, 5, 6, 16}
    assert {r for _, r, _, _ in T.LSTM_CASES} == {16, 48, 64, 256} and {m for _, _, m, _ in T.LSTM_CASES} == {1, 31, 32, 33, 70, 320}
    assert {g for *_, g in T.LSTM_CASES} == {1, 5}
    p, b, b2 = T.linear_inputs(dict(nparts=3, N=5, M=2, ld=5, ldy=5, bias=True, bias2=True, seed=1))
    assert torch.equal(T.ordered_sum(p, b, b2), ((p[0] + p[1]) + p[2]) + b + b2)


def test_lstm_finish_restatement_is_nn_lstmcell_in_double():
    """with an identity input matrix the cell's pre-activations are its input + both biases: the packed feature order, the per-clip
    gate term (row m / gb_div), the table row of the word (outside [0, V): row 0) and the cell update"""
    c = T.lstm_inputs(5, 3, 16, 33, 5)
    R, M = 16, 33
    assert set(c["word"][[0, 3, 6]].tolist()) == {-1, T.LSTM_V, T.LSTM_V + 5}
    from cvc.decode import pack_weights_tile
    ckpt = torch.arange(4 * R).float().view(4 * R, 1).repeat(1, 16)
    packed = T.frag_to_planes(pack_weights_tile(ckpt, lstm_R=R))[0, :4 * R, 0]         # the checkpoint row at every packed position
    packed = (packed.to(torch.int32) << 16).view(torch.float32).long()
    pre = torch.randn(M, 4 * R, generator=T.gen(3))
    assert torch.equal(T.unpack_gates(pre[:, packed], R), pre)
    cell = torch.nn.LSTMCell(4 * R, R).double()
    with torch.no_grad():
        cell.weight_ih.copy_(torch.eye(4 * R)); cell.weight_hh.zero_()
        cell.bias_ih.copy_(c["b_ih"]); cell.bias_hh.copy_(c["b_hh"])
        w = c["word"].clone()
        w[(w < 0) | (w >= T.LSTM_V)] = 0
        x = T.unpack_gates(c["parts"].double().sum(0), R) + c["gate_bias"].double().repeat_interleave(5, 0)[:M] + c["emb_gate"].double()[w]
        h, cn = cell(x, (torch.zeros(M, R, dtype=torch.float64), c["c_prev"].double()))
    ref = T.lstm_finish_ref(c, True)
    torch.testing.assert_close(ref[0], cn, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(ref[1], h, rtol=1e-12, atol=1e-12)
    s = T.lstm_inputs(6, 2, 16, 4, 1, saturated=True)
    assert set(s["parts"].sum(0).unique().tolist()) == {30.0, -30.0, 100.0, -100.0} and set(s["c_prev"].abs().unique().tolist()) == {1e4}
    assert bool(torch.isfinite(torch.stack(T.lstm_finish_ref(s, False))).all())


def test_reorder_and_pack_tables():
    assert {e for e, *_ in T.REORDER_CASES} == {0, 16, 32} and {p for _, p, *_ in T.REORDER_CASES} == {True, False}
    assert {b for _, _, b, _, _ in T.REORDER_CASES} == {1, 3, 5, 8} and {r for *_, r, _ in T.REORDER_CASES} == {1, 33, 70, 320}
    assert {r for *_, r in T.REORDER_CASES} == {16, 48, 256} and all(rows % beam == 0 for _, _, beam, rows, _ in T.REORDER_CASES)
    c = T.reorder_inputs(1, 16, True, 5, 70, 16)
    assert bool(((c["word"] < 0) | (c["word"] >= T.REORDER_V)).any())
    xa, hl, ca, cl = T.reorder_ref(c)
    assert xa.shape == (70, 48) and torch.equal(xa[:, :16], hl) and bool((xa[:, 16:32] >= 0).all())
    assert torch.equal(xa[0, 16:32], torch.relu(c["table"][0]))                   # word -1 reads row 0
    assert all(K % 16 == 0 and ldx % 4 == 0 for _, K, ldx in T.PACK_ANY_BLK)
    assert {K for _, K, _, _ in T.PACK_ANY_SCALAR} >= {1, 5, 17, 37} and any(ldx % 2 for _, _, ldx, _ in T.PACK_ANY_SCALAR)
    assert any(off and K % 16 == 0 and ldx % 4 == 0 for _, K, ldx, off in T.PACK_ANY_SCALAR)


# ------------------------------------------------------------------ 4. beam bookkeeping
@pytest.mark.parametrize("kw", [dict(plant=(2, 5)), dict(plant=(0, 7), frozen=0.5), dict(plant=(3,), first=True), dict(special="twins", plant=(4,)),
                                dict(special="frozen_first"), dict(special="live_first"), dict(special="all_done"),
                                dict(special="neg_inf"), dict(random_logits=True, frozen=0.3)])
def test_beam_reference_is_exhaustive_enumeration(kw):
    c = T.beam_case("micro", 4, 3, 9, 42, **kw)
    ref = T.beam_ref(c)
    for b, best in enumerate(T.brute_force(c)):
        for r, (val, flat) in enumerate(best):
            if math.isfinite(val):
                assert (int(ref["parent"][b, r]), int(ref["word"][b, r])) == (flat // 9, flat % 9) and float(ref["score"][b, r]) == val
                assert bool(ref["done"][b, r]) == (bool(c["done"][b * 3 + flat // 9]) or flat % 9 == 0)
            else:
                assert not bool(ref["live"][b, r])


@pytest.mark.parametrize("name", T.BEAM_NAMES)
def test_beam_case_candidates_are_tied_by_construction_or_a_gap_apart(name):
    """every two candidates of a clip (random-logit cases: the best beam + 1) are exactly tied by construction or >= 1e-3 apart, so
    the fp32 kernel and the fp64 scan cannot disagree about order; and the case holds what its name says"""
    c = T.shared_beam_case(name)
    assert T.gap_violations(c, every_pair=c["exact"]) == []
    B, beam, V = c["B"], c["beam"], c["V"]
    assert beam < V <= T.WG * T.ROW_CACHE and 1 <= beam <= T.BEAM_MAX and c["logits"].shape == (B * beam, V)
    ref, lg = c["ref"], c["logits"].view(B, beam, V)
    if c["exact"]:
        finite = lg[torch.isfinite(lg)]
        assert torch.equal(finite, finite.round()), "integer-valued logits"
        assert torch.equal(T.ordered_sum(c["parts"], c["bias_v"]), c["logits"])
    if name.startswith("tie_"):
        cols = [p % V for p in T.TIE_PLACES[name[4:]]]
        assert bool((lg[:, :, cols] == lg.max(2, keepdim=True).values).all())
        # the best row of a clip gives its tied columns in index order
        k0 = ref["parent"][:, 0]
        want = sorted(cols)[:min(beam, len(cols))]
        n_top = min(beam, len(cols))
        assert bool((ref["parent"][:, :n_top] == k0.view(-1, 1)).all()) and ref["word"][0, :n_top].tolist() == want
    if name == "unk_unique_max":
        assert bool((lg.argmax(2) == c["unk"]).all()) and not bool((ref["word"] == c["unk"]).any())
    if name == "unk_tied_max":
        assert not bool((ref["word"] == c["unk"]).any()) and ref["word"][0, :2].tolist() == [2, 1500]
    if name.startswith("twins"):
        cols = sorted(next(kw for n, _, kw in T.BEAM_SPECS if n == name)["plant"])
        want = [(k, v) for k in (0, 1) for v in cols][:beam]              # equal rows, equal scores: the lower k first, column by column
        n = len(want)
        assert ref["parent"][:, :n].tolist() == [[k for k, _ in want]] * B and ref["word"][:, :n].tolist() == [[v for _, v in want]] * B
        assert bool((ref["score"][:, :n] == ref["score"][:, :1]).all())
    if name in ("frozen_first", "live_first"):
        assert bool((ref["score"][:, 0] == ref["score"][:, 1]).all()) and ref["parent"][:, :2].tolist() == [[0, 1]] * B
        assert ref["word"][:, :2].tolist() == ([[0, V // 2]] if name == "frozen_first" else [[V // 2, 0]]) * B
    if name.startswith("first_step"):
        assert bool((ref["parent"] == 0).all()) and bool((c["score"].view(B, beam)[:, 1:] > c["score"].view(B, beam)[:, :1]).all())
    if name == "all_done":
        assert bool((ref["word"] == 0).all()) and bool(ref["done"].all()) and sorted(ref["parent"][0].tolist()) == list(range(beam))
    if name.startswith("neg_inf"):
        assert 0 < int(ref["live"][0].sum()) < beam
    if name == "frozen_mix":
        inherited = c["done"].bool().view(B, beam).gather(1, ref["parent"])            # a frozen parent; word 0 of a live parent; neither
        assert bool(inherited.any()) and bool((~inherited & (ref["word"] == 0)).any()) and bool((~ref["done"]).any())


def test_beam_tables_reach_every_instantiation():
    cases = {n: dict(zip(("B", "beam", "V"), a[1:4]), **kw) for n, a, kw in T.BEAM_SPECS}
    probe = lambda n: dict(V=cases[n]["V"], nparts=cases[n].get("nparts", 1), bias=cases[n].get("bias", False) or cases[n].get("bias_shift", False),
                           part_stride=cases[n]["B"] * cases[n]["beam"] * cases[n]["V"] + cases[n].get("stride_pad", 0),
                           bias_shift=cases[n].get("bias_shift", False))
    fast = [n for n in cases if T.fast_form(probe(n))]
    general = [n for n in cases if not T.fast_form(probe(n))]
    assert {T.ng_of(cases[n]["V"]) for n in fast} == set(range(1, 9))
    assert {cases[n].get("nparts", 1) for n in fast} == {1, 2, 4, 6, 8}
    assert [T.ng_of(V) for V, *_ in T.FAST_SWEEP] == [1, 1, 2, 2, 3, 3, 4, 5, 5, 6, 7, 8] and all(f"fast_V{V}_np{p}" in fast for V, p, *_ in T.FAST_SWEEP)
    assert {V for V, *_ in T.FAST_SWEEP} == {8, 1024, 1028, 2048, 2052, 3072, 4096, 5000, 5120, 6144, 7168, 8192}
    assert all(f"general_V{V}_np{p}" in general for V, p, *_ in T.GENERAL_SWEEP) and {"fallback_stride", "fallback_bias"} <= set(general)
    assert {V for V, *_ in T.GENERAL_SWEEP} >= {9, 50, 1025, 5001, 8191} and {p for _, p, *_ in T.GENERAL_SWEEP} >= {3, 5, 7}
    assert cases["fallback_stride"]["V"] % 4 == 0 and cases["fallback_bias"]["V"] % 4 == 0
    assert {c["beam"] for c in cases.values()} >= {1, 2, 5, 8} and {c["B"] for c in cases.values()} >= {1, 3, 64}
    # where the tie places sit in the float4 scan: element (tid + 256 g) * 4 + e, lane = tid & 63, wave = tid >> 6
    tid = lambda v: (v // 4) % T.WG
    grp = lambda v: (v // 4) // T.WG
    a, b = T.TIE_PLACES["float4"]
    assert a // 4 == b // 4
    a, b = T.TIE_PLACES["lanes"]
    assert tid(a) != tid(b) and tid(a) // 64 == tid(b) // 64 and grp(a) == grp(b)
    a, b = T.TIE_PLACES["waves"]
    assert tid(a) // 64 != tid(b) // 64
    a, b = T.TIE_PLACES["groups"]
    assert b == a + 1024 and tid(a) == tid(b) and grp(a) != grp(b)
    a, b = T.TIE_PLACES["rowcache"]
    assert b == a + T.WG and tid(a) // 64 != tid(b) // 64 and a % 4 == b % 4
    assert len(T.TIE_PLACES["many"]) > T.BEAM_MAX and T.TIE_PLACES["ends"] == (0, -1)


def test_backtrack_reference_and_tables():
    assert {b for b, *_ in T.BACKTRACK_CASES} == {1, 3, 64} and {k for _, k, _, _ in T.BACKTRACK_CASES} == {1, 5, 8}
    assert {t for _, _, t, _ in T.BACKTRACK_CASES} == {1, 2, 20, 256} and {n for *_, n in T.BACKTRACK_CASES} == {1, 7, 100, 257}
    assert {w for w, _ in T.GATHER_CASES} == {4, 64, 1024, 1028, 2052} and {k for _, k in T.GATHER_CASES} == {1, 5, 8}
    c = T.backtrack_inputs(3, 2, 1, 4, 3)                           # beam 1: the only row, whatever the parents say
    seq, att = T.backtrack_ref(c)
    assert torch.equal(seq, c["words"].t()) and torch.equal(att, c["att"].permute(1, 0, 2))
    c = T.backtrack_inputs(4, 6, 5, 3, 2)
    assert {int(c["parent"][2, b * 5]) for b in range(6)} >= {-1, 5, 12, -5}       # out-of-range parents on the rank-0 path
    seq, att = T.backtrack_ref(c)
    # a hand walk of clip 1 (last parent = beam: clamped to slot 4): the attention row is the parent's, the word the child's
    k2 = 4
    assert int(seq[1, 2]) == int(c["words"][2, 5]) and torch.equal(att[1, 2], c["att"][2, 5 + k2])
    k1 = min(max(int(c["parent"][1, 5 + k2]), 0), 4)
    assert int(seq[1, 1]) == int(c["words"][1, 5 + k2]) and torch.equal(att[1, 1], c["att"][1, 5 + k1])
