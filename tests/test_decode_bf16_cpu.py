"""bf16-stored decode weights without a GPU: the rounding, the weight pack and its inverse, the dtype-aware cache plan, the new
building blocks in the library's block table and the engine's refusals (DecodeEngine(weights_dtype="bf16"))."""
import os
import re

import pytest
import torch

from cvc import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _special_values():
    f = lambda bits: torch.tensor(bits, dtype=torch.int64).to(torch.int32).view(torch.float32)
    # exact ties (low half = 0x8000) above an even and above an odd kept mantissa, both signs; just below / above a tie; +-0;
    # denormals (smallest, largest, a tie); the largest finite fp32 (rounds to infinity) and the largest finite bf16; infinities
    pos = [0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001, 0x00000000, 0x00000001, 0x007FFFFF, 0x00008000,
           0x00018000, 0x00800000, 0x7F7FFFFF, 0x7F7F0000, 0x7F7F8000, 0x7F7F7FFF, 0x7F800000, 0x0000FFFF, 0x3F800000]
    bits = pos + [b - (1 << 32) + 0x80000000 for b in pos]      # the same with the sign bit set (as int32 bit patterns)
    return f(bits)


def test_bf16_round_is_round_to_nearest_even_bit_for_bit():
    from cvc.decode import bf16_round
    g = torch.Generator().manual_seed(7)
    x = torch.cat([torch.randn(100000, generator=g), torch.randn(20000, generator=g) * 1e-30, torch.randn(20000, generator=g) * 1e30,
                   torch.randn(5000, generator=g) * 1e-41, _special_values()])
    want = x.bfloat16().float()
    got = bf16_round(x)
    assert got.dtype == torch.float32 and torch.equal(got.view(torch.int32), want.view(torch.int32))      # (bit patterns: -0 stays -0)
    assert torch.equal(bf16_round(got).view(torch.int32), got.view(torch.int32))                           # idempotent
    assert (got.view(torch.int32) & 0xFFFF).eq(0).all()                                                    # a bf16 value
    t = bf16_round(_special_values())
    assert torch.isinf(t[12]) and t[13] == _special_values()[13]                # largest fp32 -> inf, largest bf16 stays
    assert torch.isnan(bf16_round(torch.tensor([float("nan")]))).all()
    with pytest.raises(RuntimeError, match="fp32"):
        bf16_round(torch.zeros(4, dtype=torch.float64))


@pytest.mark.parametrize("n,k,R", [(96, 64, None), (77, 32, None), (5000, 96, None), (4 * 40, 96, 40), (4 * 64, 160, 64)])
def test_bf16_pack_round_trip_and_layout(n, k, R):
    from cvc.decode import bf16_round, pack_weights, pack_weights_bf16, unpack_weights_bf16
    g = torch.Generator().manual_seed(n + k)
    w = torch.randn(n, k, generator=g) * torch.logspace(-6, 6, k).view(1, k)
    p = pack_weights_bf16(w, R)
    nb = (n + 31) // 32
    assert p.dtype == torch.bfloat16 and p.element_size() == 2 and p.is_contiguous()
    assert tuple(p.shape) == (nb, k // 8, 32, 8) and p.numel() * p.element_size() == 2 * nb * 32 * k
    assert torch.equal(unpack_weights_bf16(p, n, R), bf16_round(w))
    full = unpack_weights_bf16(p)                       # packed row order, zero rows beyond Nout
    assert full.shape == (nb * 32, k) and (R is not None or float(full[n:].abs().sum()) == 0.0)
    # same rows and k order as the fp32 pack: element (blk, octet o, row i, e) is k = 8 o + e of packed row 32 blk + i
    pf = pack_weights(bf16_round(w), R)                 # [nb][k/4][32][4]
    assert torch.equal(p.float().view(nb, k // 8, 32, 2, 4).permute(0, 1, 3, 2, 4).reshape(nb, k // 4, 32, 4), pf)
    # idempotent: packing the rounded matrix gives the same bits
    assert torch.equal(pack_weights_bf16(bf16_round(w), R).view(torch.int16), p.view(torch.int16))


def _sizes(name):
    d = synth.CONFIGS[name]
    fb = {"ppool": 4 * d.B * d.N * d.A, "pconv": 4 * d.B * d.F * d.A, "pool": 4 * d.B * d.N * d.R, "conv": 4 * d.B * d.F * d.R}
    return d, fb


def test_cache_plan_is_unchanged_for_fp32_and_fits_the_budget_for_bf16():
    from cvc.decode import weights as Wt
    if Wt.CACHE_BUDGET != 208 << 20 or not Wt.CACHE_GATE_WEIGHTS:
        pytest.fail("the literals below are the plans of the default settings (CVC_CACHE_BUDGET_MB / CVC_ATT_W_CACHED are set)")
    # fp32 byte counts: what the function returned before it knew of other widths (obtained by running that version)
    want = {
        ("cfg2", False): {"ppool": True, "pconv": True, "pool": False, "conv": False},
        ("cfg2", True): {"att_w": True, "ppool": True, "pconv": False, "pool": False, "conv": False},
        ("cfg5", False): {"ppool": False, "pconv": False, "pool": False, "conv": False},
        ("cfg5", True): {"att_w": False, "ppool": False, "pconv": False, "pool": False, "conv": False},
    }
    for (name, gate), plan in want.items():
        d, fb = _sizes(name)
        got = Wt.cache_plan(4 * (d.V * d.R + d.A * d.R), fb, gate_weight_bytes=4 * 4 * d.R * 2 * d.R if gate else None)
        assert got == plan and list(got) == list(plan), (name, gate, got)
    # bf16 byte counts: the language cell's matrix is a candidate; whatever is kept fits the budget
    for name in ("cfg1", "cfg2", "cfg5", "tiny"):
        d, fb = _sizes(name)
        for budget in (Wt.CACHE_BUDGET, 150 << 20, 60 << 20, 1 << 20):
            lin, att, lang = 2 * (d.V * d.R + d.A * d.R), 2 * 4 * d.R * 2 * d.R, 2 * 4 * d.R * 3 * d.R
            plan = Wt.cache_plan(lin, fb, budget=budget, gate_weight_bytes=att, lang_weight_bytes=lang)
            assert set(plan) == {"att_w", "lang_w", *fb}
            kept = (att if plan["att_w"] else 0) + (lang if plan["lang_w"] else 0) + sum(b for k, b in fb.items() if plan[k])
            assert kept <= max(budget - lin, 0), (name, budget, plan)
            assert not plan["lang_w"] or plan["att_w"]
    d, fb = _sizes("cfg2")
    plan = Wt.cache_plan(2 * (d.V * d.R + d.A * d.R), fb, gate_weight_bytes=2 * 4 * d.R * 2 * d.R, lang_weight_bytes=2 * 4 * d.R * 3 * d.R)
    assert plan["att_w"] and plan["lang_w"]          # 25 + 67 + 101 MB: both gate matrices and the linear weights fit together


def test_bf16w_blocks_are_in_the_block_table_and_check_their_arguments():
    """cvc_packed_lstm_bf16w_fwd / cvc_packed_linear_bf16w_fwd: declared in include/cvc_hip_blocks.h, bound through cvc_block(),
    absent from the dynamic symbol table; bad arguments are answered with CVC_E_BADARG before anything touches a device."""
    import ctypes
    import subprocess
    import build_hip
    from cvc import hip
    so = build_hip.build(verbose=False)
    names = ("cvc_packed_lstm_bf16w_fwd", "cvc_packed_linear_bf16w_fwd")
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cvc_hip_blocks.h")).read(), flags=re.S)
    lib = ctypes.CDLL(so)
    lib.cvc_block.restype = ctypes.c_void_p
    lib.cvc_block.argtypes = [ctypes.c_char_p]
    exported = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    for name in names:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert lib.cvc_block(name.encode()), name
        assert name in hip.BLOCKS and name in hip.SIGNATURES, name
        assert not re.search(r"\b" + name + r"\b", exported), name
    L = hip.lib()
    p = ctypes.c_void_p(4096)                       # a non-null, aligned address that is never dereferenced: every call below is refused
    lstm = lambda wp=p, stride=0, xq=p, K=64, eg=None, word=None, c=p, M=4, R=16, co=p: L.cvc_packed_lstm_bf16w_fwd(
        wp, stride, xq, K, None, None, None, eg, word, c, M, R, p, None, co, 0, None)
    lin = lambda wp=p, xq=p, K=64, M=4, N=50, ks=1, y=p, ldy=50, top2=None: L.cvc_packed_linear_bf16w_fwd(
        wp, xq, K, None, M, N, ks, y, ldy, top2, None)
    BAD = -1
    assert lstm(wp=None) == BAD and lstm(xq=None) == BAD and lstm(c=None) == BAD and lstm(co=None) == BAD
    assert lstm(K=48) == BAD and lstm(K=0) == BAD                          # K a multiple of 32, at least one chunk
    assert lstm(M=0) == BAD and lstm(M=65) == BAD
    assert lstm(R=12) == BAD and lstm(R=0) == BAD
    assert lstm(eg=p) == BAD and lstm(word=p) == BAD                       # table and words come together
    assert lstm(stride=64 * 32 - 8) == BAD and lstm(stride=64 * 32 + 4) == BAD          # blocks would overlap / lose alignment
    assert lstm(wp=ctypes.c_void_p(4098)) == BAD
    assert lin(wp=None) == BAD and lin(xq=None) == BAD and lin(y=None) == BAD
    assert lin(K=40) == BAD and lin(M=0) == BAD and lin(M=65) == BAD and lin(N=0) == BAD and lin(ks=0) == BAD
    assert lin(ks=2, top2=p) == BAD and lin(ldy=49) == BAD
    assert lin(xq=ctypes.c_void_p(4100)) == BAD


def test_engine_refuses_what_the_bf16_mode_does_not_cover():
    """Validated before anything touches a GPU; the mode is never silently run in fp32."""
    from cvc.decode import DecodeEngine
    new = lambda **kw: DecodeEngine.__init__(object.__new__(DecodeEngine), None, {}, 4, 1, weights_dtype="bf16", **kw)
    for kw, why in ((dict(beam=3), "beam"), (dict(sample_n=2, temperature=1.0), "sample_n"), (dict(sample_n=2), "sample_n"),
                    (dict(path="tile"), "tile"), (dict(path="ring"), "ring"), (dict(embgate=False), "embgate"),
                    (dict(gsk=True), "gsk"), (dict(gate_ksplit=True), "gate_ksplit"), (dict(lang_ksx=True), "lang_ksx")):
        with pytest.raises(RuntimeError, match=why):
            new(**kw)
    for bad in ("fp16", "BF16", None, 16):
        with pytest.raises(RuntimeError, match="weights_dtype"):
            DecodeEngine.__init__(object.__new__(DecodeEngine), None, {}, 4, 1, weights_dtype=bad)


def test_decode_weights_flag_lives_in_main_not_in_the_option_surface():
    """--decode_weights is an argument of cvc.main (next to --synthetic_clips), not of cvc.opts.parse_opt; the model reads it with
    an fp32 default."""
    import inspect
    from cvc import main as M, opts
    from cvc.model import captioner
    assert '"--decode_weights"' in inspect.getsource(M) and "decode_weights" not in inspect.getsource(opts)
    assert 'getattr(opts, "decode_weights", "fp32")' in inspect.getsource(captioner)
    sig = inspect.signature(captioner.DecodeAndGroundCaptionerGVDROI._sample)
    assert sig.parameters["decode_weights"].default is None
