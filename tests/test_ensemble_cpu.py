"""Ensemble decoding, the parts that need no GPU: the log-weights helper, the pure interleaving of the members' launch lists, the
engine-level refusals (EnsembleOptions.resolve), cvc.main's flags with their run-ending messages, and the block's declarations."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ ensemble_log_weights
def test_log_weights_uniform_and_normalised():
    from cvc import hip
    for M in (1, 2, 3, 8):
        lw = hip.ensemble_log_weights(None, M)
        assert lw.dtype == np.float32 and lw.shape == (M,)
        assert np.array_equal(lw, np.full(M, np.log(1.0 / M), dtype=np.float32))
    assert np.array_equal(hip.ensemble_log_weights(None, 1), np.zeros(1, np.float32))
    lw = hip.ensemble_log_weights([1, 1, 2], 3)
    assert np.array_equal(lw, np.log(np.array([0.25, 0.25, 0.5])).astype(np.float32))          # fp64 log, rounded once
    assert np.abs(hip.ensemble_log_weights((3.0, 7.0), 2) - hip.ensemble_log_weights([0.3, 0.7], 2)).max() <= 1.2e-7     # scale-free
    assert abs(np.exp(lw.astype(np.float64)).sum() - 1.0) < 1e-6


@pytest.mark.parametrize("weights,M", [([0.0, 1.0], 2), ([-1.0, 2.0], 2), ([float("nan"), 1.0], 2), ([float("inf"), 1.0], 2),
                                       ([1.0, 1.0, 1.0], 2), ([1.0], 2), (["a", 1.0], 2), (3.0, 2), (None, 0), (None, 9), (None, True)])
def test_log_weights_refusals(weights, M):
    from cvc import hip
    with pytest.raises(RuntimeError, match="ensemble_log_weights"):
        hip.ensemble_log_weights(weights, M)


# ------------------------------------------------------------------ the interleaving
def _member(name, per_step, T, lead=1, trail=0):
    """a fake launch list: `lead` launches once, per_step[t] launches and a word_select per step, `trail` launches at the end"""
    out = [(f"{name}.lead{i}", None, ()) for i in range(lead)]
    for t in range(T):
        out += [(f"{name}.s{t}.{i}", None, ()) for i in range(per_step[t])]
        out.append(("word_select", None, (name, t)))
    return out + [(f"{name}.trail{i}", None, ()) for i in range(trail)]


def test_interleave_three_members_with_different_launch_counts():
    from cvc.decode import interleave_members
    T = 3
    lists = [_member("a", [2, 2, 2], T, lead=1, trail=1), _member("b", [1, 3, 1], T, lead=3), _member("c", [4, 1, 2], T, lead=0, trail=2)]
    seen = []
    out = interleave_members(lists, T, lambda t, sel: (seen.append((t, [s[2] for s in sel])), (f"combine{t}", None, ()))[1],
                             lambda t: (f"select{t}", None, ()))
    names = [e[0] for e in out]
    # one combine + one select per step, in that order, behind all members' launches of the step, members in index order
    expect = (["a.lead0", "a.s0.0", "a.s0.1", "b.lead0", "b.lead1", "b.lead2", "b.s0.0", "c.s0.0", "c.s0.1", "c.s0.2", "c.s0.3",
               "combine0", "select0",
               "a.s1.0", "a.s1.1", "b.s1.0", "b.s1.1", "b.s1.2", "c.s1.0", "combine1", "select1",
               "a.s2.0", "a.s2.1", "b.s2.0", "c.s2.0", "c.s2.1", "combine2", "select2",
               "a.trail0", "c.trail0", "c.trail1"])
    assert names == expect
    assert "word_select" not in names                      # the members' own selections are gone
    assert seen == [(t, [("a", t), ("b", t), ("c", t)]) for t in range(T)]      # combine sees every member's source, member order
    # nothing else is lost or duplicated
    assert sorted(n for n in names if "." in n) == sorted(e[0] for l in lists for e in l if e[0] != "word_select")
    # one member: the single model through the combine launch
    out1 = interleave_members([lists[0]], T, lambda t, sel: ("combine", None, ()), lambda t: ("select", None, ()))
    assert [e[0] for e in out1].count("combine") == T and len(out1) == len(lists[0]) + T


def test_interleave_refuses_a_missing_or_doubled_word_select():
    from cvc.decode import interleave_members
    T = 3
    good = _member("a", [2, 2, 2], T)
    comb, sel = (lambda t, s: ("combine", None, ())), (lambda t: ("select", None, ()))
    missing = [e for i, e in enumerate(good) if not (e[0] == "word_select" and e[2] == ("a", 1))]
    with pytest.raises(RuntimeError, match=r"member 1's launch list has 2 word_select entries"):
        interleave_members([good, missing], T, comb, sel)
    i = [k for k, e in enumerate(good) if e[0] == "word_select"][1]
    doubled = good[:i] + [good[i]] + good[i:]
    with pytest.raises(RuntimeError, match=r"member 0's launch list has two word_select entries with nothing between"):
        interleave_members([doubled, good], T, comb, sel)
    extra = good + [("x", None, ()), ("word_select", None, ("a", 3))]
    with pytest.raises(RuntimeError, match=r"member 0's launch list has 4 word_select entries"):
        interleave_members([extra], T, comb, sel)


# ------------------------------------------------------------------ refusals that need no device
@pytest.mark.parametrize("M,kw,match", [
    (2, dict(weights_dtype="bf16"), 'weights_dtype="bf16" is refused'),
    (2, dict(mix=True, temperature=1.0), "mix=True is refused"),
    (2, dict(gsk=True), "gsk / gate_ksplit / lang_ksx are refused"),
    (2, dict(gate_ksplit=True), "gsk / gate_ksplit / lang_ksx are refused"),
    (2, dict(lang_ksx=True), "gsk / gate_ksplit / lang_ksx are refused"),
    (2, dict(tail="fused"), 'tail="fused" is refused'),
    (2, dict(combine="mean"), "combine must be one of"),
    (0, dict(), "1 .. 8 members"),
    (9, dict(), "1 .. 8 members"),
    (2, dict(member_weights=[1.0]), "member_weights"),
    (2, dict(member_weights=[1.0, 0.0]), "member_weights"),
    (2, dict(member_weights=[1.0, float("nan")]), "member_weights"),
    (2, dict(no_such_option=1), "unknown options"),
    # everything else: DecodeMode.resolve's own refusals, unchanged
    (2, dict(beam=2, temperature=1.0), "sampling .temperature. and beam search"),
    (2, dict(forced_n=1, beam=3), "forced mode"),
    (3, dict(top_k=5), "top_k / top_p"),
])
def test_engine_refusals_need_no_device(M, kw, match):
    from cvc.decode import EnsembleOptions
    with pytest.raises(RuntimeError, match=match):
        EnsembleOptions.resolve(M, 8, 50, **kw)


def test_engine_refusals_come_before_any_tensor_is_touched():
    from cvc.decode import EnsembleEngine

    class W:
        V = 50
    with pytest.raises(RuntimeError, match='weights_dtype="bf16" is refused'):
        EnsembleEngine([(W(), None), (W(), None)], 8, 1, weights_dtype="bf16")
    with pytest.raises(RuntimeError, match="1 .. 8 members"):
        EnsembleEngine([], 8, 1)


def test_options_resolve_to_the_members_mode():
    from cvc.decode import EnsembleOptions
    from cvc.decode.mode import DecodeMode
    o = EnsembleOptions.resolve(1, 8, 50)                   # M = 1 is allowed
    assert o.logw == (0.0,) and not o.geometric and o.mode == DecodeMode.resolve(8, 50)
    o = EnsembleOptions.resolve(3, 8, 50, [1, 1, 2], "logprob", beam=3, beam_history=True, no_repeat_ngram=2, own_features=True)
    assert o.geometric and o.mode == DecodeMode.resolve(8, 50, beam=3, beam_history=True, no_repeat_ngram=2)
    assert dict(o.engine_options) == dict(beam=3, beam_history=True, no_repeat_ngram=2, own_features=True)
    assert np.array_equal(np.array(o.logw, np.float32), np.log(np.array([0.25, 0.25, 0.5])).astype(np.float32))


def test_member_mismatch_names_member_and_quantity():
    from cvc.decode.ensemble import check_members
    check_members([dict(B=4, N=7, V=50)] * 3)
    for k in ("B", "N", "V"):
        bad = dict(B=4, N=7, V=50)
        bad[k] += 1
        with pytest.raises(RuntimeError, match=rf"member 2 has {k} = {bad[k]}, member 0 has {k} = "):
            check_members([dict(B=4, N=7, V=50), dict(B=4, N=7, V=50), bad])


def test_exports():
    import cvc.decode
    import cvc.model
    from cvc.model.ensemble import CaptionEnsemble
    assert cvc.model.CaptionEnsemble is CaptionEnsemble and cvc.decode.EnsembleEngine.__name__ == "EnsembleEngine"
    with pytest.raises(RuntimeError, match="1 .. 8 members"):
        CaptionEnsemble([])
    with pytest.raises(RuntimeError, match="combine must be one of"):
        CaptionEnsemble([object()], combine="mean")


def test_the_member_switch_is_internal_and_off_by_default():
    import inspect
    from cvc.decode import DecodeEngine
    assert "_ensemble" not in inspect.signature(DecodeEngine.__init__).parameters           # no public option
    assert DecodeEngine._ensemble is None and object.__new__(DecodeEngine)._ensemble is None


# ------------------------------------------------------------------ cvc.main's flags
def _parse(argv):
    from cvc import main as cvc_main
    return cvc_main.build_parser().parse_args(["--no_cfg"] + argv)


def test_main_flags_absent_add_no_option_key():
    from cvc import main as cvc_main
    from cvc import opts as cvc_opts
    opt = _parse([])
    assert not any(k.startswith("ensemble") for k in vars(opt))
    assert cvc_main.check_ensemble_flags(opt) is None
    assert not any(k.startswith("ensemble") for k in vars(cvc_opts.build_parser().parse_args([])))      # flags of cvc.main, not cvc.opts


def test_main_flags_parse(tmp_path):
    from cvc import main as cvc_main
    a, b = tmp_path / "b.pth", tmp_path / "c.pth"
    a.write_bytes(b"")
    b.write_bytes(b"")
    opt = _parse(["--resume", "True", "--ensemble", f"{a},{b}", "--ensemble_weights", "1,1,2", "--ensemble_combine", "logprob"])
    assert cvc_main.check_ensemble_flags(opt) == ([str(a), str(b)], [1.0, 1.0, 2.0], "logprob")
    opt = _parse(["--resume", "True", "--ensemble", str(a)])
    assert cvc_main.check_ensemble_flags(opt) == ([str(a)], None, "prob")


def test_main_flags_end_the_run_with_a_message(tmp_path):
    import torch
    from cvc import main as cvc_main
    a = tmp_path / "b.pth"
    a.write_bytes(b"")
    with pytest.raises(SystemExit, match="--ensemble needs --resume True"):
        cvc_main.check_ensemble_flags(_parse(["--ensemble", str(a)]))
    with pytest.raises(SystemExit, match="2 weights for 3 members"):
        cvc_main.check_ensemble_flags(_parse(["--resume", "True", "--ensemble", f"{a},{a}", "--ensemble_weights", "1,2"]))
    with pytest.raises(SystemExit, match="no such checkpoint file: .*missing.pth"):
        cvc_main.check_ensemble_flags(_parse(["--resume", "True", "--ensemble", str(tmp_path / "missing.pth")]))
    with pytest.raises(SystemExit, match="finite numbers > 0"):
        cvc_main.check_ensemble_flags(_parse(["--resume", "True", "--ensemble", str(a), "--ensemble_weights", "1,0"]))
    with pytest.raises(SystemExit, match="--eval_obj_grounding_gt exclude each other"):
        cvc_main.check_ensemble_flags(_parse(["--resume", "True", "--ensemble", str(a), "--eval_obj_grounding_gt"]))
    with pytest.raises(SystemExit, match="need --ensemble"):
        cvc_main.check_ensemble_flags(_parse(["--ensemble_weights", "1,2"]))
    # a member whose vocabulary differs
    ref = {"embed.0.weight": torch.zeros(50, 8), "logit.weight": torch.zeros(50, 16), "logit.bias": torch.zeros(50)}
    cvc_main.check_member_state("b.pth", {k: v.clone() for k, v in ref.items()}, ref)
    other = dict(ref, **{"embed.0.weight": torch.zeros(60, 8), "logit.weight": torch.zeros(60, 16), "logit.bias": torch.zeros(60)})
    with pytest.raises(SystemExit, match=r"b.pth has a different vocabulary: embed.0.weight is \(60, 8\)"):
        cvc_main.check_member_state("b.pth", other, ref)
    with pytest.raises(SystemExit, match="does not fit a model built from these options: logit.bias"):
        cvc_main.check_member_state("b.pth", {k: v for k, v in ref.items() if k != "logit.bias"}, ref)


# ------------------------------------------------------------------ the block's declarations
def test_ensemble_block_is_declared_tabled_and_bound():
    import ctypes
    from cvc import hip
    name = "cvc_ensemble_logprobs"
    blocks_h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cvc_hip_blocks.h")).read(), flags=re.S)
    core_h = open(os.path.join(ROOT, "include", "cvc_hip.h")).read()
    m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, blocks_h)
    assert m and name not in core_h                       # a building block: the core header keeps its exports
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 9 and params[-1].startswith("cvc_stream_t") and params[0].startswith("const cvc_ensemble_src*")
    assert name in hip.BLOCKS and len(hip.SIGNATURES[name]) == 9
    assert re.search(r"#define\s+CVC_ENSEMBLE_MAX\s+8\b", blocks_h) and hip.ENSEMBLE_MAX == 8
    # the descriptor as the C compiler lays it out: pointer, int (padded), long long, pointer
    assert ctypes.sizeof(hip.EnsembleSrc) == 32 and hip.EnsembleSrc.part_stride.offset == 16 and hip.EnsembleSrc.bias.offset == 24
    assert "CVC_B(%s)" % name in open(os.path.join(ROOT, "cyclical-visual-captioning_amd", "csrc", "blocks.hip")).read()
    assert os.path.isfile(os.path.join(ROOT, "cyclical-visual-captioning_amd", "csrc", "ensemble.hip"))
    lib = hip.lib()
    lib.cvc_block.restype = ctypes.c_void_p
    assert lib.cvc_block(name.encode()) and lib.cvc_block(b"cvc_ensemble_mix")
    # the build refuses scratch in the combine kernel
    import build_hip
    assert "ensemble_logprobs_kernel" in build_hip.NO_SCRATCH_KERNELS["ensemble.hip"]
