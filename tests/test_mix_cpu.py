"""Scheduled sampling, what needs no GPU: the schedule, the host restatement of the coin, the hash sites, the command line, the
block's place in the library and its host-side argument checks, and the engine's refusals."""
import ctypes
import os
import re

import numpy as np
import pytest

import mix_ref as MR
import sample_oracle as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "cvc_mixed_select_parts"


def test_schedule_over_a_hand_written_table():
    from cvc.trainer import ss_prob_at
    # (epoch, start, increase_every, increase_prob, max_prob) -> share
    table = [((0, -1, 5, 0.05, 0.25), 0.0), ((99, -1, 1, 0.5, 1.0), 0.0),            # never
             ((0, 3, 5, 0.05, 0.25), 0.0), ((2, 3, 5, 0.05, 0.25), 0.0),              # before the start
             ((3, 3, 5, 0.05, 0.25), 0.0), ((7, 3, 5, 0.05, 0.25), 0.0),              # the first stair is 0
             ((8, 3, 5, 0.05, 0.25), 0.05), ((12, 3, 5, 0.05, 0.25), 0.05), ((13, 3, 5, 0.05, 0.25), 0.05 * 2),
             ((27, 3, 5, 0.05, 0.25), 0.05 * 4), ((28, 3, 5, 0.05, 0.25), 0.25), ((500, 3, 5, 0.05, 0.25), 0.25),   # the cap
             ((0, 0, 1, 0.25, 0.25), 0.0), ((1, 0, 1, 0.25, 0.25), 0.25), ((2, 0, 1, 0.25, 0.25), 0.25),
             ((4, 0, 2, 0.3, 1.0), 0.3 * 2), ((40, 0, 2, 0.3, 1.0), 1.0)]
    for args, want in table:
        got = ss_prob_at(*args)
        assert isinstance(got, float) and got == want, (args, got, want)


def test_host_coin_is_strictly_inside_the_unit_interval():
    rows = 4096
    for seed, call, t in ((0, 1, 0), (7, 3, 5), (2 ** 63 + 11, 9, 63)):
        u = MR.coin_uniform(seed, call, t, rows)
        assert u.dtype == np.float32 and (u > 0).all() and (u < 1).all()
        assert not MR.took(seed, call, t, rows, 0.0).any()                 # p = 0 takes none
        assert MR.took(seed, call, t, rows, 1.0).all()                     # p = 1 takes all
        share = MR.took(seed, call, t, rows, 0.25).mean()
        assert abs(share - 0.25) < 5 * np.sqrt(0.25 * 0.75 / rows), share  # (a fair coin: five standard deviations)
    # the extreme hash values stay inside too
    for h in (0, 0xFFFFFFFF):
        u = (np.float32(h >> 9) + np.float32(0.5)) * np.float32(2.0 ** -23)
        assert 0 < u < 1
    # other steps, other calls: other coins
    assert not np.array_equal(MR.coin_uniform(7, 3, 5, rows), MR.coin_uniform(7, 3, 6, rows))
    assert not np.array_equal(MR.coin_uniform(7, 3, 5, rows), MR.coin_uniform(7, 4, 5, rows))


def test_mix_sites_collide_with_no_dropout_site_and_no_sample_site():
    from cvc import dropout
    src = open(os.path.join(ROOT, "include", "cvc_hip_blocks.h")).read()
    const = {k: int(v, 16) for k, v in re.findall(r"#define (CVC_\w+_SITE) (0x[0-9A-Fa-f]+)u", src)}
    assert const["CVC_MIX_SITE"] == MR.MIX_SITE and const["CVC_SAMPLE_SITE"] == S.SAMPLE_SITE
    mix = {MR.MIX_SITE + t for t in range(MR.T_MAX)}
    sample = {S.SAMPLE_SITE + t for t in range(MR.T_MAX)}
    drop = set(dropout._SITES.values())
    for t in range(256):
        drop |= {dropout.site_id("out_a.%d" % t), dropout.site_id("out_c.%d" % t)}
    drop |= {s + 64 * g for s in list(drop) for g in range(64)}           # the loops' per-group sites (site + 64 g)
    assert len(mix) == MR.T_MAX and not (mix & sample) and not (mix & drop)
    assert all(s < 2 ** 32 for s in mix)


def test_main_parser_accepts_the_new_flags():
    from cvc import main as cvc_main
    p = cvc_main.build_parser()
    o = p.parse_args([])
    assert (o.scheduled_sampling_start, o.scheduled_sampling_increase_every) == (-1, 5)
    assert (o.scheduled_sampling_increase_prob, o.scheduled_sampling_max_prob) == (0.05, 0.25)
    assert (o.scheduled_sampling_temperature, o.scheduled_sampling_seed) == (1.0, 1)
    o = p.parse_args(["--scheduled_sampling_start", "2", "--scheduled_sampling_increase_every", "3", "--scheduled_sampling_increase_prob",
                      "0.1", "--scheduled_sampling_max_prob", "0.5", "--scheduled_sampling_temperature", "0.7",
                      "--scheduled_sampling_seed", "9"])
    assert (o.scheduled_sampling_start, o.scheduled_sampling_increase_every, o.scheduled_sampling_increase_prob,
            o.scheduled_sampling_max_prob, o.scheduled_sampling_temperature, o.scheduled_sampling_seed) == (2, 3, 0.1, 0.5, 0.7, 9)
    # flags of cvc.main, not of the reference's option surface
    from cvc import opts as cvc_opts
    with pytest.raises(SystemExit):
        cvc_opts.build_parser().parse_args(["--scheduled_sampling_start", "2"])


def test_block_is_in_the_table_not_exported_and_checks_its_arguments_without_a_launch():
    import subprocess
    import build_hip
    from cvc import hip
    so = build_hip.build(verbose=False)
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cvc_hip_blocks.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^;]*)\)\s*;", src)
    assert m and len(m.group(1).split(",")) == len(hip.SIGNATURES[NAME]) == len(hip.SIGNATURES["cvc_sample_select_parts"]) + 6
    lib = ctypes.CDLL(so)
    lib.cvc_block.restype = ctypes.c_void_p
    lib.cvc_block.argtypes = [ctypes.c_char_p]
    assert lib.cvc_block(NAME.encode()) and NAME in hip.BLOCKS
    exported = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    assert not re.search(r"\b" + NAME + r"\b", exported)
    assert f"CVC_B({NAME})" in open(os.path.join(ROOT, "cyclical-visual-captioning_amd", "csrc", "blocks.hip")).read()
    fn = getattr(hip.lib(), NAME)
    fake = ctypes.c_void_p(16)

    def call(parts=fake, nparts=1, stride=0, M=4, V=50, inv_tau=1.0, state=fake, t=0, word=fake, wstride=1, given=fake, gstride=1,
             prob=fake):
        return fn(parts, nparts, stride, None, M, V, 1, inv_tau, state, t, word, wstride, None, given, gstride, prob, None, None, None,
                  None)

    # the checks of cvc_sample_select_parts ...
    assert call(parts=None) == -1 and call(state=None) == -1 and call(word=None) == -1 and call(t=-1) == -1
    assert call(inv_tau=0.0) == -1 and call(inv_tau=float("inf")) == -1 and call(inv_tau=float("nan")) == -1
    assert call(nparts=0) == -1 and call(M=0) == -1 and call(V=1) == -1 and call(wstride=0) == -1
    assert call(nparts=2, stride=10) == -1
    assert call(V=9000) == -2 and call(M=70000, V=8192 * 8) == -2
    # ... and its own
    assert call(given=None) == -1 and call(gstride=0) == -1 and call(prob=None) == -1


def test_engine_refuses_what_the_mixed_mode_does_not_combine_with():
    """validated before anything touches a GPU"""
    from cvc.decode import DecodeEngine
    new = lambda **kw: DecodeEngine.__init__(object.__new__(DecodeEngine), None, {}, 4, 1, mix=True, **kw)
    for kw in (dict(), dict(temperature=1.0, beam=3), dict(temperature=1.0, forced_n=1), dict(temperature=1.0, no_repeat_ngram=2),
               dict(temperature=1.0, no_immediate_repeat=True), dict(temperature=1.0, min_len=2), dict(temperature=1.0, ban_words=[3]),
               dict(temperature=1.0, bad_endings=[3]), dict(temperature=1.0, top_k=5), dict(temperature=1.0, top_p=0.9),
               dict(temperature=1.0, weights_dtype="bf16")):
        with pytest.raises(RuntimeError):
            new(**kw)
    with pytest.raises(RuntimeError, match="mix"):
        new(temperature=1.0, top_k=5)
    with pytest.raises(RuntimeError, match="bool"):
        DecodeEngine.__init__(object.__new__(DecodeEngine), None, {}, 4, 1, mix=1, temperature=1.0)
