"""Constrained decoding without a GPU: the building block in the library's table and its host-side argument checks, the engine's
refusals, the CLI's flags, and properties of the fp64 reference (tests/constrain_ref.py) on the CPU oracle's decodes."""
import ctypes
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

from cvc import synth
from oracle import ref_cpu as O
import sample_oracle as S
import constrain_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNK = synth.UNK_IDX
NAME = "cvc_constrained_select_parts"
BADARG, TOOBIG = -1, -2


# ------------------------------------------------------------------ the block: table, binding, argument checks
def test_block_is_in_the_table_and_bound_with_the_headers_argument_count():
    import subprocess
    import build_hip
    from cvc import hip
    so = build_hip.build(verbose=False)
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cvc_hip_blocks.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m
    nargs = len([a for a in m.group(1).split(",") if a.strip()])
    assert NAME in hip.BLOCKS and len(hip.SIGNATURES[NAME]) == nargs
    assert nargs == len(hip.SIGNATURES["cvc_sample_select_trunc_parts"]) + 4           # hist, hist_stride, descriptor, nbanned
    lib = ctypes.CDLL(so)
    lib.cvc_block.restype = ctypes.c_void_p
    lib.cvc_block.argtypes = [ctypes.c_char_p]
    assert lib.cvc_block(NAME.encode())
    exported = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    assert not re.search(r"\b" + NAME + r"\b", exported)                               # the exported ABI does not grow
    blocks_src = open(os.path.join(ROOT, "cyclical-visual-captioning_amd", "csrc", "blocks.hip")).read()
    assert f"CVC_B({NAME})" in blocks_src
    # the descriptor's layout is the C compiler's: 4 ints, 2 pointers, 1 int (padded)
    assert ctypes.sizeof(hip.Constraint) == 16 + 16 + 8 and hip.Constraint.ban.offset == 16 and hip.Constraint.nbad.offset == 32


def test_host_argument_checks_return_their_codes_and_launch_nothing():
    from cvc import hip
    fn = getattr(hip.lib(), NAME)
    fake = ctypes.c_void_p(16)

    def call(parts=fake, nparts=1, stride=0, M=4, V=50, inv_tau=1.0, k=0, p=1.0, state=fake, t=0, word=fake, hist=fake, hstride=4,
             n=0, imm=0, min_len=0, nban=0, ban=None, nbad=0, bad=None, desc=True):
        c = hip.Constraint(n, imm, min_len, nban, ban, bad, nbad) if desc else None
        return fn(parts, nparts, stride, None, M, V, 1, inv_tau, k, p, state, t, word, 1, None, None, None, hist, hstride, c, None, None)

    # too big: the history, the vocabulary, the hash counter
    assert call(t=65) == TOOBIG and call(V=8193) == TOOBIG and call(M=1 << 20, V=4096) == TOOBIG
    # the checks of the sampling blocks
    assert call(parts=None) == BADARG and call(word=None) == BADARG and call(state=None) == BADARG
    assert call(inv_tau=-1.0) == BADARG and call(inv_tau=float("inf")) == BADARG and call(inv_tau=float("nan")) == BADARG
    assert call(nparts=2, stride=10) == BADARG and call(t=-1) == BADARG
    assert call(k=-1) == BADARG and call(p=0.0) == BADARG and call(p=1.5) == BADARG and call(p=float("nan")) == BADARG
    # the rules
    assert call(n=-1) == BADARG and call(n=65) == BADARG and call(min_len=-1) == BADARG
    assert call(nban=-1, ban=fake) == BADARG and call(nban=257, ban=fake) == BADARG
    assert call(nbad=-1, bad=fake) == BADARG and call(nbad=257, bad=fake) == BADARG
    assert call(nban=3, ban=None) == BADARG and call(nbad=1, bad=None) == BADARG
    assert call(desc=False) == BADARG
    assert call(t=3, hist=None) == BADARG
    # arg-max mode: no state needed, but nothing to truncate
    assert call(inv_tau=0.0, k=5) == BADARG and call(inv_tau=0.0, p=0.5) == BADARG
    assert call(inv_tau=0.0, state=None, parts=None) == BADARG                        # (still checked)


# ------------------------------------------------------------------ the engine's refusals
def test_engine_refuses_before_anything_is_allocated():
    from cvc.decode import DecodeEngine
    W = types.SimpleNamespace(V=50, R=32, A=32, E=32)
    new = lambda T=4, W=W, feats=None, **kw: DecodeEngine.__init__(object.__new__(DecodeEngine), W, feats or {}, T, 1, **kw)
    with pytest.raises(RuntimeError, match="beam"):
        new(no_repeat_ngram=3, beam=3)
    with pytest.raises(RuntimeError, match="forced"):
        new(min_len=2, forced_n=1)
    for kw in (dict(gsk=True), dict(gate_ksplit=True), dict(lang_ksx=True)):
        with pytest.raises(RuntimeError, match="default schedules"):
            new(no_immediate_repeat=True, **kw)
    with pytest.raises(RuntimeError, match="T <= 64"):
        new(T=65, no_repeat_ngram=2)
    for kw in (dict(no_repeat_ngram=-1), dict(no_repeat_ngram=2.0), dict(no_repeat_ngram=True), dict(no_repeat_ngram=65),
               dict(min_len=-2), dict(min_len="3"), dict(no_immediate_repeat="yes"), dict(ban_words=[3, -1]), dict(ban_words=[2.5]),
               dict(ban_words=7), dict(bad_endings=["the"]), dict(bad_endings=[50]), dict(ban_words=[4, 50])):
        with pytest.raises(RuntimeError, match="no_repeat_ngram|min_len|no_immediate_repeat|ban_words|bad_endings"):
            new(**kw)
    with pytest.raises(RuntimeError, match="at most 256"):
        new(W=types.SimpleNamespace(V=1000, R=32, A=32, E=32), ban_words=list(range(257)))
    # top_k / top_p still need a temperature; sample_n > 1 too
    with pytest.raises(RuntimeError, match="temperature"):
        new(no_repeat_ngram=3, top_k=5)
    with pytest.raises(RuntimeError, match="temperature"):
        new(no_repeat_ngram=3, sample_n=2)
    # the packed path without the embedding-gate schedule: refused on the shapes alone (CPU tensors: nothing reaches a device)
    B, N, Fr = 2, 5, 3
    feats = dict(fc_feats=torch.zeros(B, 32), conv_feats=torch.zeros(B, Fr, 32), p_conv_feats=torch.zeros(B, Fr, 32),
                 pool_feats=torch.zeros(B, N, 32), p_pool_feats=torch.zeros(B, N, 32), pnt_mask=torch.zeros(B, N + 1))
    with pytest.raises(RuntimeError, match="embedding-gate"):
        new(feats=feats, min_len=2, embgate=False)


def test_flags_live_in_cvc_main_and_not_in_cvc_opts():
    from cvc import main as cvc_main, opts
    src_main, src_opts = inspect.getsource(cvc_main), inspect.getsource(opts)
    for flag in ("--no_repeat_ngram", "--no_immediate_repeat", "--min_caption_len", "--ban_words", "--bad_endings"):
        assert flag in src_main and flag not in src_opts and flag[2:] not in src_opts
    wtoi = {"a": 4, "the": 7, "of": 9}
    assert cvc_main.word_ids("a, the,12,of", wtoi, "--bad_endings") == [4, 7, 12, 9]
    assert cvc_main.word_ids("", wtoi, "--ban_words") == []
    with pytest.raises(SystemExit, match="zebra"):
        cvc_main.word_ids("a,zebra", wtoi, "--ban_words")


def test_model_reads_the_constraints_from_opts_with_defaults():
    from cvc.model import captioner
    src = inspect.getsource(captioner)
    for k in ("no_repeat_ngram", "no_immediate_repeat", "min_caption_len", "ban_word_ids", "bad_ending_ids"):
        assert re.search(r'getattr\(opts, "%s"' % k, src), k


# ------------------------------------------------------------------ the reference
def test_banned_by_hand():
    V = 12
    h = np.array([[5, 6, 5, 6, 5, 0, 0, 0]])
    ids = lambda t, **kw: sorted(np.flatnonzero(CR.banned(h, t, V, UNK, **kw)[0]).tolist())
    assert ids(0) == [UNK] and ids(5) == [UNK]
    assert ids(4, no_repeat_ngram=1) == [UNK, 5, 6]
    assert ids(3, no_repeat_ngram=2) == [UNK, 6]                  # history 5 6 5: "5 6" was seen
    assert ids(5, no_repeat_ngram=3) == [UNK, 6]                  # history 5 6 5 6 5: "6 5 6" was seen
    assert ids(4, no_repeat_ngram=3) == [UNK, 5]
    assert ids(1, no_repeat_ngram=3) == [UNK] and ids(2, no_repeat_ngram=3) == [UNK]      # t < n: no earlier window
    assert ids(3, no_immediate_repeat=True) == [UNK, 5] and ids(0, no_immediate_repeat=True) == [UNK]
    assert ids(2, min_len=3) == [0, UNK] and ids(3, min_len=3) == [UNK]
    assert ids(3, bad_endings=[5]) == [0, UNK] and ids(4, bad_endings=[5]) == [UNK] and ids(0, bad_endings=[5]) == [UNK]
    assert ids(2, ban_words=[3, 3, 11, 12, -1, UNK]) == [UNK, 3, 11]                   # ids outside [0, V) ban nothing
    # several matches ban different words
    h2 = np.array([[7, 2, 7, 3, 7, 4, 7]])
    assert sorted(np.flatnonzero(CR.banned(h2, 7, V, UNK, no_repeat_ngram=2)[0]).tolist()) == [UNK, 2, 3, 4]


def test_with_nothing_banned_the_reference_is_sample_oracles():
    g = torch.Generator().manual_seed(3)
    z = torch.randn(12, 50, generator=g) * 1.5
    z[::2, UNK] = 9.0
    noise = S.gumbel_noise(5, 2, 1, 12, 50)
    tau = 0.7
    inv_tau = float(np.float32(1.0 / tau))
    only_unk = CR.banned(np.zeros((12, 4), np.int64), 2, 50, UNK, no_repeat_ngram=64)
    assert only_unk.sum() == 12 and only_unk[:, UNK].all()
    w0, s0, lp0 = S.select(z, noise, tau, UNK)
    w, s, lp, info = CR.select(z, only_unk, noise, inv_tau)
    assert np.array_equal(w, w0) and not info["empty"].any()
    np.testing.assert_allclose(s[np.isfinite(s)], s0[np.isfinite(s0)], rtol=0, atol=1e-6)      # product with fp32 1 / tau vs quotient
    np.testing.assert_allclose(lp, lp0.double().numpy(), rtol=0, atol=1e-5)
    # arg-max mode: the arg-max without UNK
    wa, _, _, _ = CR.select(z, only_unk, None, 0.0)
    zz = z.clone()
    zz[:, UNK] = -float("inf")
    assert np.array_equal(wa, zz.argmax(1).numpy())
    # a row without an allowed word: word 0, log-prob -inf
    allb = np.ones((12, 50), bool)
    we, se, lpe, ie = CR.select(z, allb, noise, inv_tau)
    assert (we == 0).all() and np.isneginf(lpe).all() and ie["empty"].all() and np.isneginf(se).all()


def _case(name):
    d = synth.CONFIGS[name]
    return d, O.to_torch(synth.hot_path_state_dict(d, 4321)), O.to_torch(synth.clip_features(d, 4321))


@pytest.fixture(scope="module")
def greedy():
    out = {}
    with torch.no_grad():
        for name in ("tiny", "cfg1"):
            d, P, f = _case(name)
            out[name] = O.greedy_sample(P, f, d.T, UNK, return_logprobs=True)[0].numpy()
    return out


def test_the_unconstrained_decodes_repeat(greedy):
    """What the constraints are for, and why the properties below cannot hold vacuously: every row of both decodes repeats a word
    and a bigram, 3 of 4 cfg1 rows (and every tiny row) a trigram."""
    assert greedy["tiny"].tolist() == [[20] * 4] * 3
    assert greedy["cfg1"][1].tolist() == [3340, 1034, 2904, 2904, 3560, 3560, 3560, 3560, 3560, 2046]
    for name in ("tiny", "cfg1"):
        for n in (1, 2):
            assert CR.repeats_ngram(greedy[name], n).all(), (name, n)
    assert CR.repeats_ngram(greedy["tiny"], 3).all()
    assert CR.repeats_ngram(greedy["cfg1"], 3).sum() == 3


@pytest.mark.parametrize("name", ["tiny", "cfg1"])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_reference_decode_holds_no_repeated_ngram(greedy, name, n):
    d, P, f = _case(name)
    with torch.no_grad():
        plain = CR.decode(P, f, d.T, UNK)
        seq, att, lp, scores, info = CR.decode(P, f, d.T, UNK, no_repeat_ngram=n)
    assert np.array_equal(plain[0].numpy(), greedy[name]) and not plain[4]["fired"].any()       # no rule: the oracle's greedy decode
    seq = seq.numpy()
    assert not CR.repeats_ngram(seq, n).any() and not (seq == UNK).any()
    # the ban fired wherever the unconstrained decode repeats, and the decode is the greedy one up to the first firing
    fired = info["fired"].any(1)
    assert np.array_equal(fired, CR.repeats_ngram(greedy[name], n)) and fired.sum() >= (3 if n == 3 and name == "cfg1" else d.B)
    first = np.where(fired, info["fired"].argmax(1), d.T)
    for r in range(d.B):
        assert np.array_equal(seq[r, :first[r]], greedy[name][r, :first[r]])
        if fired[r]:
            assert seq[r, first[r]] != greedy[name][r, first[r]]
    assert (info["nbanned"] >= 1).all() and (info["nbanned"][:, 0] == 1).all()
    assert np.isfinite(lp.numpy()).all()


def eager_eos(P, delta):
    """the checkpoint with word 0's logit bias raised: a captioner that likes to stop (the synthetic ones never do)"""
    P = dict(P)
    P["logit.bias"] = P["logit.bias"].clone()
    P["logit.bias"][0] += delta
    return P


@pytest.mark.parametrize("name,delta,L", [("tiny", 0.2, 3), ("cfg1", 0.8, 6)])
def test_reference_decode_respects_lists_min_len_and_bad_endings(name, delta, L):
    d, P, f = _case(name)
    P = eager_eos(P, delta)
    with torch.no_grad():
        free = CR.decode(P, f, d.T, UNK, no_immediate_repeat=True)[0].numpy()
        # the rules have something to do: every free row stops before L, and puts its later stops behind these words
        assert (free[:, :L] == 0).any(1).all()
        bad = sorted(set(free[:, :-1][free[:, 1:] == 0].tolist()) - {0})
        ban = sorted(set(free[:, 0].tolist()) - {0}) or [int(free[0, 1])]
        assert bad and ban
        seq, _, lp, scores, info = CR.decode(P, f, d.T, UNK, no_immediate_repeat=True, min_len=L, bad_endings=bad, ban_words=ban)
    seq = seq.numpy()
    assert not np.isin(seq, ban + [UNK]).any()
    assert not (seq[:, :L] == 0).any()
    assert not (seq[:, 1:][np.isin(seq[:, :-1], bad)] == 0).any()
    assert not (seq[:, 1:] == seq[:, :-1]).any()
    assert info["fired"][:, :L].any(1).all()
    nb = info["nbanned"]
    assert (nb[:, 0] == 1 + 1 + len(ban)).all()                   # UNK, word 0 (min_len), the list; no history yet
    assert nb.max() <= 3 + len(ban)
