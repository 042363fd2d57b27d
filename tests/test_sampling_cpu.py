"""Sampled decoding without a GPU: the host mirror of the noise, the CPU reference sampler (tests/sample_oracle.py) against the
greedy oracle and against the distribution it samples from, and the new building blocks in the library's block table."""
import os
import re

import numpy as np
import pytest
import torch

from cvc import synth
from oracle import ref_cpu as O
import sample_oracle as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tiny_inputs(seed=99):
    d = synth.CONFIGS["tiny"]
    return d, O.to_torch(synth.hot_path_state_dict(d, seed)), O.to_torch(synth.clip_features(d, seed))


def test_noise_mirror_is_inside_the_open_interval_and_finite():
    h = np.array([0, 1, 511, 512, 0x7FFFFFFF, 0xFFFFFDFF, 0xFFFFFFFF], dtype=np.uint32)
    u = S.uniform_from_hash(h)
    assert (u > 0).all() and (u < 1).all()
    # the documented end points: 2^-24 and 1 - 2^-24, both exact in fp32
    assert u[0] == 2.0 ** -24 and u[-1] == 1.0 - 2.0 ** -24
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)
    g = S.gumbel_from_hash(h)
    assert np.isfinite(g).all()
    np.testing.assert_allclose(g[0], -np.log(-np.log(2.0 ** -24)), rtol=0, atol=0)
    np.testing.assert_allclose(g[[0, -1]], [-2.8115409, 16.6355323], atol=1e-6)
    # one hash value of the generator, pinned: seed (7, 9), call 1, step 0, counter 0
    h0 = synth.dropout_hash(7, 9, 1, S.SAMPLE_SITE, np.array([0, 1], dtype=np.uint32))
    assert h0.tolist() == [0x02010EE3, 0xD6DCADC0]
    np.testing.assert_allclose(S.gumbel_from_hash(h0), [-1.5789715, 1.7419332], atol=1e-6)
    assert np.array_equal(S.gumbel_noise(7 | (9 << 32), 1, 0, 1, 2)[0], S.gumbel_from_hash(h0))


def test_noise_depends_on_seed_call_step_and_element():
    base = S.gumbel_noise(5, 1, 0, 4, 50)
    for other in (S.gumbel_noise(6, 1, 0, 4, 50), S.gumbel_noise(5, 2, 0, 4, 50), S.gumbel_noise(5, 1, 1, 4, 50)):
        assert not np.array_equal(base, other)
    # rows are addressed by their counter r * V + v only: a window of rows is a slice of the whole
    assert np.array_equal(S.gumbel_noise(5, 1, 0, 2, 50, row0=2), base[2:])
    # Gumbel(0, 1): mean = Euler's constant, variance = pi^2 / 6
    g = S.gumbel_noise(11, 1, 0, 400, 500)
    assert abs(g.mean() - 0.5772157) < 0.01 and abs(g.var() - np.pi ** 2 / 6) < 0.03


def test_oracle_at_a_tiny_temperature_is_greedy():
    d, P, f = tiny_inputs()
    with torch.no_grad():
        seq_g, att_g, lp_g, _ = O.greedy_sample(P, f, d.T, synth.UNK_IDX, return_logprobs=True)
        seq, att, lp, _ = S.sample(P, f, d.T, synth.UNK_IDX, n=1, tau=1e-4, seed=3, call=1)
    assert torch.equal(seq, seq_g)
    np.testing.assert_allclose(att.numpy(), att_g.numpy(), rtol=0, atol=0)
    np.testing.assert_allclose(lp.numpy(), lp_g.numpy(), rtol=0, atol=1e-6)


def test_oracle_never_samples_unk():
    d, P, f = tiny_inputs()
    # make UNK the most likely word by far at every step: it must still never be drawn
    P = dict(P)
    b = P["logit.bias"].clone()
    b[synth.UNK_IDX] = 50.0
    P["logit.bias"] = b
    with torch.no_grad():
        seq, _, lp, scores = S.sample(P, f, d.T, synth.UNK_IDX, n=8, tau=2.0, seed=1, call=1)
    assert not (seq == synth.UNK_IDX).any()
    assert np.isneginf(scores[..., synth.UNK_IDX]).all()
    # the log-prob is over the full vocabulary, UNK included: the sampled words are unlikely under it
    assert float(lp.max()) < -10.0


@pytest.mark.parametrize("tau", [0.5, 1.0, 2.0])
def test_one_step_distribution_matches_softmax_without_unk(tau):
    """Step 0 of every row of a clip sees the same logits; the rows differ only through the noise.  Counts over 4 000 rows per
    clip against softmax(z / tau) restricted to v != UNK (fixed seed: deterministic)."""
    d, P, f = tiny_inputs()
    n = 4000
    with torch.no_grad():
        out, _, _, _, _ = O.decoder_step(P, O.embed(P, torch.zeros(d.B, dtype=torch.long)), f["fc_feats"], f["conv_feats"],
                                         f["p_conv_feats"], f["pool_feats"], f["p_pool_feats"], f["pnt_mask"][:, 1:],
                                         O.init_hidden(d.B, d.R))
        z = torch.nn.functional.linear(out, P["logit.weight"], P["logit.bias"])
    zr = z.repeat_interleave(n, 0)
    word, _, _ = S.select(zr, S.gumbel_noise(2024, 1, 0, d.B * n, d.V), tau, synth.UNK_IDX)
    for b in range(d.B):
        counts = np.bincount(word[b * n:(b + 1) * n], minlength=d.V)
        assert counts[synth.UNK_IDX] == 0
        p = torch.softmax(z[b].double() / tau, 0).numpy()
        p[synth.UNK_IDX] = 0.0
        p /= p.sum()
        stat, df = S.chi_square(counts, p)
        assert stat < S.chi_square_critical(df), (b, tau, stat, df)


def test_sampling_blocks_are_in_the_block_table_and_not_exported():
    """cvc_sample_select_parts / cvc_sample_advance: declared in include/cvc_hip_blocks.h, bound through cvc_block(), absent from
    the dynamic symbol table (the exported ABI stays include/cvc_hip.h)."""
    import ctypes
    import subprocess
    import build_hip
    from cvc import hip
    so = build_hip.build(verbose=False)
    names = ("cvc_sample_select_parts", "cvc_sample_advance")
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
    # host-side argument checks (no launch): null pointers, a temperature that is not positive, V beyond the register cache
    assert L.cvc_sample_advance(None, None) == -1
    assert L.cvc_sample_select_parts(None, 1, 0, None, 4, 50, 1, 1.0, None, 0, None, 1, None, None) == -1
    fake = ctypes.c_void_p(16)
    assert L.cvc_sample_select_parts(fake, 1, 0, None, 4, 50, 1, 0.0, fake, 0, fake, 1, None, None) == -1
    assert L.cvc_sample_select_parts(fake, 1, 0, None, 4, 50, 1, float("inf"), fake, 0, fake, 1, None, None) == -1
    assert L.cvc_sample_select_parts(fake, 1, 0, None, 4, 9000, 1, 1.0, fake, 0, fake, 1, None, None) == -2
    assert L.cvc_sample_select_parts(fake, 2, 10, None, 4, 50, 1, 1.0, fake, 0, fake, 1, None, None) == -1


def test_engine_refuses_what_sampling_does_not_combine_with():
    """The sampling options are validated before anything touches a GPU."""
    from cvc.decode import DecodeEngine
    with pytest.raises(RuntimeError, match="beam"):
        DecodeEngine.__init__(object.__new__(DecodeEngine), None, {}, 4, 1, beam=3, temperature=1.0)
    with pytest.raises(RuntimeError, match="gsk"):
        DecodeEngine.__init__(object.__new__(DecodeEngine), None, {}, 4, 1, gsk=True, temperature=1.0)
    with pytest.raises(RuntimeError, match="temperature"):
        DecodeEngine.__init__(object.__new__(DecodeEngine), None, {}, 4, 1, temperature=0.0)
    with pytest.raises(RuntimeError, match="temperature"):
        DecodeEngine.__init__(object.__new__(DecodeEngine), None, {}, 4, 1, sample_n=3)
