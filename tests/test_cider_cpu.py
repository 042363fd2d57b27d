"""CIDEr-D table, the two building blocks' surface and the self-critical flags -- everything that needs no GPU."""
import ctypes
import math
import os
import subprocess
import types

import numpy as np
import pytest
import torch

import cider_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _corpus(seed=0, n=60, V=11, T=9):
    rng = np.random.default_rng(seed)
    caps = []
    for _ in range(n):
        L = int(rng.integers(1, T + 1))
        c = np.zeros(T, dtype=np.int64)
        c[:L] = rng.integers(1, V, L)
        if L == T and rng.random() < 0.5:
            pass                               # a caption that never ends
        elif L == T:
            c[T - 1] = 0
        caps.append(c)
    return caps


def test_restatement_on_hand_cases():
    """the two values of the definition's hand check: an identical pair with L = 2 scores 5 (two of the four orders exist), a
    full-length identical pair 10"""
    corpus = _corpus()
    df, n_doc = R.doc_freq(corpus)
    s, parts = R.score([3, 0, 0, 0, 0, 0], [[3, 0, 0, 0, 0, 0]], df, n_doc)
    assert abs(s - 5.0) < 1e-12 and parts[2] == 0 and parts[3] == 0
    full = [1, 2, 3, 4, 5, 6]
    assert abs(R.score(full, [full], df, n_doc)[0] - 10.0) < 1e-12
    assert R.score(full, [], df, n_doc)[0] == 0


def test_table_against_the_restatement():
    from cvc.cider import CiderD
    corpus = _corpus()
    df, n_doc = R.doc_freq(corpus)
    t = CiderD.from_captions(corpus)
    keys = t.keys_host
    assert keys.dtype == np.uint64 and len(keys) == len(df) == len(t)
    assert np.all(keys[1:] > keys[:-1])                                           # unique, ascending as unsigned values
    want = {R.key(g): np.float32(R.idf64(df, n_doc, g)) for g in df}
    assert set(int(k) for k in keys) == set(want)
    for k, v in zip(keys.tolist(), t.idf_host.tolist()):
        assert np.float32(v) == want[int(k)], (hex(k), v, want[int(k)])          # the fp64 value rounded to fp32
    assert t.idf_host.dtype == np.float32
    assert t.n_doc == n_doc and t.idf_unseen == math.log(n_doc)
    # the order is part of the key: a unigram's key has one non-zero field, in the highest bits
    assert R.key((4,)) == 5 << 48 and R.key((4, 0)) == (5 << 48) | (1 << 32)
    # torch tensors are taken too, and the top bit survives the int64 storage
    big = CiderD.from_captions([torch.tensor([65534, 3, 0])])
    assert int(big.keys_host.max()) >> 48 == 65535
    assert big.keys_host.view(np.int64).min() < 0


def test_table_refusals():
    from cvc.cider import CiderD
    with pytest.raises(RuntimeError, match="65535"):
        CiderD.from_captions([np.array([1, 65535, 0])])
    with pytest.raises(RuntimeError, match="63"):
        CiderD.from_captions([np.ones(64, dtype=np.int64)])
    CiderD.from_captions([np.ones(63, dtype=np.int64), np.array([65534, 0])])        # the limits themselves are fine


def test_from_dataset_reads_the_items_captions():
    from cvc.cider import CiderD

    class DS:
        def __len__(self):
            return 2

        def __getitem__(self, i):
            gt = torch.zeros(10, 5, dtype=torch.int64)
            gt[0, :3] = torch.tensor([1 + i, 2, 3])
            gt[1, :2] = torch.tensor([7, 8])          # beyond num[0]: not a caption
            return (None, None, gt, torch.tensor([1.0, 0, 0]))
    t = CiderD.from_dataset(DS())
    want = CiderD.from_captions([np.array([1, 2, 3, 0, 0]), np.array([2, 2, 3, 0, 0])])
    assert t.n_doc == 2 and np.array_equal(t.keys_host, want.keys_host) and np.array_equal(t.idf_host, want.idf_host)


def test_blocks_declared_listed_bound_and_not_exported():
    import build_hip
    from cvc import hip
    from test_cabi import declared_functions, BLOCKS_H
    names = ("cvc_cider_d", "cvc_scst_weights")
    lib = hip.lib()
    lib.cvc_block.restype = ctypes.c_void_p
    declared = declared_functions(BLOCKS_H)
    out = subprocess.check_output(["nm", "-D", "--defined-only", build_hip.build(verbose=False)], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for n in names:
        assert n in declared and n in hip.BLOCKS and n in hip.SIGNATURES
        assert lib.cvc_block(n.encode())
        assert n not in exported


def test_bad_arguments_return_badarg_before_any_launch():
    from cvc import hip
    lib = hip.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)                    # non-null; never dereferenced: every call below is refused on the host

    def cider(cand=p, refs=p, nref=p, rows=4, T=5, per=2, Rmax=1, keys=p, idf=p, G=1, sigma=6.0, reward=p):
        return lib.cvc_cider_d(cand, refs, nref, rows, T, per, Rmax, keys, idf, G, 1.0, sigma, reward, None, None)
    assert cider(cand=None) == -1 and cider(refs=None) == -1 and cider(nref=None) == -1 and cider(reward=None) == -1
    assert cider(keys=None) == -1 and cider(idf=None) == -1
    assert cider(T=0) == -1 and cider(T=64) == -1
    assert cider(rows=5) == -1                   # rows % per_clip != 0
    assert cider(Rmax=0) == -1 and cider(G=-1) == -1 and cider(rows=0) == -1 and cider(sigma=0.0) == -1

    def weights(reward=p, base=None, rows=4, per=2, cand=p, T=5, adv=p, w=p):
        return lib.cvc_scst_weights(reward, base, rows, per, cand, T, 0, adv, w, None)
    assert weights(reward=None) == -1 and weights(cand=None) == -1 and weights(adv=None) == -1 and weights(w=None) == -1
    assert weights(rows=5) == -1 and weights(T=0) == -1 and weights(rows=0) == -1
    assert weights(base=p) == -1                 # a baseline is given with one sample per clip only ...
    assert weights(per=1) == -1                  # ... and then it must be given


def test_wrappers_refuse_shapes_that_do_not_fit_and_cpu_tensors():
    from cvc import hip
    from cvc.cider import CiderD
    t = CiderD.from_captions([np.array([1, 2, 0])])
    keys, idf = torch.from_numpy(t.keys_host.view(np.int64).copy()), torch.from_numpy(t.idf_host.copy())
    cand, refs, nref = torch.zeros(4, 3, dtype=torch.int64), torch.zeros(2, 1, 3, dtype=torch.int64), torch.ones(2, dtype=torch.int32)
    for bad in (dict(cand=cand[:3]), dict(refs=refs[:, :, :2]), dict(nref=nref[:1]), dict(idf=idf[:1])):
        kw = dict(cand=cand, refs=refs, nref=nref, keys=keys, idf=idf)
        kw.update(bad)
        with pytest.raises(RuntimeError, match="do not fit"):
            hip.cider_d(kw["cand"], kw["refs"], kw["nref"], kw["keys"], kw["idf"], t.idf_unseen)
    with pytest.raises(RuntimeError, match="GPU"):                       # no CPU fallback
        hip.cider_d(cand, refs, nref, keys, idf, t.idf_unseen)
    with pytest.raises(RuntimeError, match="do not fit"):
        hip.scst_weights(torch.zeros(3), None, 2, cand)
    with pytest.raises(RuntimeError, match="GPU"):
        hip.scst_weights(torch.zeros(4), None, 2, cand)
    with pytest.raises(RuntimeError, match="63"):
        t.score(torch.zeros(2, 64, dtype=torch.int64), torch.zeros(2, 1, 64, dtype=torch.int64), nref)


def test_flags_live_in_main_not_in_opts():
    from cvc import main as cvc_main
    from cvc import opts as cvc_opts
    o = cvc_main.build_parser().parse_args(["--scst_after", "3", "--scst_samples", "4", "--scst_temperature", "0.8", "--scst_seed", "9",
                                            "--scst_dropout"])
    assert (o.scst_after, o.scst_samples, o.scst_temperature, o.scst_seed, o.scst_dropout) == (3, 4, 0.8, 9, True)
    d = cvc_main.build_parser().parse_args([])
    assert (d.scst_after, d.scst_samples, d.scst_temperature, d.scst_seed, d.scst_dropout) == (-1, 5, 1.0, 1, False)
    ref = cvc_opts.build_parser().parse_args([])
    assert not any(k.startswith("scst") for k in vars(ref))
    with pytest.raises(SystemExit):
        cvc_opts.build_parser().parse_args(["--scst_after", "3"])


def _stub_trainer(monkeypatch, scst_after):
    from cvc import trainer as tr

    class Loader(list):
        pass
    monkeypatch.setattr(tr, "DevicePrefetcher", lambda loader, prepare, device, limit=None: iter(list(loader)[:limit]))
    opts = types.SimpleNamespace(att_model="cyclical", batch_size=2, seq_per_img=1, disp_interval=1, hip_graph=0, scst_after=scst_after)
    t = tr.Trainer(opts, None, torch.nn.Linear(1, 1), None, Loader([{}] * 4), None)
    calls = dict(xe=0, scst=0)

    def xe(b):
        calls["xe"] += 1
        return tuple(torch.zeros(()) for _ in range(5))

    def scst(b):
        calls["scst"] += 1
        return torch.tensor(0.5), torch.tensor(2.0 * calls["scst"]), torch.tensor(1.0), torch.tensor(0.25)
    monkeypatch.setattr(t, "train_step_prepared", xe)
    monkeypatch.setattr(t, "scst_step_prepared", scst)
    return t, calls


def test_train_never_takes_a_self_critical_step_by_default(monkeypatch, capsys):
    t, calls = _stub_trainer(monkeypatch, -1)
    for epoch in range(3):
        t.train(epoch)
    assert calls == dict(xe=9, scst=0) and t.reward_history == {}
    assert "Reward" not in capsys.readouterr().out


def test_train_takes_self_critical_steps_from_scst_after_on(monkeypatch, capsys):
    t, calls = _stub_trainer(monkeypatch, 1)
    t.train(0)
    assert calls == dict(xe=3, scst=0)
    t.train(1)
    assert calls == dict(xe=3, scst=3)
    assert t.reward_history == {1: [2.0, 4.0, 6.0]}                     # the mean reward of every display interval
    assert "Reward 6.0000" in capsys.readouterr().out
