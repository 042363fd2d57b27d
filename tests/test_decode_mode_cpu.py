"""DecodeMode.resolve (cvc/decode/mode.py) against the recorded table tests/golden/decode_modes.json: for the empty call, every
single setting of decode_mode_cases.SETTINGS and every pair of them, the refusal that fires (message for message) or the
normalised options and derived flags -- as DecodeEngine.__init__ gave them on the commit before the mode was a value of its own.
Checked through the engine and on DecodeMode directly; no GPU."""
import dataclasses
import inspect

import pytest

import decode_mode_cases as MC


@pytest.fixture(scope="module")
def table():
    return MC.recorded()


def test_the_table_covers_the_grid(table):
    grid = MC.grid()
    assert len(grid) == 1 + len(MC.SETTINGS) + sum(1 for i, a in enumerate(MC.SETTINGS) for b in MC.SETTINGS[i + 1:] if not set(a) & set(b))
    assert [kw for kw, _ in table] == MC.plain(grid)
    assert all(set(out) in ({"refused"}, {"mode"}) for _, out in table)
    # every switch of the engine is in the settings (own_features / driver / seed / inv_temp / unk_idx choose no mode)
    from cvc.decode import DecodeEngine
    options = set(inspect.signature(DecodeEngine.__init__).parameters) - {"self", "weights", "feats", "unk_idx", "inv_temp", "own_features",
                                                                           "driver", "seed"}
    assert options == {k for s in MC.SETTINGS for k in s}


def test_the_engine_gives_the_recorded_outcomes(table):
    bad = [(kw, got, out) for kw, out in table for got in [MC.outcome(kw)] if got != out]
    assert not bad, (len(bad), bad[:3])


def test_resolve_gives_the_recorded_outcomes(table):
    from cvc.decode.mode import DecodeMode
    assert set(MC.FIELDS) <= {f.name for f in dataclasses.fields(DecodeMode)}
    bad = []
    for kw, out in table:
        T, args = MC.arguments(kw)
        args = {k: v for k, v in args.items() if k not in MC.ENGINE_ONLY}
        try:
            m = DecodeMode.resolve(T, MC.V, **args)
            got = {"mode": MC.plain({n: getattr(m, n) for n in MC.FIELDS if getattr(m, n) is not None})}
            assert m == DecodeMode.resolve(T, MC.V, **args) and hash(m) == hash(DecodeMode.resolve(T, MC.V, **args))
            # the schedule requests: untouched, or "off" in the modes that exclude the experimental schedules
            off = m.forced or m.constrained or m.sampling or m.bf16w
            assert (m.gate_ksplit, m.lang_ksx) == ((False, False) if off else (args.get("gate_ksplit"), args.get("lang_ksx")))
            assert m.gsk == (False if m.bf16w else args.get("gsk"))
        except RuntimeError as e:
            got = {"refused": str(e)}
        if got != out:
            bad.append((kw, got, out))
    assert not bad, (len(bad), bad[:3])


def test_mode_is_a_value():
    from cvc.decode.mode import DecodeMode
    a = DecodeMode.resolve(12, None, beam=4, beam_history=True, ban_words=[])
    assert a == DecodeMode.resolve(12, None, beam=4, beam_history=True) and len({a, DecodeMode.resolve(12, None, beam=4, beam_history=True)}) == 1
    assert a != DecodeMode.resolve(12, None, beam=4)
    with pytest.raises(dataclasses.FrozenInstanceError):
        a.beam = 1
    # flags: the mode's share of the key of DecodeEngine.capture's first, uncaptured decode -- these twelve, no option values
    m = DecodeMode.resolve(12, 50, beam=6, beam_history=True, force_n=2, length_penalty=0.7, ban_words=[3])
    assert m.flags == (m.beam > 1, m.sampling, m.weights_dtype, m.trunc, m.forced, m.constrained, m.beam_hist, m.grouped, m.ranked,
                       m.forcing, m.mix, m.stoch) == (True, False, "fp32", False, False, True, True, False, True, True, False, False)
    assert m.flags == DecodeMode.resolve(20, 50, beam=4, beam_history=True, force_n=1, min_len=2).flags
    assert DecodeMode.resolve(12, None, temperature=0.5, top_k=3).flags == DecodeMode.resolve(12, None, temperature=2.0, top_p=0.5, sample_n=4).flags


def test_the_mode_needs_no_device_and_no_library():
    """the module imports neither torch nor cvc.hip: the options are checked where nothing else is needed"""
    import cvc.decode.mode as mode
    src = inspect.getsource(mode)
    assert "import torch" not in src and "hip" not in {n for n in vars(mode) if not n.startswith("__")}


def test_every_refusal_of_resolve_is_in_the_table(table):
    """every `raise` of cvc/decode/mode.py is reached by a recorded case (traced line by line, standard library only)"""
    import sys
    import cvc.decode.mode as mode
    from cvc.decode.mode import DecodeMode
    path = inspect.getsourcefile(mode)
    lines = inspect.getsourcelines(mode)[0]
    raises = {i + 1 for i, l in enumerate(lines) if l.lstrip().startswith("raise ")}
    assert len(raises) >= 39
    hit = set()

    def tracer(frame, event, arg):
        if frame.f_code.co_filename != path:
            return None
        if event == "line" and frame.f_lineno in raises:
            hit.add(frame.f_lineno)
        return tracer
    old = sys.gettrace()
    sys.settrace(tracer)
    try:
        for kw, out in table:
            if "refused" in out:
                T, args = MC.arguments(kw)
                try:
                    DecodeMode.resolve(T, MC.V, **{k: v for k, v in args.items() if k not in MC.ENGINE_ONLY})
                except RuntimeError:
                    pass
    finally:
        sys.settrace(old)
    assert not raises - hit, [lines[n - 1].strip() for n in sorted(raises - hit)]


def test_the_engine_cache_key_is_made_of_the_options(monkeypatch):
    """captioner._decode_engine: two calls share an engine exactly when the weights, the feature shapes, softmax_temp, T, the graph
    switch, the caller's extra part and every option passed on agree (lists as tuples; `unkeyed` options apart); prepare() runs
    before capture on a new engine and after the features on a cached one; only may_bind re-points a driver-bound engine."""
    import types
    import torch
    from cvc.model import captioner
    log = []

    class Engine:
        def __init__(self, weights, feats, T, unk_idx, **kw):
            self.kw, self._plan, self.graph = dict(kw, T=T, unk_idx=unk_idx), None, None
            log.append("new")
        capture = lambda self: (log.append("capture"), setattr(self, "graph", object()))
        load_features = lambda self, feats: log.append("load")
        bind_features = lambda self, feats: log.append("bind")
    monkeypatch.setattr(captioner, "DecodeEngine", Engine)
    feats = dict(fc_feats=torch.zeros(2, 8), conv_feats=torch.zeros(2, 3, 8), pool_feats=torch.zeros(2, 5, 8))
    model = types.SimpleNamespace(opts=types.SimpleNamespace(softmax_temp=2.0), use_hip_graph=True, unk_idx=7, decode_weights=lambda W=object(): W)
    get = lambda slot="_engine_cache", feats=feats, T=6, **kw: captioner.DecodeAndGroundCaptionerGVDROI._decode_engine(model, slot, feats, T, **kw)
    prepare = lambda e: log.append("prepare")
    e = get(beam=3, ban_words=[3, 4], prepare=prepare)
    assert log == ["new", "prepare", "capture"] and e.kw == dict(beam=3, ban_words=[3, 4], T=6, unk_idx=7, inv_temp=0.5, own_features=True)
    assert model._engine_cache[1] is e and isinstance(hash(model._engine_cache[0]), int)
    del log[:]
    assert get(beam=3, ban_words=(3, 4), prepare=prepare) is e and log == ["load", "prepare"]
    assert get(beam=3, ban_words=(3, 4), may_bind=True) is e            # (a captured graph keeps its pointers: no re-pointing)
    e.graph, e._plan = None, object()
    del log[:]
    assert get(beam=3, ban_words=(3, 4), may_bind=True) is e and get(beam=3, ban_words=(3, 4)) is e and log == ["bind", "load"]
    # any option, the caller's extra part, T, a feature shape, softmax_temp, the graph switch, the weights: another engine
    for change in (dict(beam=4), dict(ban_words=(3,)), dict(top_k=0), dict(extra=(True,)), dict(T=7),
                   dict(feats=dict(feats, pool_feats=torch.zeros(2, 6, 8)))):
        e = get(beam=3, ban_words=(3, 4))
        assert get(beam=3, ban_words=(3, 4)) is e and get(**{**dict(beam=3, ban_words=(3, 4)), **change}) is not e
    for attr, value in (("use_hip_graph", False), ("opts", types.SimpleNamespace(softmax_temp=1.0)), ("decode_weights", lambda W=object(): W)):
        e = get(beam=3, ban_words=(3, 4))
        setattr(model, attr, value)
        assert get(beam=3, ban_words=(3, 4)) is not e
    # an unkeyed option reaches a new engine and does not distinguish cached ones; the slots are independent
    e = get("_ss_cache", unkeyed=("seed",), seed=1, mix=True)
    assert e.kw["seed"] == 1 and get("_ss_cache", unkeyed=("seed",), seed=2, mix=True) is e and get("_ss_cache", seed=2, mix=True) is not e
    assert model._engine_cache[1] is not model._ss_cache[1]
