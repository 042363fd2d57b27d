"""The cases of tests/test_decode_mode_cpu.py: what DecodeEngine's mode resolution (cvc/decode/mode.py) makes of its option
arguments -- the refusal that fires, or the normalised options and derived flags -- for the empty call, every single setting below
and every pair of settings that do not set the same argument.  tests/golden/decode_modes.json holds the outcomes as recorded on the
commit before DecodeMode existed (the checks then stood in DecodeEngine.__init__); a pull request that adds a decode mode adds
its settings here and re-records the table by running this module as a script: the JSON diff shows which combinations changed.
No GPU, no built library: the engine is constructed on a bare object without features and stops at the first feature it reads."""
import hashlib
import json
import os
import sys
import types

T_DEFAULT, V = 4, 50
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_modes.json")

# what a resolved mode consists of (DecodeEngine attributes of the same names); inv_tau / stoch_inv_tau exist only in the modes
# that read them
FIELDS = ("forced", "constrained", "mix", "beam_hist", "grouped", "forcing", "ranked", "stoch", "sampling", "given", "trunc", "bf16w",
          "nq", "cons", "groups", "diversity", "length_penalty", "force_n", "top_k", "top_p", "inv_tau", "stoch_inv_tau",
          "weights_dtype")
ENGINE_ONLY = ("tail",)               # arguments the engine checks against the batch and the library, not the mode

# Every switch at an on value ("T" is the engine's T, not an option), then the combinations that are needed to get past the first
# refusal of a mode (a stochastic / forcing / grouped beam, a mixed sampler), then one malformed value for every argument that is
# type- or range-checked.  Non-finite numbers are written as strings ("nan", "inf"): _value() converts them.
SETTINGS = [
    dict(beam=4), dict(beam=4, beam_history=True), dict(beam_history=True), dict(temperature=0.7), dict(sample_n=3),
    dict(sample_n=3, temperature=1.3), dict(top_k=5), dict(top_p=0.9), dict(forced_n=2), dict(no_repeat_ngram=2),
    dict(no_immediate_repeat=True), dict(min_len=3), dict(ban_words=[3, 3, 7]), dict(ban_words=[60]), dict(bad_endings=[4]),
    dict(beam_groups=2), dict(beam_groups=3), dict(diversity=0.5), dict(length_penalty=0.7), dict(force_n=1), dict(force_n=2),
    dict(mix=True), dict(stochastic=True), dict(stochastic_tau=0.0), dict(stochastic_tau=0.5), dict(weights_dtype="bf16"),
    dict(gsk=True), dict(gate_ksplit=True), dict(gate_ksplit="fused"), dict(lang_ksx=True), dict(path="tile"), dict(path="ring"),
    dict(embgate=False), dict(tail="fused"), dict(T=65),
    dict(beam=4, beam_history=True, stochastic=True), dict(beam=4, beam_history=True, force_n=1),
    dict(beam=6, beam_history=True, force_n=2), dict(beam=4, beam_history=True, beam_groups=2), dict(temperature=0.7, mix=True),
    # malformed
    dict(mix=1), dict(top_k=-1), dict(top_p=0.0), dict(top_p="nan"), dict(forced_n=-1), dict(force_n=4), dict(beam_groups=0),
    dict(diversity=-1), dict(diversity="nan"), dict(length_penalty=-0.5), dict(ban_words=list(range(257))), dict(ban_words=[-1]),
    dict(bad_endings=5), dict(no_repeat_ngram=65), dict(min_len=-1), dict(no_immediate_repeat=2), dict(weights_dtype="fp16"),
    dict(beam_history=1), dict(stochastic=1), dict(stochastic_tau="inf"), dict(temperature=0.0), dict(temperature="inf"),
    dict(sample_n=0),
]


def _value(v):
    return float(v) if v in ("nan", "inf", "-inf") else v


def arguments(kw):
    """a case as written here -> (T, the engine's keyword arguments)"""
    kw = {k: _value(v) for k, v in kw.items()}
    return kw.pop("T", T_DEFAULT), kw


def rows():
    """the grid, one row per setting: [the empty case, every single setting], then for each setting its pairs with the later
    settings that do not set the same argument"""
    return [[{}] + [dict(s) for s in SETTINGS]] + [[{**a, **b} for b in SETTINGS[i + 1:] if not set(a) & set(b)]
                                                   for i, a in enumerate(SETTINGS)]


def grid():
    return [kw for row in rows() for kw in row]


def plain(x):
    """x as it reads after a trip through JSON (tuples are lists there)"""
    return json.loads(json.dumps(x))


def weights():
    return types.SimpleNamespace(V=V, R=32, A=32, E=32)


def outcome(kw):
    """What the engine makes of a case: {"refused": message}, or {"mode": the FIELDS present on the half-built engine} when the
    options pass and the constructor goes on to read the (missing) features."""
    from cvc.decode import DecodeEngine
    T, kw = arguments(kw)
    eng = object.__new__(DecodeEngine)
    try:
        DecodeEngine.__init__(eng, weights(), {}, T, 1, **kw)
    except RuntimeError as e:
        return {"refused": str(e)}
    except KeyError as e:
        assert e.args == ("fc_feats",), e
        return {"mode": plain({n: getattr(eng, n) for n in FIELDS if hasattr(eng, n)})}
    raise AssertionError(f"the engine was built without features: {kw}")


# The fixture: "default" = the mode of the empty call; "outcomes" = every distinct outcome under a short key (the first hex digits
# of its SHA-1: adding one renames no other), a mode as its difference from the default; "rows" = the keys of rows(), each row
# labelled with its setting -- a changed combination shows as a changed key in the row of its first setting.
def _key(out):
    return hashlib.sha1(json.dumps(out, sort_keys=True).encode()).hexdigest()[:5]


def _dumps(x):
    return json.dumps(x, sort_keys=True, separators=(",", ":"))


def write(outcomes):
    """outcomes: outcome(kw) for kw in grid()"""
    default = outcomes[0]["mode"]
    short = lambda o: o if "refused" in o else {"mode": {k: v for k, v in o["mode"].items() if k not in default or default[k] != v}}
    assert all(set(default) <= set(o["mode"]) for o in outcomes if "mode" in o)
    table = {_key(o): short(o) for o in outcomes}
    assert len(table) == len({_dumps(o) for o in outcomes}), "two outcomes share a key: lengthen _key"
    keys, lines = iter(outcomes), []
    for label, row in zip([{}] + SETTINGS, rows()):
        lines.append(_dumps([label, " ".join(_key(next(keys)) for _ in row)]))
    with open(GOLDEN, "w") as f:
        f.write('{"default": ' + _dumps(default) + ',\n"outcomes": {\n' + ",\n".join(f'"{k}": {_dumps(table[k])}' for k in sorted(table)) +
                '},\n"rows": [\n' + ",\n".join(lines) + "\n]}\n")


def recorded():
    """-> [(kw, outcome)] in grid() order"""
    with open(GOLDEN) as f:
        z = json.load(f)
    assert [label for label, _ in z["rows"]] == plain([{}] + SETTINGS)
    full = lambda o: o if "refused" in o else {"mode": {**z["default"], **o["mode"]}}
    out = [full(z["outcomes"][k]) for _, row in z["rows"] for k in row.split()]
    assert len(out) == len(grid())
    return list(zip(plain(grid()), out))


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "cyclical-visual-captioning_amd")]
    outcomes = [outcome(kw) for kw in grid()]
    write(outcomes)
    refused = {o["refused"] for o in outcomes if "refused" in o}
    print(f"{len(outcomes)} cases, {sum('refused' in o for o in outcomes)} refused with {len(refused)} distinct messages -> {GOLDEN}")
