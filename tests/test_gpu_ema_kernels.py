"""The weight average inside the optimizer step on the GPU (csrc/optim.hip: optim_adam_ema_kernel, optim_sgd_ema_kernel,
optim_adamax_ema_kernel and optim_finalize_ema_kernel behind cvc_adam / sgd / adamax_clip_step_ema; ema_swap_kernel behind
cvc_ema_swap), driven through the C entries over hand-built tables, against tests/ema_ref.py (proven on the CPU in
tests/test_ema_ref_cpu.py).

The method is tests/test_gpu_optim_kernels.py's: every table is ONE step from known operands; p, g, the rule's state, the step
counts, the kernels' scratch and -- in an arena of its own -- the shadows e live between bands of 64 sentinel floats with sentinel
gaps between the segments.  Every table is stepped twice from the same host operands: by the PLAIN entry on one set of arenas and by
the _ema entry on another.  p, g, the state, the step counts and norm_coef must agree bit for bit (the plain entry is what
tests/test_gpu_optim_kernels.py and tests/test_gpu_optim_rules.py hold to fp64); e is held to K x the bound of ema_ref.ema_fp64
under the device's own p_new and d_eff, and keeps its bits where p_new == e (a third of every table's shadows is built from the
plain run's p_new).  One table = the nine sizes x the eight alignment forms of (p, e), 72 segments.  Every comparison prints its
max ratio |err| / (K x bound) (run with -s).

Measured on an MI355X (K = 4; 1 = at the bound): e 0.25 for Adam, for SGD with and without a buffer and for Adamax, on every
table -- the fma's own rounding next to a power of two fills its u |e_new|, 1.0 of the bound without K.  The file takes 6 s."""
import numpy as np
import pytest
import torch

import ema_ref as ER
import optim_ref as OR
from optim_ref import BAND, CHUNK, SENTINEL, U

pytestmark = pytest.mark.gpu

BADARG = -1
F = np.float32
SIZES = (1, 3, 4, 5, 255, 1025, CHUNK - 1, CHUNK + 1, 2 * CHUNK + 3)
# (offset of p, offset of e) inside their 16-byte-aligned slots, in floats: e aligned and off by 1, 2, 3, alone and with a misaligned p
FORMS = ((0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 1), (2, 2), (3, 3))
RULES = ("adam", "sgd", "sgd0", "adamax")              # sgd0: no momentum buffer
KEYS = {"adam": "pgmv", "sgd": "pgm", "sgd0": "pg", "adamax": "pgmv"}
BETAS, EPS, MOM = (0.9, 0.999), 1e-8, 0.9


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a visible MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def L(dev):
    from cvc import hip
    lib = hip.lib()
    assert lib.cvc_optim_chunk_elems() == CHUNK
    return lib


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


class Layout:
    """segments of `ns` elements, segment i at slot + offs[i][k] of arena k; BAND sentinels at both ends, >= 4 between two slots"""

    def __init__(self, ns, forms):
        self.ns = list(ns)
        self.forms = list(forms)                      # (p offset, e offset); g, m, v follow p's slot alignment (offset 0)
        pos, self.starts = BAND, []
        for n in self.ns:
            self.starts.append(pos)
            pos += (n + 3 + 3) // 4 * 4 + 4
        self.size = pos + BAND
        self.off = np.concatenate(([0], np.cumsum(self.ns)))
        self.total = int(self.off[-1])

    def index(self, k):
        o = {"p": 0, "e": 1}
        return np.concatenate([np.arange(a + (f[o[k]] if k in o else 0), a + (f[o[k]] if k in o else 0) + n)
                               for n, a, f in zip(self.ns, self.starts, self.forms)])

    def first(self, k, i):
        o = {"p": 0, "e": 1}
        return self.starts[i] + (self.forms[i][o[k]] if k in o else 0)


def seeded(total, rule, seed):
    rng = np.random.default_rng(seed)
    scales = np.array([1e-3, 1.0, 30.0])
    g = rng.standard_normal(total) * scales[rng.integers(0, 3, total)]
    g[rng.random(total) < 0.1] = 0.0
    v = (np.abs(rng.standard_normal(total)) * scales[rng.integers(0, 3, total)]) ** 2
    if rule == "adamax":
        v = np.sqrt(v) + 1e-3                          # exp_inf: a magnitude
    m = np.sqrt(np.abs(v)) * rng.uniform(-1.0, 1.0, total)
    return dict(p=rng.standard_normal(total).astype(F), g=g.astype(F), m=m.astype(F), v=v.astype(F))


class Side:
    """one set of arenas + tables for one entry (plain or _ema) over a Layout"""

    def __init__(self, dev, lay, rule, host, e_host=None, null=()):
        from cvc.optim import _CHUNK_DT, _SEG_DT
        self.dev, self.lay, self.rule, self.keys = dev, lay, rule, KEYS[rule]
        self.null = set(null)
        self.idx = {k: lay.index(k) for k in self.keys + "e"}
        self.host0, self.arena = {}, {}
        ks = self.keys + ("e" if e_host is not None else "")
        for k in ks:
            a = np.full(lay.size, SENTINEL, dtype=F)
            a[self.idx[k]] = e_host if k == "e" else host[k]
            if k == "e":                               # a NULL shadow has no storage: sentinels where its slot would be
                for i in self.null:
                    a[lay.first("e", i):lay.first("e", i) + lay.ns[i]] = SENTINEL
            self.host0[k] = a
            self.arena[k] = torch.from_numpy(a).to(dev)
            assert self.arena[k].data_ptr() % 16 == 0
        nseg = len(lay.ns)
        st = np.full(nseg + 2 * BAND, SENTINEL, dtype=F)
        st[BAND:BAND + nseg] = [OR.T_BEFORE[i % 6] for i in range(nseg)]
        self.steps0 = st
        self.steps = torch.from_numpy(st).to(dev)
        seg = np.zeros(nseg, dtype=_SEG_DT)
        for i, n in enumerate(lay.ns):
            for k in self.keys:
                seg[k][i] = self.arena[k].data_ptr() + 4 * lay.first(k, i)
            if rule in ("adam", "adamax"):
                seg["step"][i] = self.steps.data_ptr() + 4 * (BAND + i)
            seg["n"][i], seg["lr"][i], seg["wd"][i] = n, OR.LRS[i % 3], OR.WDS[(i // 3) % 2]
        self.seg_np = seg
        cs, cstart = OR.chunk_table(lay.ns)
        ch = np.zeros(len(cs), dtype=_CHUNK_DT)
        ch["seg"], ch["start"] = cs, cstart
        self.nseg, self.nchunk = nseg, len(ch)
        self.seg_t = torch.from_numpy(seg.view(np.uint8)).to(dev)
        self.chunk_t = torch.from_numpy(ch.view(np.uint8)).to(dev)
        self.partial = torch.full((self.nchunk + 2 * BAND,), SENTINEL, device=dev)
        self.nc = torch.full((2 + 2 * BAND,), SENTINEL, device=dev)
        self.nc[BAND:BAND + 2] = 0
        self.ptrs = self.state = None
        if e_host is not None:
            ptr = np.array([0 if i in self.null else self.arena["e"].data_ptr() + 4 * lay.first("e", i) for i in range(nseg)], dtype=np.int64)
            for i, f in enumerate(lay.forms):
                assert i in self.null or (ptr[i] % 16 == 0) == (f[1] == 0)
                assert (int(seg["p"][i]) % 16 == 0) == (f[0] == 0)
            self.ptrs = torch.from_numpy(ptr).to(dev)
            self.state = torch.full((2 + 2 * BAND,), SENTINEL, device=dev)

    def set_state(self, n, d_eff=-5.0):
        self.state[BAND:BAND + 2] = torch.tensor([float(n), d_eff], device=self.dev)

    def args(self, max_norm, inv, write_grad, skip, decay=None, warmup=0):
        from cvc import hip
        rule_args = {"adam": (BETAS[0], BETAS[1], EPS), "adamax": (BETAS[0], BETAS[1], EPS), "sgd": (MOM,), "sgd0": (MOM,)}[self.rule]
        a = [self.seg_t.data_ptr(), self.nseg, self.chunk_t.data_ptr(), self.nchunk, float(max_norm), float(inv), *rule_args, write_grad,
             self.partial[BAND:].data_ptr(), self.nc[BAND:].data_ptr(), skip.data_ptr() if skip is not None else None]
        if decay is not None:
            a += [self.ptrs.data_ptr(), self.state[BAND:].data_ptr(), float(decay), int(warmup)]
        return a + [hip._stream()]

    def entry(self, L, ema):
        return getattr(L, {"adam": "cvc_adam_clip_step", "adamax": "cvc_adamax_clip_step", "sgd": "cvc_sgd_clip_step",
                           "sgd0": "cvc_sgd_clip_step"}[self.rule] + ("_ema" if ema else ""))

    def read(self):
        out = {k: self.arena[k].cpu().numpy() for k in self.arena}
        out["steps"], out["nc"], out["partial"] = self.steps.cpu().numpy(), self.nc.cpu().numpy(), self.partial.cpu().numpy()
        if self.state is not None:
            out["state"] = self.state.cpu().numpy()
        return out

    def check_sentinels(self, got):
        for k in self.arena:
            used = np.zeros(self.lay.size, dtype=bool)
            used[self.idx[k]] = True
            if k == "e":
                for i in self.null:
                    used[self.lay.first("e", i):self.lay.first("e", i) + self.lay.ns[i]] = False
            assert (got[k][~used] == SENTINEL).all(), "the %s arena was written outside its segments" % k
        for name, n in (("steps", self.nseg), ("partial", self.nchunk), ("nc", 2)) + ((("state", 2),) if self.state is not None else ()):
            a = got[name]
            assert (a[:BAND] == SENTINEL).all() and (a[BAND + n:] == SENTINEL).all(), "%s: a sentinel band was written" % name
        if self.rule in ("sgd", "sgd0"):
            assert same_bits(got["steps"], self.steps0)


def big_layout():
    pairs = [(n, f) for n in SIZES for f in FORMS]
    return Layout([n for n, _ in pairs], [f for _, f in pairs])


def run_pair(dev, L, rule, lay, write_grad, decay=0.9, warmup=0, n_before=3, null=(), skip=None, max_norm=5.0, inv=0.5, seed=1):
    """the plain entry on one set of arenas, the _ema entry on another, from the same operands; the shadows are seeded from the plain
    run's p_new -> (plain side, ema side, plain result, ema result, e before, `same` mask)"""
    host = seeded(lay.total, rule, seed)
    a = Side(dev, lay, rule, host)
    assert a.entry(L, False)(*a.args(max_norm, inv, write_grad, skip)) == 0
    torch.cuda.synchronize()
    ra = a.read()
    p_new = ra["p"][a.idx["p"]]
    e0, same = ER.shadow_values(p_new, host["p"], seed + 100)
    b = Side(dev, lay, rule, host, e_host=e0, null=null)
    b.set_state(n_before)
    assert b.entry(L, True)(*b.args(max_norm, inv, write_grad, skip, decay, warmup)) == 0
    torch.cuda.synchronize()
    rb = b.read()
    a.check_sentinels(ra)
    b.check_sentinels(rb)
    return a, b, ra, rb, e0, same


def assert_plain_bits(a, b, ra, rb, what):
    for k in a.keys:
        assert same_bits(ra[k], rb[k]), "%s: %s differs from the plain entry" % (what, k)
    for k in ("steps", "nc", "partial"):
        assert same_bits(ra[k], rb[k]), "%s: %s differs from the plain entry" % (what, k)


# ------------------------------------------------------------------------------------------------ one step, every size x form
@pytest.mark.parametrize("write_grad", [0, 1, 2])
@pytest.mark.parametrize("rule", RULES)
def test_one_step_plain_bits_and_the_average_inside_its_bound(dev, L, rule, write_grad):
    lay = big_layout()
    a, b, ra, rb, e0, same = run_pair(dev, L, rule, lay, write_grad)
    what = "%s write_grad %d" % (rule, write_grad)
    assert_plain_bits(a, b, ra, rb, what)
    host_g = seeded(lay.total, rule, 1)["g"]
    g = rb["g"][b.idx["g"]]
    assert (not bits(g).any()) if write_grad == 2 else (same_bits(g, host_g) if write_grad == 0 else not same_bits(g, host_g))
    assert not same_bits(rb["p"][b.idx["p"]], seeded(lay.total, rule, 1)["p"])
    n1, d_eff = rb["state"][BAND], rb["state"][BAND + 1]
    assert n1 == 4 and d_eff == F(0.9)
    ER.check_shadow(rb["e"][b.idx["e"]], rb["p"][b.idx["p"]], e0, d_eff, what, same=same)
    assert same.sum() > lay.total // 4
    moving = bits(rb["p"][b.idx["p"]]) != bits(e0)              # (lr == 0 segments: a trailing shadow IS the parameter)
    assert (bits(rb["e"][b.idx["e"]])[moving] != bits(e0)[moving]).mean() > 0.9        # ... and the others were averaged


@pytest.mark.parametrize("rule", RULES)
def test_a_null_shadow_leaves_the_segment_to_the_plain_step(dev, L, rule):
    lay = big_layout()
    null = set(range(0, len(lay.ns), 3))
    a, b, ra, rb, e0, same = run_pair(dev, L, rule, lay, 1, null=null)
    assert_plain_bits(a, b, ra, rb, rule + " null shadows")
    keep = np.concatenate([np.arange(lay.off[i], lay.off[i + 1]) for i in range(len(lay.ns)) if i not in null])
    ER.check_shadow(rb["e"][b.idx["e"]][keep], rb["p"][b.idx["p"]][keep], e0[keep], rb["state"][BAND + 1], rule + " null shadows")
    # (check_sentinels has seen the e arena untouched where the NULL segments' slots would be)


@pytest.mark.parametrize("write_grad", [0, 1, 2])
@pytest.mark.parametrize("rule", RULES)
def test_a_void_step_leaves_the_average_and_its_state(dev, L, rule, write_grad):
    lay = Layout([1, 5, 1025, CHUNK + 1] * 2, [(0, 0)] * 4 + [(1, 3)] * 4)
    skip = torch.tensor([1], dtype=torch.int32, device=dev)
    a, b, ra, rb, e0, _same = run_pair(dev, L, rule, lay, write_grad, skip=skip, warmup=1)
    assert_plain_bits(a, b, ra, rb, rule + " void")
    host = seeded(lay.total, rule, 1)
    for k in b.keys:
        if k != "g":
            assert same_bits(rb[k][b.idx[k]], host[k]), k
    assert same_bits(rb["steps"], b.steps0)
    assert same_bits(rb["e"][b.idx["e"]], e0)
    assert same_bits(rb["state"][BAND:BAND + 2], np.array([3.0, -5.0], dtype=F))
    g = rb["g"][b.idx["g"]]
    assert (not bits(g).any()) if write_grad == 2 else same_bits(g, host["g"])
    assert not rb["nc"][BAND:BAND + 2].any()


@pytest.mark.parametrize("warmup", [0, 1])
@pytest.mark.parametrize("rule", ["adam", "sgd"])
def test_three_steps_of_the_decay_state(dev, L, rule, warmup):
    """ema_state after every one of three steps from n = 0: the count, d_eff against its fp64 statement (one correctly rounded
    division: within u d_eff), e inside the bound of every step under that step's d_eff; d = 0.9999, so the warm-up decides"""
    lay = Layout([5, 1025, CHUNK + 1], [(0, 0), (0, 1), (1, 0)])
    host = seeded(lay.total, rule, 7)
    e0 = (host["p"] + F(0.25)).astype(F)
    b = Side(dev, lay, rule, host, e_host=e0)
    b.set_state(0)
    e = e0
    for it in range(3):
        assert b.entry(L, True)(*b.args(5.0, 1.0, 1, None, 0.9999, warmup)) == 0
        torch.cuda.synchronize()
        r = b.read()
        b.check_sentinels(r)
        n1, d_eff = r["state"][BAND], r["state"][BAND + 1]
        want = ER.d_eff_fp64(0.9999, it, bool(warmup))
        print("%s warmup %d step %d: n %g d_eff %.9g (fp64 %.12g)" % (rule, warmup, it + 1, n1, d_eff, want))
        assert n1 == it + 1 and abs(float(d_eff) - want) <= U * want
        assert (want == (1.0 + it) / (10.0 + it)) if warmup else (d_eff == F(0.9999))
        ER.check_shadow(r["e"][b.idx["e"]], r["p"][b.idx["p"]], e, d_eff, "%s warmup %d step %d" % (rule, warmup, it + 1))
        e = r["e"][b.idx["e"]]
        b.arena["g"].copy_(torch.from_numpy(b.host0["g"]))           # (fresh gradients: the clip rescaled the written ones)


@pytest.mark.parametrize("rule", RULES)
def test_alignment_forms_give_the_same_bits(dev, L, rule):
    """the same values through the float4 form (everything aligned, tails of < 4 elements in the scalar loop) and the scalar form
    (e alone off by one; p and e off): with the clip off (the norm's summation order differs) p, the state and e are bit-identical"""
    outs = []
    for form in ((0, 0), (0, 1), (3, 2)):
        lay = Layout(SIZES, [form] * len(SIZES))
        host = seeded(lay.total, rule, 5)
        e0, _same = ER.shadow_values((host["p"] * np.float32(0.99)).astype(F), host["p"], 6)
        b = Side(dev, lay, rule, host, e_host=e0)
        b.set_state(1)
        assert b.entry(L, True)(*b.args(0.0, 0.5, 1, None, 0.9, 1)) == 0
        torch.cuda.synchronize()
        r = b.read()
        b.check_sentinels(r)
        outs.append({k: r[k][b.idx[k]] for k in b.keys + "e"})
        assert r["nc"][BAND + 1] == F(0.5)
    for o in outs[1:]:
        for k in o:
            assert same_bits(o[k], outs[0][k]), k
    assert not same_bits(outs[0]["e"], e0)


# ------------------------------------------------------------------------------------------------ the exchange
def test_the_swap_exchanges_bits_and_twice_is_the_identity(dev, L):
    from cvc import hip
    lay = big_layout()
    host = seeded(lay.total, "sgd0", 3)
    rng = np.random.default_rng(4)
    e0 = rng.standard_normal(lay.total).astype(F)
    e0[::7] = np.nan                                   # a copy: NaN payloads, signed zeros and denormals travel as they are
    e0[1::7] = -0.0
    e0[2::7] = F(1e-42)
    null = {5, 40}
    b = Side(dev, lay, "sgd0", host, e_host=e0, null=null)
    live = np.concatenate([np.arange(lay.off[i], lay.off[i + 1]) for i in range(len(lay.ns)) if i not in null])
    dead = np.concatenate([np.arange(lay.off[i], lay.off[i + 1]) for i in sorted(null)])
    call = lambda: L.cvc_ema_swap(b.seg_t.data_ptr(), b.nseg, b.chunk_t.data_ptr(), b.nchunk, b.ptrs.data_ptr(), hip._stream())
    assert call() == 0
    torch.cuda.synchronize()
    r = b.read()
    b.check_sentinels(r)
    assert same_bits(r["p"][b.idx["p"]][live], e0[live]) and same_bits(r["e"][b.idx["e"]][live], host["p"][live])
    assert same_bits(r["p"][b.idx["p"]][dead], host["p"][dead])
    assert same_bits(r["g"], b.host0["g"])
    assert call() == 0
    torch.cuda.synchronize()
    r = b.read()
    b.check_sentinels(r)
    assert same_bits(r["p"], b.host0["p"]) and same_bits(r["e"], b.host0["e"])
    for over in (dict(segs=None), dict(chunks=None), dict(ema=None), dict(nseg=0), dict(nchunk=0), dict(nchunk=-1)):
        good = dict(segs=b.seg_t.data_ptr(), nseg=b.nseg, chunks=b.chunk_t.data_ptr(), nchunk=b.nchunk, ema=b.ptrs.data_ptr(), stream=hip._stream())
        assert L.cvc_ema_swap(*dict(good, **over).values()) == BADARG, over
    torch.cuda.synchronize()
    r = b.read()
    assert same_bits(r["p"], b.host0["p"]) and same_bits(r["e"], b.host0["e"])


# ------------------------------------------------------------------------------------------------ argument checks
@pytest.mark.parametrize("rule", ["adam", "sgd", "adamax"])
def test_bad_arguments_are_refused_before_any_launch(dev, L, rule):
    lay = Layout([5, 1025], [(0, 0), (0, 1)])
    host = seeded(lay.total, rule, 9)
    b = Side(dev, lay, rule, host, e_host=host["p"][::-1].copy())
    b.set_state(2)
    good = b.args(1.0, 1.0, 1, None, 0.9, 1)
    names = ["segs", "nseg", "chunks", "nchunk", "max_norm", "inv_world"] + {"sgd": ["momentum"]}.get(rule, ["beta1", "beta2", "eps"]) + \
        ["write_grad", "partial", "norm_coef", "skip", "ema", "ema_state", "decay", "warmup", "stream"]
    assert len(names) == len(good)
    good = dict(zip(names, good))
    overs = [dict(decay=1.0), dict(decay=-0.1), dict(decay=1.5), dict(decay=float("nan")), dict(decay=float("inf")), dict(ema=None),
             dict(ema_state=None), dict(segs=None), dict(chunks=None), dict(partial=None), dict(norm_coef=None), dict(nseg=0),
             dict(nchunk=0), dict(inv_world=0.0)]
    overs += [dict(momentum=1.0), dict(momentum=-0.1)] if rule == "sgd" else [dict(beta1=1.0), dict(beta2=-0.5), dict(eps=-1e-8)]
    if rule == "adamax":
        overs.append(dict(eps=0.0))
    fn = b.entry(L, True)
    for over in overs:
        assert fn(*dict(good, **over).values()) == BADARG, over
    torch.cuda.synchronize()
    r = b.read()
    for k in b.arena:
        assert same_bits(r[k], b.host0[k]), k
    assert same_bits(r["steps"], b.steps0) and not r["nc"][BAND:BAND + 2].any() and (r["partial"] == SENTINEL).all()
    assert same_bits(r["state"][BAND:BAND + 2], np.array([2.0, -5.0], dtype=F))
    assert fn(*good.values()) == 0                     # the same arguments, all good: the step runs, decay 0 included
    assert fn(*dict(good, decay=0.0).values()) == 0
    torch.cuda.synchronize()
    r = b.read()
    b.check_sentinels(r)
    assert r["state"][BAND] == 4 and r["state"][BAND + 1] == 0
