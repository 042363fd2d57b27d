"""The SGD-with-momentum and Adamax steps on the GPU (csrc/optim.hip: optim_sgd_kernel behind cvc_sgd_clip_step, optim_adamax_kernel
behind cvc_adamax_clip_step, with the norm and finalize launches they share with Adam), driven by cvc.optim.ClipSGD / ClipAdamax,
element-wise against the fp64 references and the bounds of tests/optim_rules_ref.py (proven against torch.optim.SGD / Adamax on the
CPU in tests/test_optim_rules_ref_cpu.py, which also shows that the bounds notice a wrong kernel).

The method is tests/test_gpu_optim_kernels.py's: every table is ONE step from known operands; p, g, the rule's state arrays and the
step counts live in arenas with a band of 64 sentinel floats on both sides and sentinel gaps between the segments, and so do the
kernels' scratch (`partial`, `norm_coef`); the state is misaligned by presetting opt.state[p] with views; the optimizer lays out
every table itself.  The reference is fed the device's own coefficient (norm_coef[1]); the norm and the coefficient are checked
through optim_ref.check_norm / check_coef.  Every comparison prints its max ratio |err| / (K x bound) (run with -s).

Measured on an MI355X, the worst over the 58 tables of optim_rules_ref.ALL_TABLES (K = 4; 1 = at the bound):
  SGD      p 0.25    momentum_buffer 0.24    written gradient 1.0 of its single rounding
  Adamax   p 0.25    exp_avg 0.24            exp_inf 0.25             written gradient 1.0 of its single rounding
  norm     0.10 of the bound of its summation structure
i.e. both kernels sit at their float32 restatement's own distance from fp64 (1.0 of the bound without K).  The whole file takes 8 s.
test_six_steps_equal_clip_grad_norm_plus_the_torch_optimizer is what holds SGD's buffer to torch's rounding (the product first, then
the sum): see its docstring."""
import functools

import numpy as np
import pytest
import torch

import optim_ref as OR
import optim_rules_ref as RR
from optim_ref import BAND, CHUNK, SENTINEL

pytestmark = pytest.mark.gpu

BADARG = -1
STATE = {"sgd": {"m": "momentum_buffer"}, "adamax": {"m": "exp_avg", "v": "exp_inf"}}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a visible MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def L(dev):
    from cvc import hip
    return hip.lib()


@functools.lru_cache(maxsize=None)
def values(name):
    return RR.values(RR.TABLES[name])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def keys_of(table):
    """the operands the table's rule has"""
    return "pgmv" if table.rule == "adamax" else ("pgm" if table.mom != 0 else "pg")


def make_opt(table, groups):
    from cvc.optim import ClipAdamax, ClipSGD
    if table.rule == "sgd":
        return ClipSGD(groups, lr=1e-3, momentum=table.mom)
    return ClipAdamax(groups, betas=table.betas, eps=OR.EPS)


# ------------------------------------------------------------------------------------------------ snapshots of an optimizer's tensors
class Snap:
    """p, g and the state arrays of every parameter that has a gradient, flat and side by side on the host (an array the rule does
    not have, or a state not yet there: zeros); the step counts (SGD: zeros); the segment sizes"""

    def __init__(self, opt, params, rule):
        self.act = [i for i, q in enumerate(params) if q.grad is not None]
        dev = params[0].device
        ps = [params[i] for i in self.act]
        sts = [opt.state[q] for q in ps]

        def cat(ts):
            return torch.cat([t.detach().reshape(-1) for t in ts]).cpu().numpy()

        def state(k):
            name = STATE[rule].get(k)
            return cat([st[name] if name in st and st[name] is not None else torch.zeros_like(q) for q, st in zip(ps, sts)])
        self.p, self.g, self.m, self.v = cat(ps), cat([q.grad for q in ps]), state("m"), state("v")
        self.steps = torch.stack([st["step"].detach().to(dev, torch.float32).reshape(()) if "step" in st else torch.zeros((), device=dev)
                                  for st in sts]).cpu().numpy()
        self.ns = np.array([q.numel() for q in ps], dtype=np.int64)
        self.off = np.concatenate(([0], np.cumsum(self.ns)))

    def seg(self, key, j):
        return getattr(self, key)[self.off[j]:self.off[j + 1]]


def reference(opt, rule, pre, coef):
    groups = [opt.param_groups[i] for i in pre.act]
    lr = np.repeat(np.array([g["lr"] for g in groups], dtype=np.float32), pre.ns)
    wd = np.repeat(np.array([g["weight_decay"] for g in groups], dtype=np.float32), pre.ns)
    g0 = opt.param_groups[0]
    if rule == "sgd":
        return lr, RR.sgd_step_fp64(pre.p, pre.g, pre.m, lr, wd, g0["momentum"], coef)
    return lr, RR.adamax_step_fp64(pre.p, pre.g, pre.m, pre.v, np.repeat(pre.steps, pre.ns), lr, wd, g0["betas"][0], g0["betas"][1],
                                   g0["eps"], coef)


def verify(opt, rule, pre, post, coef, what, written="clipped", k=None):
    """one step from `pre` to `post` against the rule's fp64 step under the device's coefficient: p and the state inside K x their
    bounds, the gradient as `written` ("clipped": g coef within its one rounding; "zero"; "untouched": the same bits), Adamax's step
    counts + 1, lr == 0 leaves p's bits alone.  lr and weight decay are the param groups' (one parameter per group) at the call."""
    assert pre.act == post.act
    lr, ref = reference(opt, rule, pre, coef)
    has_m = rule == "adamax" or opt.param_groups[0]["momentum"] != 0
    r = OR.check_elements(post.p, post.m if has_m else None, post.v if rule == "adamax" else None,
                          post.g if written == "clipped" else None, ref, what, RR.K[rule] if k is None else k)
    if written == "zero":
        assert not bits(post.g).any(), what
    elif written == "untouched":
        assert same_bits(post.g, pre.g), what
    assert np.array_equal(post.steps, pre.steps + 1 if rule == "adamax" else pre.steps), what
    still = (lr == 0) & np.isfinite(ref.p)
    assert same_bits(post.p[still], pre.p[still]), what + ": lr == 0 moved a parameter"
    moved = still & (pre.g != 0)
    if has_m and moved.any() and np.isfinite(coef) and coef != 0:
        assert (bits(post.m[moved]) != bits(pre.m[moved])).any(), what          # ... but not its state
    return r


# ------------------------------------------------------------------------------------------------ one table in sentinel-banded arenas
class Rig:
    """A ClipSGD / ClipAdamax over one table of tests/optim_rules_ref.py.  vals: other operands than the table's seeded ones;
    no_grad: segments whose parameter gets no gradient (and no preset state)."""

    def __init__(self, dev, table, vals=None, no_grad=()):
        self.table, self.dev, self.rule = table, dev, table.rule
        self.keys = keys_of(table)
        vals = values(table.name) if vals is None else vals
        segs = table.segs
        starts, size = OR.layout(segs)
        col = {"p": 0, "g": 1, "m": 2, "v": 3}
        self.idx = {k: np.concatenate([np.arange(a + s.offs[col[k]], a + s.offs[col[k]] + s.n) for s, a in zip(segs, starts)]) for k in self.keys}
        self.used, host = {}, {}
        live = np.repeat(np.array([i not in no_grad for i in range(len(segs))]), [s.n for s in segs])
        for k in self.keys:
            host[k] = np.full(size, SENTINEL, dtype=np.float32)
            at = self.idx[k] if k == "p" else self.idx[k][live]
            host[k][at] = getattr(vals, k) if k == "p" else getattr(vals, k)[live]
            self.used[k] = np.zeros(size, dtype=bool)
            self.used[k][at] = True
        self.arena = {k: torch.from_numpy(host[k]).to(dev) for k in self.keys}
        assert all(a.data_ptr() % 16 == 0 for a in self.arena.values())
        nseg = len(segs)
        st = np.full(nseg + 2 * BAND, SENTINEL, dtype=np.float32)
        st[BAND:BAND + nseg] = [s.t for s in segs]
        self.steps = torch.from_numpy(st).to(dev)
        self.params, groups = [], []
        for i, (s, a) in enumerate(zip(segs, starts)):
            q = torch.nn.Parameter(self.arena["p"][a + s.offs[0]:a + s.offs[0] + s.n])
            if i not in no_grad:
                q.grad = self.arena["g"][a + s.offs[1]:a + s.offs[1] + s.n]
            self.params.append(q)
            groups.append({"params": [q], "lr": s.lr, "weight_decay": s.wd})
        self.opt = make_opt(table, groups)
        for i, (s, a, q) in enumerate(zip(segs, starts, self.params)):
            if i in no_grad:
                continue
            state = {STATE[self.rule][k]: self.arena[k][a + s.offs[col[k]]:a + s.offs[col[k]] + s.n] for k in self.keys[2:]}
            if self.rule == "adamax":
                state["step"] = self.steps[BAND + i]
            if state:
                self.opt.state[q] = state
            for k, t in [("p", q), ("g", q.grad)] + [(k, state[STATE[self.rule][k]]) for k in self.keys[2:]]:
                assert (t.data_ptr() % 16 == 0) == (s.offs[col[k]] == 0), (i, k)
        self.partial = self.nc = None

    def own_scratch(self):
        """`partial` and `norm_coef` of the table the optimizer built, moved between sentinel bands (the key, hence the table, stays)"""
        t = self.opt._build_table()
        if self.partial is None or t[3].data_ptr() != self.partial[BAND:].data_ptr():
            self.nchunk = t[6]
            self.partial = torch.full((self.nchunk + 2 * BAND,), SENTINEL, device=self.dev)
            self.nc = torch.full((2 + 2 * BAND,), SENTINEL, device=self.dev)
            self.nc[BAND:BAND + 2] = 0
            self.opt._table = t[:3] + (self.partial[BAND:BAND + self.nchunk], self.nc[BAND:BAND + 2]) + t[5:]
        return self.opt._table

    def snap(self):
        return Snap(self.opt, self.params, self.rule)

    def step(self, max_norm=None, inv=None, plain=False, **kw):
        """one clip_and_step (plain: opt.step()) -> (pre, post, norm, coef), the last two as the device left them in norm_coef"""
        self.own_scratch()
        pre = self.snap()
        if plain:
            self.opt.step()
        else:
            ret = self.opt.clip_and_step(self.table.max_norm if max_norm is None else max_norm, self.table.inv if inv is None else inv, **kw)
            assert ret.data_ptr() == self.nc[BAND:].data_ptr()
        torch.cuda.synchronize()
        post = self.snap()
        nc = self.nc.cpu().numpy()
        self.bands_intact()
        return pre, post, nc[BAND], nc[BAND + 1]

    def bands_intact(self):
        for k in self.keys:
            a = self.arena[k].cpu().numpy()
            assert (a[~self.used[k]] == SENTINEL).all(), "the %s arena was written outside its segments" % k
        for name, t, n in (("steps", self.steps, len(self.table.segs)), ("partial", self.partial, self.nchunk), ("norm_coef", self.nc, 2)):
            a = t.cpu().numpy()
            assert (a[:BAND] == SENTINEL).all() and (a[BAND + n:] == SENTINEL).all(), "%s: a sentinel band was written" % name
        if self.rule == "sgd":              # (SGD keeps no step count: nothing between the bands moves either)
            assert np.array_equal(self.steps.cpu().numpy()[BAND:BAND + len(self.table.segs)], [s.t for s in self.table.segs])

    def grads(self, pre):
        return [pre.seg("g", j) for j in range(len(pre.ns))]


def with_values(table, **over):
    v = values(table.name)
    return v._replace(**{k: (f(getattr(v, k)) if callable(f) else f).astype(np.float32) for k, f in over.items()})


BIG = {"sgd": "sgd-multi-chunk-m+3", "adamax": "adamax-multi-chunk-v+1", "sgd0": "sgd-mom0-multi-chunk-g+2"}
RULES3 = ["sgd", "sgd0", "adamax"]           # sgd0: the buffer-less form


def big(which):
    return RR.TABLES[BIG[which]]


# ------------------------------------------------------------------------------------------------ one step, element-wise
@pytest.mark.parametrize("name", [t.name for t in RR.ALL_TABLES])
def test_one_step_elementwise_against_fp64(dev, name):
    """p, the state and the written gradient inside their bounds under the device's coefficient; the norm inside the bound of its
    summation structure; the coefficient from the device's norm within 4 u (inv exactly when the clip is off or not reached);
    Adamax's step counts + 1; lr == 0 leaves p alone; all sentinels intact"""
    table = RR.TABLES[name]
    rig = Rig(dev, table)
    pre, post, norm, coef = rig.step()
    verify(rig.opt, table.rule, pre, post, coef, name)
    OR.check_norm(norm, rig.grads(pre), table.inv, pre.ns, rig.nchunk, name)
    OR.check_coef(norm, coef, table.max_norm, table.inv, name)
    if table.max_norm == 1e9:
        assert coef == np.float32(table.inv)
    assert float(rig.opt.last_norm) == norm


def test_the_segment_tables_leave_out_what_a_rule_does_not_have(dev, L):
    from cvc.optim import _SEG_DT
    for which, null in (("sgd", ("v", "step")), ("sgd0", ("m", "v", "step")), ("adamax", ())):
        rig = Rig(dev, big(which))
        segs = rig.own_scratch()[1].cpu().numpy().view(_SEG_DT)
        for k in ("p", "g", "m", "v", "step"):
            assert (segs[k] == 0).all() if k in null else (segs[k] != 0).all(), (which, k)
        assert np.array_equal(segs["n"], [s.n for s in rig.table.segs])


# ------------------------------------------------------------------------------------------------ exact checks
@pytest.mark.parametrize("which", RULES3)
def test_alignment_forms_compute_the_same_bits(dev, which):
    """the same values through the float4 form (every operand aligned) and the scalar form (every operand one element off): with
    the clip off p, the state and the written gradient are bit-identical"""
    base = big(which)
    ns = OR.SMALL_N + (CHUNK + 4, 2 * CHUNK + 3)
    a = base._replace(name="forms-aligned-" + which, segs=[OR.Seg(n, OR.ALIGNED, *RR._cycle(i)) for i, n in enumerate(ns)], max_norm=0.0, inv=0.5)
    b = a._replace(segs=[s._replace(offs=(1, 1, 1, 1)) for s in a.segs])
    vals = RR.values(a)
    (_pa, post_a, norm_a, coef_a), (_pb, post_b, norm_b, coef_b) = Rig(dev, a, vals).step(), Rig(dev, b, vals).step()
    assert coef_a == coef_b == np.float32(0.5)
    assert all(same_bits(getattr(post_a, k), getattr(post_b, k)) for k in "pgmv")
    assert np.array_equal(post_a.steps, post_b.steps)
    assert abs(float(norm_a) - float(norm_b)) <= 2 * OR.norm_rel_bound(ns, 6) * float(norm_a)       # two summation orders


@pytest.mark.parametrize("which", RULES3)
def test_every_element_is_updated_exactly_once(dev, which):
    """clip off, inv 0.5, a fresh state, no weight decay: the written gradient is 0.5 g bitwise and SGD's buffer is that value --
    an element updated twice would hold 0.25 g and another buffer, one left out g and 0; Adamax's exp_inf is |0.5 g| + eps rounded"""
    base = big(which)
    table = base._replace(segs=[s._replace(t=0, wd=0.0) for s in base.segs])
    rig = Rig(dev, table, with_values(base, m=np.zeros_like, v=np.zeros_like))
    pre, post, _norm, coef = rig.step(max_norm=0.0, inv=0.5)
    assert coef == np.float32(0.5)
    half = np.float32(0.5) * pre.g
    assert same_bits(post.g, half)
    if which == "sgd":
        assert np.array_equal(post.m, half)                                # (mom x 0 + -0 is +0: values, not bits)
    if which == "adamax":
        assert same_bits(post.v, np.abs(half) + np.float32(OR.EPS)) and (post.steps == 1).all()
    verify(rig.opt, table.rule, pre, post, coef, which + " fresh")


@pytest.mark.parametrize("which", RULES3)
def test_write_grad_modes_and_determinism(dev, which):
    """write_grad=False leaves g's bits, zero_grad=True leaves zeros, and p and the state do not depend on it; two runs from the
    same inputs give the same bits everywhere, the norm under an active clip included"""
    table = big(which)
    runs = {}
    for mode, kw in (("clipped", {}), ("again", {}), ("untouched", dict(write_grad=False)), ("zero", dict(zero_grad=True)),
                     ("zero-over-write", dict(write_grad=False, zero_grad=True))):
        runs[mode] = Rig(dev, table).step(**kw)
    pre, post, norm, coef = runs["clipped"]
    assert 0 < coef < 1
    verify(Rig(dev, table).opt, table.rule, pre, post, coef, which)
    for mode, (pre2, post2, norm2, coef2) in runs.items():
        assert same_bits(pre2.g, pre.g)
        assert bits(np.array([norm2, coef2])).tolist() == bits(np.array([norm, coef])).tolist(), mode
        assert all(same_bits(getattr(post2, k), getattr(post, k)) for k in "pmv") and np.array_equal(post2.steps, post.steps), mode
    assert same_bits(runs["again"][1].g, post.g) and not same_bits(post.g, pre.g)
    assert same_bits(runs["untouched"][1].g, pre.g)
    assert not bits(runs["zero"][1].g).any() and not bits(runs["zero-over-write"][1].g).any()


def test_step_alone_is_the_unclipped_update(dev):
    for which in RULES3:
        table = big(which)
        (pre1, post1, norm1, coef1), (_pre2, post2, norm2, coef2) = Rig(dev, table).step(plain=True), Rig(dev, table).step(0.0, 1.0, write_grad=False)
        assert coef1 == coef2 == 1 and bits(np.array([norm1])).tolist() == bits(np.array([norm2])).tolist()
        assert all(same_bits(getattr(post1, k), getattr(post2, k)) for k in "pgmv") and same_bits(post1.g, pre1.g)


# ------------------------------------------------------------------------------------------------ the skip word
@pytest.mark.parametrize("which", RULES3)
@pytest.mark.parametrize("mode,kw", [("zero", dict(zero_grad=True)), ("clipped", {}), ("untouched", dict(write_grad=False))])
def test_a_set_skip_word_voids_the_step(dev, which, mode, kw):
    """p, the state and every step count keep their bits, norm_coef is [0, 0]; the gradients are zeroed under zero_grad=True (what
    Trainer asks for) and untouched otherwise.  With the word cleared the same table steps."""
    rig = Rig(dev, big(which))
    skip = torch.tensor([7], dtype=torch.int32, device=dev)
    pre, post, norm, coef = rig.step(skip=skip, **kw)
    assert bits(np.array([norm, coef])).tolist() == [0, 0]
    assert all(same_bits(getattr(post, k), getattr(pre, k)) for k in "pmv") and np.array_equal(post.steps, pre.steps)
    assert (not bits(post.g).any()) if mode == "zero" else same_bits(post.g, pre.g)
    assert int(skip) == 7
    skip.zero_()
    if mode == "zero":                       # (the void step left zero gradients: fresh ones)
        for q in rig.params:
            q.grad.copy_(torch.full_like(q, 0.125))
    pre, post, norm, coef = rig.step(skip=skip, **kw)
    verify(rig.opt, rig.rule, pre, post, coef, "after a void step (%s, %s)" % (which, mode), written=mode)


# ------------------------------------------------------------------------------------------------ NaN gradients
@pytest.mark.parametrize("rule", ["sgd", "adamax"])
@pytest.mark.parametrize("clip", [False, True])
def test_one_nan_gradient_element(dev, rule, clip):
    """unclipped: the NaN stays where it is -- NaN p and state (Adamax: exp_avg AND exp_inf, as torch.maximum hands a NaN on; fmaxf
    would have dropped it) at that element only.  Under a clip the norm, the coefficient and every element are NaN, as in torch."""
    table = RR.TABLES[rule + "-shape-300"]
    v = values(table.name)
    g = v.g.copy()
    at = int(v.off[123]) + 2
    g[at] = np.nan
    rig = Rig(dev, table, v._replace(g=g))
    pre, post, norm, coef = rig.step(max_norm=5.0 if clip else 0.0)
    assert norm != norm
    keys = "pmv" if rule == "adamax" else "pm"
    if clip:
        assert coef != coef and all(np.isnan(getattr(post, k)).all() for k in keys + "g")
    else:
        bad = np.zeros(len(g), dtype=bool)
        bad[at] = True
        assert coef == np.float32(table.inv)
        for k in keys + "g":
            assert np.array_equal(np.isnan(getattr(post, k)), bad), k
    verify(rig.opt, rule, pre, post, coef, "%s nan, clip %s" % (rule, clip))


# ------------------------------------------------------------------------------------------------ the optimizers' behaviour
@pytest.mark.parametrize("rule", ["sgd", "adamax"])
def test_a_parameter_without_gradient_gets_no_state(dev, rule):
    table = RR.TABLES[rule + "-shape-257"]
    dead = (0, 100, 256)
    rig = Rig(dev, table, no_grad=dead)
    before = [rig.params[i].detach().clone() for i in dead]
    pre, post, _norm, coef = rig.step()
    assert len(pre.act) == 257 - 3
    verify(rig.opt, rule, pre, post, coef, "three parameters without gradient")
    for i, b in zip(dead, before):
        assert len(rig.opt.state[rig.params[i]]) == 0 and torch.equal(rig.params[i].detach(), b)


def test_sgd_without_momentum_keeps_no_state(dev):
    rig = Rig(dev, big("sgd0"))
    rig.step()
    assert all(len(rig.opt.state[q]) == 0 for q in rig.params)


def _new_grads(rig, seed):
    rng = np.random.default_rng(seed)
    for q in rig.params:
        if q.grad is not None:
            q.grad.copy_(torch.from_numpy((rng.standard_normal(q.numel()) * 10.0 ** rng.integers(-3, 2)).astype(np.float32)))


@pytest.mark.parametrize("rule", ["sgd", "adamax"])
def test_a_scheduler_rewrites_the_rates_in_place(dev, rule):
    rig = Rig(dev, RR.TABLES[rule + "-shape-300"])
    pre, post, _norm, coef = rig.step()
    verify(rig.opt, rule, pre, post, coef, "before the scheduler")
    t0, ptr = rig.opt._table, rig.opt._table[1].data_ptr()
    for i, g in enumerate(rig.opt.param_groups):
        g["lr"] = g["lr"] * 0.5 if i % 2 else 3e-4
    _new_grads(rig, 1)
    pre, post, _norm, coef = rig.step()
    assert rig.opt._table is t0 and rig.opt._table[1].data_ptr() == ptr and not rig.opt._retired
    assert len({g["lr"] for g in rig.opt.param_groups}) > 2
    verify(rig.opt, rule, pre, post, coef, "new rates")                        # verify() reads the param groups' current rates
    rig.opt.param_groups[5]["weight_decay"] = 0.02
    rig.opt.sync_hyperparameters()
    _new_grads(rig, 2)
    pre, post, _norm, coef = rig.step()
    assert rig.opt._table is t0 and rig.opt._table[1].data_ptr() == ptr
    verify(rig.opt, rule, pre, post, coef, "a new weight decay")


def test_constructors_refuse_what_the_kernels_do_not_do(dev):
    from cvc.optim import ClipAdamax, ClipSGD
    q = torch.nn.Parameter(torch.zeros(4, device=dev))
    for kw in (dict(nesterov=True, momentum=0.9), dict(dampening=0.1, momentum=0.9), dict(maximize=True), dict(differentiable=True)):
        with pytest.raises(ValueError):
            ClipSGD([q], lr=1e-3, **kw)
    for kw in (dict(maximize=True), dict(differentiable=True)):
        with pytest.raises(ValueError):
            ClipAdamax([q], **kw)
    with pytest.raises(TypeError, match="momentun"):
        ClipSGD([q], lr=1e-3, momentun=0.9)                     # a misspelt argument is not dropped
    with pytest.raises(TypeError, match="beta"):
        ClipAdamax([q], beta=(0.9, 0.99))
    r = torch.nn.Parameter(torch.zeros(4, device=dev))
    q.grad, r.grad = torch.ones_like(q), torch.ones_like(r)
    with pytest.raises(ValueError):
        ClipSGD([{"params": [q], "momentum": 0.9}, {"params": [r], "momentum": 0.5}], lr=1e-3).step()
    with pytest.raises(ValueError):
        ClipAdamax([{"params": [q]}, {"params": [r], "betas": (0.8, 0.999)}]).step()
    with pytest.raises(ValueError):
        ClipAdamax([{"params": [q]}, {"params": [r], "eps": 1e-6}]).step()
    for cls in (ClipSGD, ClipAdamax):
        c = torch.nn.Parameter(torch.zeros(4))
        c.grad = torch.ones(4)
        with pytest.raises(RuntimeError, match="contiguous float32 GPU parameters and gradients only"):
            cls([c], lr=1e-3).step()
        h = torch.nn.Parameter(torch.zeros(4, 6, device=dev))
        h.grad = torch.ones(6, 4, device=dev).t()
        with pytest.raises(RuntimeError, match="contiguous float32 GPU parameters and gradients only"):
            cls([h], lr=1e-3).step()
    assert torch.equal(q.detach(), torch.zeros(4, device=dev))


# ------------------------------------------------------------------------------------------------ argument checks
@pytest.mark.parametrize("rule", ["sgd", "adamax"])
def test_bad_arguments_are_refused_before_any_launch(dev, L, rule):
    from cvc import hip
    rig = Rig(dev, RR.TABLES[rule + "-shape-1"])
    t = rig.own_scratch()
    head = dict(segs=t[1].data_ptr(), nseg=t[5], chunks=t[2].data_ptr(), nchunk=t[6], max_norm=1.0, inv_world=1.0)
    tail = dict(write_grad=1, partial=t[3].data_ptr(), norm_coef=t[4].data_ptr(), skip=None, stream=hip._stream())
    common = (dict(segs=None), dict(chunks=None), dict(partial=None), dict(norm_coef=None), dict(nseg=0), dict(nseg=-1), dict(nchunk=0),
              dict(nchunk=-3), dict(inv_world=0.0), dict(inv_world=-1.0))
    if rule == "sgd":
        fn, good = L.cvc_sgd_clip_step, dict(head, momentum=0.9, **tail)
        own = (dict(momentum=1.0), dict(momentum=-0.1), dict(momentum=1.5))
    else:
        fn, good = L.cvc_adamax_clip_step, dict(head, beta1=0.9, beta2=0.999, eps=1e-8, **tail)
        own = (dict(beta1=1.0), dict(beta1=-0.1), dict(beta2=1.0), dict(beta2=-0.5), dict(beta2=1.5), dict(eps=0.0), dict(eps=-1e-8))
    before = rig.snap()
    for over in common + own:
        a = dict(good, **over)
        assert list(a) == list(good) and fn(*a.values()) == BADARG, over
    torch.cuda.synchronize()
    after = rig.snap()
    assert all(same_bits(getattr(after, k), getattr(before, k)) for k in "pgmv") and np.array_equal(after.steps, before.steps)
    assert not rig.nc[BAND:BAND + 2].cpu().numpy().any() and (rig.partial.cpu().numpy() == SENTINEL).all()
    rig.bands_intact()
    assert fn(*good.values()) == 0                     # the same arguments, all good: the step runs
    torch.cuda.synchronize()
    now = rig.snap()
    assert not same_bits(now.p, before.p) and np.array_equal(now.steps, before.steps + (rule == "adamax"))


# ------------------------------------------------------------------------------------------------ against torch on the GPU
def _make(dev, base, big_t, arena, weight_decay, extra):
    ps = [torch.nn.Parameter(b.clone().to(dev)) for b in base]
    ps.append(torch.nn.Parameter(big_t.clone().to(dev)))
    a = arena.clone().to(dev)
    ps.append(torch.nn.Parameter(a[1:]))                       # 4-byte aligned storage offset: the scalar path of the kernels
    dead = torch.nn.Parameter(torch.ones(8, device=dev))       # never receives a gradient
    groups = [dict({"params": [p], "lr": 1e-3 * (0.1 if i % 3 == 0 else 1.0), "weight_decay": weight_decay}, **extra)
              for i, p in enumerate(ps + [dead])]
    return ps, dead, groups


@pytest.mark.parametrize("rule", ["sgd", "adamax"])
@pytest.mark.parametrize("weight_decay,max_norm", [(0.0, 0.5), (0.01, 0.5), (0.0, 1e6)])
def test_six_steps_equal_clip_grad_norm_plus_the_torch_optimizer(dev, rule, weight_decay, max_norm):
    """ClipSGD / ClipAdamax.clip_and_step against nn.utils.clip_grad_norm_ + torch.optim.SGD(momentum=0.9) / torch.optim.Adamax
    over six steps, with the shapes and tolerances of test_clip_adam_equals_clip_grad_norm_plus_torch_adam (tests/test_gpu_train.py):
    rtol 2e-6, atol 1e-6 for parameters and state; per-group learning rates, odd sizes, a parameter that never gets a gradient, a
    4-byte-aligned view.

    The case [sgd, weight_decay 0, max_norm 1e6] (no clip: gradients of scale 3 meet a buffer of scale 10) holds optim_sgd_kernel to
    torch's rounding of the buffer, mom x buf rounded before g is added (buf.mul_(0.9).add_(g)): a fused fma(0.9, buf, g) is 8.4e-7
    (step 4) and 1.12e-6 (step 6) beyond 2e-6 |torch| where 1e-6 is allowed -- at the worst element 0.9 x -9.1534 + 8.1925 = -0.0456
    cancels two hundredfold, and the buffers differ by an ulp of 9.15 from step 4 on.  With torch's rounding the difference is 0."""
    from cvc.optim import ClipAdamax, ClipSGD
    g = torch.Generator().manual_seed(11)
    big_t = torch.randn(3 * 65536 + 7, generator=g)
    base = [torch.randn(*s, generator=g) for s in [(257, 129), (65536 * 2,), (5,), (1,), (64, 1024)]]
    arena = torch.randn(1000 + 1, generator=g)
    extra = {"momentum": 0.9} if rule == "sgd" else {"betas": (0.8, 0.99)}
    names = list(STATE[rule].values())
    pa, dead_a, ga = _make(dev, base, big_t, arena, weight_decay, extra)
    pb, dead_b, gb = _make(dev, base, big_t, arena, weight_decay, extra)
    ref = torch.optim.SGD(ga, lr=1e-3) if rule == "sgd" else torch.optim.Adamax(ga)
    opt = ClipSGD(gb, lr=1e-3) if rule == "sgd" else ClipAdamax(gb)
    worst = dict(p=0.0, **{n: 0.0 for n in names})
    for it in range(6):
        grads = [torch.randn(p.shape, generator=g) * (3.0 if it % 2 else 0.01) for p in pa]
        for p, q, gr in zip(pa, pb, grads):
            p.grad = gr.clone().to(dev)
            q.grad = gr.clone().to(dev)
        n_ref = torch.nn.utils.clip_grad_norm_(pa + [dead_a], max_norm)
        ref.step()
        n_got = opt.clip_and_step(max_norm, 1.0)
        assert float(n_got) == pytest.approx(float(n_ref), rel=2e-6)
        for p, q in zip(pa, pb):
            sa, sb = ref.state[p], opt.state[q]
            worst["p"] = max(worst["p"], float(((q - p).abs() - 2e-6 * p.abs()).max().detach()))
            for n in names:
                worst[n] = max(worst[n], float(((sb[n] - sa[n]).abs() - 2e-6 * sa[n].abs()).max()))
        print("step %d: worst |got - torch| - 2e-6 |torch| so far (allowed 1e-6): %s" % (it + 1, ", ".join("%s %.3g" % kv for kv in worst.items())))
        for p, q in zip(pa, pb):
            assert torch.allclose(q, p, rtol=2e-6, atol=1e-6), it
            assert torch.allclose(q.grad, p.grad, rtol=2e-6, atol=1e-9)                       # the clipped gradient, written back
            sa, sb = ref.state[p], opt.state[q]
            for n in names:
                assert torch.allclose(sb[n], sa[n], rtol=2e-6, atol=1e-6), (it, n)
            if rule == "adamax":
                assert float(sb["step"]) == float(sa["step"]) == it + 1
    assert torch.equal(dead_b, torch.ones(8, device=dev)) and len(opt.state[dead_b]) == 0           # skipped, as torch skips it
    assert set(opt.state_dict()["state"][0].keys()) == set(names) | ({"step"} if rule == "adamax" else set())


# ------------------------------------------------------------------------------------------------ state_dict round trips
def _plain_params(dev, seed, sizes=(5, 1027, 300, CHUNK + 1)):
    rng = np.random.default_rng(seed)
    ps = [torch.nn.Parameter(torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(dev)) for n in sizes]
    groups = [{"params": [q], "lr": (1e-3, 1e-4)[i % 2], "weight_decay": (0.0, 0.01)[i % 2]} for i, q in enumerate(ps)]
    return ps, groups


def _plain_grads(ps, seed):
    rng = np.random.default_rng(seed)
    for q in ps:
        q.grad = torch.from_numpy(rng.standard_normal(q.numel()).astype(np.float32)).to(q.device)


def _copy_params(dst, src):
    with torch.no_grad():
        for q, r in zip(dst, src):
            q.copy_(r)


@pytest.mark.parametrize("rule", ["sgd", "adamax"])
def test_resume_from_the_torch_optimizer_and_back(dev, rule):
    """load_state_dict from torch.optim.SGD / torch.optim.Adamax (capturable=False: its `step` is a CPU tensor) after two of its
    steps, then ONE step of ours: the update is the reference's from the loaded state, Adamax's counts go on on the device.  And
    back: the torch optimizer resumes from our state_dict and steps; its step is torch's arithmetic in torch's order, held to
    2 K x the bounds -- a misread state or count is off by orders of magnitude, not by a rounding."""
    from cvc.optim import ClipAdamax, ClipSGD
    mk_ref = (lambda g, **kw: torch.optim.SGD(g, lr=1e-3, momentum=0.9, foreach=False)) if rule == "sgd" else \
        (lambda g, **kw: torch.optim.Adamax(g, betas=(0.8, 0.99), foreach=False, **kw))
    mk = (lambda g: ClipSGD(g, lr=1e-3, momentum=0.9)) if rule == "sgd" else (lambda g: ClipAdamax(g, betas=(0.8, 0.99)))
    pa, ga = _plain_params(dev, 3)
    ref = mk_ref(ga)
    for it in range(2):
        _plain_grads(pa, 20 + it)
        ref.step()
    if rule == "adamax":
        assert not ref.state[pa[0]]["step"].is_cuda
    pb, gb = _plain_params(dev, 3)
    _copy_params(pb, pa)
    opt = mk(gb)
    opt.load_state_dict(ref.state_dict())
    _plain_grads(pb, 30)
    pre = Snap(opt, pb, rule)
    assert all(same_bits(pre.seg("m", j), ref.state[r][STATE[rule]["m"]].cpu().numpy()) for j, r in enumerate(pa))
    if rule == "adamax":
        assert (pre.steps == 2).all()
    opt.clip_and_step(1.0, 1.0)
    torch.cuda.synchronize()
    post = Snap(opt, pb, rule)
    verify(opt, rule, pre, post, float(opt._table[4][1]), "resumed from the torch optimizer")
    if rule == "adamax":
        assert all(opt.state[q]["step"].is_cuda and float(opt.state[q]["step"]) == 3 for q in pb)
    # ... and back
    pc, gc = _plain_params(dev, 3)
    _copy_params(pc, pb)
    back = mk_ref(gc, capturable=True)
    back.load_state_dict(opt.state_dict())
    _plain_grads(pc, 31)
    pre = Snap(back, pc, rule)
    assert same_bits(pre.m, post.m) and same_bits(pre.v, post.v) and np.array_equal(pre.steps, post.steps)
    back.step()
    torch.cuda.synchronize()
    verify(back, rule, pre, Snap(back, pc, rule), 1.0, "the torch optimizer resumed from ours", written="untouched", k=2 * RR.K[rule])


def test_a_none_momentum_buffer_becomes_a_zero_buffer(dev):
    """a state saved by torch.optim.SGD before its first step of a parameter holds momentum_buffer = None: zeros, whose first step
    (buf = mom 0 + ge) is torch's"""
    from cvc.optim import ClipSGD
    pa, ga = _plain_params(dev, 4)
    pb, gb = _plain_params(dev, 4)
    ref, opt = torch.optim.SGD(ga, lr=1e-3, momentum=0.9, foreach=False), ClipSGD(gb, lr=1e-3, momentum=0.9)
    sd = ref.state_dict()
    sd["state"] = {i: {"momentum_buffer": None} for i in range(len(pa))}
    ref.load_state_dict(sd)
    opt.load_state_dict(sd)
    assert all(opt.state[q]["momentum_buffer"] is None for q in pb)
    _plain_grads(pa, 40)
    _plain_grads(pb, 40)
    ref.step()
    pre = Snap(opt, pb, "sgd")
    assert not pre.m.any()
    opt.step()
    torch.cuda.synchronize()
    post = Snap(opt, pb, "sgd")
    verify(opt, "sgd", pre, post, 1.0, "from a None buffer", written="untouched")
    for p, q in zip(pa, pb):
        assert torch.allclose(q, p, rtol=2e-6, atol=1e-6) and torch.allclose(opt.state[q]["momentum_buffer"], ref.state[p]["momentum_buffer"], rtol=2e-6, atol=1e-6)


# ------------------------------------------------------------------------------------------------ captured
@pytest.mark.parametrize("rule", ["sgd", "adamax"])
def test_a_captured_clip_and_step_replays_bit_equal_to_eager_calls(dev, rule):
    """one clip_and_step captured into a graph (three launches on one stream: no parallel branches) and replayed three times equals
    three eager calls bit for bit: parameters, state, step counts, the gradients the clip rescales every time, the norm"""
    from cvc.optim import ClipAdamax, ClipSGD
    mk = (lambda g: ClipSGD(g, lr=1e-3, momentum=0.9)) if rule == "sgd" else (lambda g: ClipAdamax(g, betas=(0.8, 0.99)))
    runs = []
    warm, warm_groups = _plain_params(dev, 7, sizes=(9,))      # (the library's kernels are loaded before anything is captured)
    _plain_grads(warm, 51)
    mk(warm_groups).clip_and_step(0.5, 1.0)
    for graphed in (False, True):
        ps, groups = _plain_params(dev, 6)
        _plain_grads(ps, 50)
        opt = mk(groups)
        if graphed:
            opt._build_table()                       # state and tables exist before the capture; nothing is launched
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                opt.clip_and_step(0.5, 1.0)
            before = Snap(opt, ps, rule)
            assert not before.m.any() and not before.steps.any()          # the capture ran nothing
            for _ in range(3):
                graph.replay()
        else:
            for _ in range(3):
                opt.clip_and_step(0.5, 1.0)
        torch.cuda.synchronize()
        runs.append((Snap(opt, ps, rule), float(opt.last_norm)))
    (a, na), (b, nb) = runs
    assert all(same_bits(getattr(a, k), getattr(b, k)) for k in "pgmv") and np.array_equal(a.steps, b.steps) and na == nb
    assert a.m.any() and (rule == "sgd" or (a.steps == 3).all())
