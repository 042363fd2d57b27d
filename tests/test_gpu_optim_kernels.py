"""The optimizer step's kernels on the GPU (csrc/optim.hip: optim_sumsq_kernel, optim_finalize_kernel, optim_adam_kernel behind
cvc_adam_clip_step), driven by cvc.optim.ClipAdam, element-wise against the fp64 reference and the bounds of tests/optim_ref.py
(proven against torch.optim.Adam on the CPU in tests/test_optim_ref_cpu.py, which also shows that the bounds notice a wrong kernel).

Every case is ONE step from known operands.  p, g, m, v and the step counts live in arenas with a band of 64 sentinel floats on both
sides and sentinel gaps between the segments; so do the kernel's own scratch (`partial`, `norm_coef`).  The bands and gaps must
survive every step.  The parameters are Parameter(arena[k:k + n]) with the gradient a like-shaped view of the gradient arena; the
moments are misaligned by presetting opt.state[p] with views.  No pointer table is built by hand: ClipAdam lays out every table.
The reference is fed the device's own coefficient (norm_coef[1]), so the norm's rounding does not leak into the element-wise
comparison; the norm and the coefficient have their own checks: bitwise where the sum of squares is exact in any order (all-ones
gradients, planted powers of two), bounded by the summation structure (optim_ref.norm_depth) otherwise.

Every comparison prints its max ratio |err| / (K x bound) and max-abs error (run with -s).  Measured on an MI355X, the worst over
the 36 tables of optim_ref.ADAM_TABLES (K = 4; 1 = at the bound):
  p 0.25    m 0.24    v 0.22    written gradient 1.0 of its single rounding u |g coef| (no constant: a rounding next to a power of
                                two fills it)
  norm      relative error <= 7.5e-8 against fp64, 0.07 of the bound of its summation structure (9e-7 for the tables of small
            segments, 8.5e-6 where a thread adds 256 squares one after the other; the 2e-6 of tests/test_gpu_train.py lies between)
i.e. the kernel sits at the float32 restatement's own distance from fp64 (that restatement reaches 1.0 of the bound WITHOUT K, 0.25
with), and the wrong kernels of tests/test_optim_ref_cpu.py are 1e4 .. 1e6 bounds away.  The whole file takes 7 s, 2 of them the
first test's library load.

One defect was found, by test_alignment_forms_compute_the_same_bits: the same values gave other bits of p, m and v depending on the
operands' alignment.  optim_adam_kernel's `upd` left the fusing of g + wd p and beta2 v + (1 - beta2) g g to the compiler's
contraction, which made FMAs of them in the float4 loop and rounded products in the two scalar loops (a misaligned operand; the < 4
tail elements of an aligned segment).  Both were inside the bounds; `upd` now spells every product-and-sum as fmaf, the float4
loop's arithmetic, and the forms agree bitwise.  Nothing else was found in csrc/optim.hip or cvc/optim.py.
"""
import functools

import numpy as np
import pytest
import torch

import optim_ref as OR
from optim_ref import BAND, CHUNK, SENTINEL

pytestmark = pytest.mark.gpu

BADARG = -1
KEYS = ("p", "g", "m", "v")


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
    return OR.values(OR.TABLES[name])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------ snapshots of an optimizer's tensors
class Snap:
    """p, g, m, v of every parameter that has a gradient, flat and side by side on the host; the step counts; the segment sizes"""

    def __init__(self, opt, params):
        self.act = [i for i, q in enumerate(params) if q.grad is not None]
        dev = params[0].device
        ps = [params[i] for i in self.act]
        sts = [opt.state[q] for q in ps]

        def cat(ts):
            return torch.cat([t.detach().reshape(-1) for t in ts]).cpu().numpy()
        self.p, self.g = cat(ps), cat([q.grad for q in ps])
        self.m = cat([st["exp_avg"] if len(st) else torch.zeros_like(q) for q, st in zip(ps, sts)])
        self.v = cat([st["exp_avg_sq"] if len(st) else torch.zeros_like(q) for q, st in zip(ps, sts)])
        self.steps = torch.stack([st["step"].detach().to(dev, torch.float32).reshape(()) if len(st) else torch.zeros((), device=dev)
                                  for st in sts]).cpu().numpy()
        self.ns = np.array([q.numel() for q in ps], dtype=np.int64)
        self.off = np.concatenate(([0], np.cumsum(self.ns)))

    def seg(self, key, j):
        """operand `key` of the j-th ACTIVE parameter"""
        return getattr(self, key)[self.off[j]:self.off[j + 1]]


def verify(opt, params, pre, post, coef, what, written="clipped", k=None):
    """one step from `pre` to `post` against step_fp64 under the device's coefficient: p, m, v inside K x their bounds, the gradient
    as `written` ("clipped": g coef within its one rounding; "zero"; "untouched": the same bits), every active step count + 1,
    lr == 0 leaves p's bits alone.  lr and weight decay are the param groups' (one parameter per group) at the time of the call."""
    assert pre.act == post.act
    groups = [opt.param_groups[i] for i in pre.act]
    lr = np.repeat(np.array([g["lr"] for g in groups], dtype=np.float32), pre.ns)
    wd = np.repeat(np.array([g["weight_decay"] for g in groups], dtype=np.float32), pre.ns)
    b1, b2 = opt.param_groups[0]["betas"]
    ref = OR.step_fp64(pre.p, pre.g, pre.m, pre.v, np.repeat(pre.steps, pre.ns), lr, wd, b1, b2, opt.param_groups[0]["eps"], coef)
    r = OR.check_elements(post.p, post.m, post.v, post.g if written == "clipped" else None, ref, what, k)
    if written == "zero":
        assert not bits(post.g).any(), what
    elif written == "untouched":
        assert same_bits(post.g, pre.g), what
    assert np.array_equal(post.steps, pre.steps + 1), what
    still = (lr == 0) & np.isfinite(ref.p)                  # (0 x NaN is NaN: a NaN coefficient poisons these too, as in torch)
    assert same_bits(post.p[still], pre.p[still]), what + ": lr == 0 moved a parameter"
    moved = still & (pre.g != 0)
    if moved.any() and np.isfinite(coef) and coef != 0:
        assert (bits(post.m[moved]) != bits(pre.m[moved])).any() and (bits(post.v[moved]) != bits(pre.v[moved])).any(), what
    return r


# ------------------------------------------------------------------------------------------------ one table in sentinel-banded arenas
class Rig:
    """A ClipAdam over one table of tests/optim_ref.py.  vals: other operands than the table's seeded ones (a Values); no_grad:
    segments whose parameter gets no gradient (and no preset state)."""

    def __init__(self, dev, table, vals=None, no_grad=()):
        from cvc.optim import ClipAdam
        self.table, self.dev = table, dev
        vals = values(table.name) if vals is None else vals
        segs = table.segs
        starts, size = OR.layout(segs)
        self.idx = {k: np.concatenate([np.arange(a + s.offs[j], a + s.offs[j] + s.n) for s, a in zip(segs, starts)])
                    for j, k in enumerate(KEYS)}
        self.used, host = {}, {}
        live = np.repeat(np.array([i not in no_grad for i in range(len(segs))]), [s.n for s in segs])
        for k in KEYS:
            host[k] = np.full(size, SENTINEL, dtype=np.float32)
            at = self.idx[k] if k == "p" else self.idx[k][live]
            host[k][at] = getattr(vals, k) if k == "p" else getattr(vals, k)[live]
            self.used[k] = np.zeros(size, dtype=bool)
            self.used[k][at] = True
        self.arena = {k: torch.from_numpy(host[k]).to(dev) for k in KEYS}
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
        self.opt = ClipAdam(groups, betas=table.betas, eps=OR.EPS)
        for i, (s, a, q) in enumerate(zip(segs, starts, self.params)):
            if i not in no_grad:
                self.opt.state[q] = {"step": self.steps[BAND + i], "exp_avg": self.arena["m"][a + s.offs[2]:a + s.offs[2] + s.n],
                                     "exp_avg_sq": self.arena["v"][a + s.offs[3]:a + s.offs[3] + s.n]}
            for j, t in enumerate((q, q.grad) + ((self.opt.state[q]["exp_avg"], self.opt.state[q]["exp_avg_sq"]) if i not in no_grad else ())):
                if t is not None:
                    assert (t.data_ptr() % 16 == 0) == (s.offs[j] == 0), (i, j)
        self.partial = self.nc = None

    def own_scratch(self):
        """`partial` and `norm_coef` of the table ClipAdam built, moved between sentinel bands (the table's key, hence the table,
        stays)"""
        t = self.opt._build_table()
        if self.partial is None or t[3].data_ptr() != self.partial[BAND:].data_ptr():
            self.nchunk = t[6]
            self.partial = torch.full((self.nchunk + 2 * BAND,), SENTINEL, device=self.dev)
            self.nc = torch.full((2 + 2 * BAND,), SENTINEL, device=self.dev)
            self.nc[BAND:BAND + 2] = 0
            self.opt._table = t[:3] + (self.partial[BAND:BAND + self.nchunk], self.nc[BAND:BAND + 2]) + t[5:]
        return self.opt._table

    def step(self, max_norm=None, inv=None, plain=False, **kw):
        """one clip_and_step (plain: opt.step()) -> (pre, post, norm, coef), the last two as the device left them in norm_coef"""
        self.own_scratch()
        pre = Snap(self.opt, self.params)
        if plain:
            self.opt.step()
        else:
            ret = self.opt.clip_and_step(self.table.max_norm if max_norm is None else max_norm, self.table.inv if inv is None else inv, **kw)
            assert ret.data_ptr() == self.nc[BAND:].data_ptr()
        torch.cuda.synchronize()
        post = Snap(self.opt, self.params)
        nc = self.nc.cpu().numpy()
        self.bands_intact()
        return pre, post, nc[BAND], nc[BAND + 1]

    def bands_intact(self):
        for k in KEYS:
            a = self.arena[k].cpu().numpy()
            assert (a[~self.used[k]] == SENTINEL).all(), "the %s arena was written outside its segments" % k
        for name, t, n in (("steps", self.steps, len(self.table.segs)), ("partial", self.partial, self.nchunk), ("norm_coef", self.nc, 2)):
            a = t.cpu().numpy()
            assert (a[:BAND] == SENTINEL).all() and (a[BAND + n:] == SENTINEL).all(), "%s: a sentinel band was written" % name

    def grads(self, pre):
        return [pre.seg("g", j) for j in range(len(pre.ns))]


def with_values(table, **over):
    """the table's seeded operands with some replaced (arrays, or a function of the seeded array)"""
    v = values(table.name)
    return v._replace(**{k: (f(getattr(v, k)) if callable(f) else f).astype(np.float32) for k, f in over.items()})


def fresh(table, beta1=0.5, wd=0.0, lr=None):
    """the table with zero step counts (hence zero moments), one weight decay and beta1"""
    return table._replace(segs=[s._replace(t=0, wd=wd, lr=s.lr if lr is None else lr) for s in table.segs], betas=(beta1, table.betas[1]))


def zero_moments(table):
    return with_values(table, m=np.zeros_like, v=np.zeros_like)


EXACT_TABLES = [t.name for t in OR.SHAPE_TABLES] + ["small-sizes-x-forms", "chunk-sizes-g+1", "chunk-sizes-p+1", "multi-chunk-aligned",
                                                    "multi-chunk-g+2"]
BIG = "shape-300+2"               # nchunk 305 > nseg 302 > 256, every alignment form, a misaligned multi-chunk segment


# ------------------------------------------------------------------------------------------------ the library and the tables
def test_chunk_size_and_the_tables_clipadam_builds(dev, L):
    from cvc.optim import _CHUNK_DT, _SEG_DT
    assert int(L.cvc_optim_chunk_elems()) == CHUNK == 65536
    rig = Rig(dev, OR.TABLES[BIG])
    t = rig.own_scratch()
    ns = [s.n for s in rig.table.segs]
    seg, start = OR.chunk_table(ns)
    chunks = t[2].cpu().numpy().view(_CHUNK_DT)
    assert t[5] == len(ns) and t[6] == len(seg) == 305
    assert np.array_equal(chunks["seg"], seg) and np.array_equal(chunks["start"], start) and not chunks["pad"].any()
    segs = t[1].cpu().numpy().view(_SEG_DT)
    assert np.array_equal(segs["n"], ns)
    assert np.array_equal(segs["lr"], np.array([s.lr for s in rig.table.segs], dtype=np.float32))
    assert np.array_equal(segs["wd"], np.array([s.wd for s in rig.table.segs], dtype=np.float32))
    for k, st in enumerate(("p", "g", "m", "v")):
        want = [x.data_ptr() for x in ([q for q in rig.params], [q.grad for q in rig.params], [rig.opt.state[q]["exp_avg"] for q in rig.params],
                                       [rig.opt.state[q]["exp_avg_sq"] for q in rig.params])[k]]
        assert np.array_equal(segs[st], np.array(want, dtype=np.uint64))
    assert np.array_equal(segs["step"], rig.steps.data_ptr() + 4 * (BAND + np.arange(len(ns), dtype=np.uint64)))


# ------------------------------------------------------------------------------------------------ one step, element-wise
@pytest.mark.parametrize("name", [t.name for t in OR.ADAM_TABLES])
def test_one_step_elementwise_against_fp64(dev, name):
    """p, m, v and the written gradient inside their bounds under the device's coefficient; the norm inside the bound of its summation
    structure; the coefficient from the device's norm within 4 u (inv exactly when the clip is off or not reached); every step count
    + 1; lr == 0 leaves p alone; all sentinels intact"""
    table = OR.TABLES[name]
    rig = Rig(dev, table)
    pre, post, norm, coef = rig.step()
    verify(rig.opt, rig.params, pre, post, coef, name)
    OR.check_norm(norm, rig.grads(pre), table.inv, pre.ns, rig.nchunk, name)
    OR.check_coef(norm, coef, table.max_norm, table.inv, name)
    if table.max_norm == 1e9:
        assert coef == np.float32(table.inv)
    assert float(rig.opt.last_norm) == norm


def test_a_negative_max_norm_switches_the_clip_off(dev):
    rig = Rig(dev, OR.TABLES["shape-257"])
    pre, post, norm, coef = rig.step(max_norm=-1.0, inv=0.25)
    assert coef == np.float32(0.25)
    OR.check_norm(norm, rig.grads(pre), 0.25, pre.ns, rig.nchunk, "max_norm -1")
    verify(rig.opt, rig.params, pre, post, coef, "max_norm -1")


# ------------------------------------------------------------------------------------------------ exact checks
@pytest.mark.parametrize("name", EXACT_TABLES)
def test_norm_of_all_ones_is_exact(dev, name):
    """every partial sum is an integer below 2^24 in any order: norm_coef[0] is float32(sqrt(N)) bitwise -- an element summed twice or
    left out changes N"""
    table = OR.TABLES[name]
    n = int(values(name).off[-1])
    assert n < 2 ** 24
    rig = Rig(dev, table, with_values(table, g=np.ones_like))
    _pre, _post, norm, coef = rig.step(max_norm=0.0, inv=1.0)
    assert norm == np.float32(np.sqrt(np.float64(n))) and coef == np.float32(1), (norm, n)


PLANTED = OR.Table("planted", [OR.Seg(3 * CHUNK + 1023 + 4, OR.ALIGNED, 1e-3, 0.0, 0), OR.Seg(CHUNK + 4, OR.FORMS[4], 1e-3, 0.0, 0),
                               OR.Seg(7, OR.ALIGNED, 1e-3, 0.0, 0)], OR.DEFAULT_BETAS, 0.0, 1.0)
OR.TABLES.setdefault("planted", PLANTED)


def planted_positions(segs):
    """up to 12 (segment, element): the first, the last of the first segment, the last of the last, both sides of every chunk
    boundary, the first and last element of the aligned form's scalar tail (the < 4 elements behind the last whole float4)"""
    last = len(segs) - 1
    cand = [(0, 0), (0, segs[0].n - 1), (last, segs[last].n - 1)]
    for i, s in enumerate(segs):
        for c in range(1, -(-s.n // CHUNK)):
            cand += [(i, c * CHUNK - 1), (i, c * CHUNK)]
    for i, s in enumerate(segs):
        if s.offs == OR.ALIGNED and s.n % 4:
            cand += [(i, s.n - s.n % 4), (i, s.n - 1)]
    out = []
    for c in cand:
        if c not in out:
            out.append(c)
    return out[:12]


@pytest.mark.parametrize("name", EXACT_TABLES + ["planted"])
def test_norm_of_planted_powers_of_two_is_exact(dev, name):
    """g = 0 but 2^j at the edge positions: the sum of 4^j is exact in any order, the norm is float32(sqrt(sum)) bitwise -- an edge
    element that is skipped or read twice shows"""
    table = OR.TABLES[name]
    v = values(name)
    g = np.zeros_like(v.g)
    pos = planted_positions(table.segs)
    if name == "planted":
        n0 = table.segs[0].n
        assert len(pos) == 12 and {(0, CHUNK - 1), (0, 3 * CHUNK), (0, n0 - 3), (0, n0 - 1), (1, CHUNK), (2, 6)} <= set(pos)
    for j, (i, e) in enumerate(pos):
        g[v.off[i] + e] = 2.0 ** j
    rig = Rig(dev, table, v._replace(g=g))
    _pre, _post, norm, _coef = rig.step(max_norm=0.0, inv=1.0)
    want = np.float32(np.sqrt(np.float64(sum(4 ** j for j in range(len(pos))))))
    assert norm == want, (norm, want, pos)


@pytest.mark.parametrize("name", EXACT_TABLES)
def test_every_element_is_updated_exactly_once(dev, name):
    """clip off, inv 0.5, beta1 0.5, zero moments, no weight decay: the written gradient is 0.5 g and exp_avg 0.25 g, bitwise -- an
    element updated twice would hold 0.25 g and 0.3125 g, one left out g and 0"""
    table = fresh(OR.TABLES[name])
    rig = Rig(dev, table, zero_moments(OR.TABLES[name]))
    pre, post, _norm, coef = rig.step(max_norm=0.0, inv=0.5)
    assert coef == np.float32(0.5)
    assert same_bits(post.g, np.float32(0.5) * pre.g) and same_bits(post.m, np.float32(0.25) * pre.g)
    assert (post.steps == 1).all()
    verify(rig.opt, rig.params, pre, post, coef, name + " fresh")


def test_write_grad_modes_and_determinism(dev):
    """write_grad=False leaves g's bits, zero_grad=True leaves zeros, and p, m, v do not depend on it; two runs from the same inputs
    give the same bits everywhere, the norm under an active clip included"""
    table = OR.TABLES[BIG]
    runs = {}
    for mode, kw in (("clipped", {}), ("again", {}), ("untouched", dict(write_grad=False)), ("zero", dict(zero_grad=True)),
                     ("zero-over-write", dict(write_grad=False, zero_grad=True))):
        rig = Rig(dev, table)
        runs[mode] = rig.step(**kw)
    pre, post, norm, coef = runs["clipped"]
    assert 0 < coef < 1
    for mode, (pre2, post2, norm2, coef2) in runs.items():
        assert same_bits(pre2.g, pre.g)
        assert bits(np.array([norm2, coef2])).tolist() == bits(np.array([norm, coef])).tolist(), mode
        assert all(same_bits(getattr(post2, k), getattr(post, k)) for k in "pmv") and np.array_equal(post2.steps, post.steps), mode
    assert same_bits(runs["again"][1].g, post.g) and not same_bits(post.g, pre.g)
    assert same_bits(runs["untouched"][1].g, pre.g)
    assert not bits(runs["zero"][1].g).any() and not bits(runs["zero-over-write"][1].g).any()


def test_alignment_forms_compute_the_same_bits(dev):
    """the same values through the float4 form (all four operands aligned) and the scalar form (every operand one element off):
    with the clip off (no norm in the coefficient) p, m, v and the written gradient are bit-identical"""
    ns = OR.SMALL_N + (CHUNK + 4, 2 * CHUNK + 3)
    a = OR.Table("forms-aligned", [OR.Seg(n, OR.ALIGNED, *OR._cycle(i)) for i, n in enumerate(ns)], OR.DEFAULT_BETAS, 0.0, 0.5)
    b = a._replace(segs=[s._replace(offs=(1, 1, 1, 1)) for s in a.segs])
    vals = OR.values(a)
    (_pa, post_a, norm_a, coef_a), (_pb, post_b, norm_b, coef_b) = Rig(dev, a, vals).step(), Rig(dev, b, vals).step()
    assert coef_a == coef_b == np.float32(0.5)
    assert all(same_bits(getattr(post_a, k), getattr(post_b, k)) for k in "pgmv")
    assert abs(float(norm_a) - float(norm_b)) <= 2 * OR.norm_rel_bound(ns, 6) * float(norm_a)       # two summation orders


# ------------------------------------------------------------------------------------------------ the skip word
@pytest.mark.parametrize("mode,kw", [("zero", dict(zero_grad=True)), ("clipped", {}), ("untouched", dict(write_grad=False))])
def test_a_set_skip_word_voids_the_step(dev, mode, kw):
    """p, m, v and every step count keep their bits, norm_coef is [0, 0]; the gradients are zeroed under zero_grad=True (what
    Trainer asks for) and untouched otherwise"""
    rig = Rig(dev, OR.TABLES[BIG])
    skip = torch.tensor([7], dtype=torch.int32, device=dev)
    pre, post, norm, coef = rig.step(skip=skip, **kw)
    assert bits(np.array([norm, coef])).tolist() == [0, 0]
    assert all(same_bits(getattr(post, k), getattr(pre, k)) for k in "pmv") and np.array_equal(post.steps, pre.steps)
    assert (not bits(post.g).any()) if mode == "zero" else same_bits(post.g, pre.g)
    assert int(skip) == 7
    # the word cleared: the same table steps
    skip.zero_()
    pre, post, norm, coef = rig.step(skip=skip, **kw)
    verify(rig.opt, rig.params, pre, post, coef, "after a void step (%s)" % mode, written=mode)


@pytest.mark.parametrize("kw", [dict(zero_grad=True), {}])
def test_a_clear_skip_word_is_no_skip_word(dev, kw):
    table = OR.TABLES[BIG]
    skip = torch.zeros(1, dtype=torch.int32, device=dev)
    (_p1, post1, norm1, coef1), (_p2, post2, norm2, coef2) = Rig(dev, table).step(**kw), Rig(dev, table).step(skip=skip, **kw)
    assert bits(np.array([norm1, coef1])).tolist() == bits(np.array([norm2, coef2])).tolist()
    assert all(same_bits(getattr(post1, k), getattr(post2, k)) for k in "pgmv") and np.array_equal(post1.steps, post2.steps)


# ------------------------------------------------------------------------------------------------ NaN and Inf gradients
@pytest.mark.parametrize("bad", ["nan", "inf"])
def test_one_nonfinite_gradient_element(dev, bad):
    """ordinary NaN arithmetic, one step each.  NaN: the norm, the coefficient and every element of p, m and v are NaN (torch's
    clamp(NaN, max=1); fminf would have returned 1).  Inf: the norm is Inf, the coefficient 0, and the step is step_fp64's under
    that coefficient (the Inf element's g coef is NaN, every other gradient is cancelled)"""
    table = OR.TABLES["shape-300"]
    v = values(table.name)
    g = v.g.copy()
    g[v.off[123] + 2] = float(bad)
    rig = Rig(dev, table, v._replace(g=g))
    pre, post, norm, coef = rig.step()
    if bad == "nan":
        assert norm != norm and coef != coef
        assert all(np.isnan(getattr(post, k)).all() for k in "pgmv")
    else:
        assert norm == np.float32("inf") and coef == 0
        assert np.isnan(post.p[v.off[123] + 2]) and np.isnan(post.p).sum() == 1
    verify(rig.opt, rig.params, pre, post, coef, bad)
    OR.check_coef(norm, coef, table.max_norm, table.inv, bad)


# ------------------------------------------------------------------------------------------------ ClipAdam's behaviour
def test_a_parameter_without_gradient_keeps_an_empty_state(dev):
    table = OR.TABLES["shape-257"]
    dead = (0, 100, 256)
    rig = Rig(dev, table, no_grad=dead)
    before = [rig.params[i].detach().clone() for i in dead]
    pre, post, _norm, coef = rig.step()
    assert len(pre.act) == 257 - 3
    verify(rig.opt, rig.params, pre, post, coef, "three parameters without gradient")
    for i, b in zip(dead, before):
        assert len(rig.opt.state[rig.params[i]]) == 0 and torch.equal(rig.params[i].detach(), b)


def _new_grads(rig, seed):
    """fresh gradients of the table's scales, written into the gradient views"""
    rng = np.random.default_rng(seed)
    for q in rig.params:
        if q.grad is not None:
            q.grad.copy_(torch.from_numpy((rng.standard_normal(q.numel()) * 10.0 ** rng.integers(-3, 2)).astype(np.float32)))


def test_a_scheduler_rewrites_the_rates_in_place(dev):
    rig = Rig(dev, OR.TABLES["shape-300"])
    pre, post, _norm, coef = rig.step()
    verify(rig.opt, rig.params, pre, post, coef, "before the scheduler")
    t0 = rig.opt._table
    for i, g in enumerate(rig.opt.param_groups):
        g["lr"] = g["lr"] * 0.5 if i % 2 else 3e-4
    _new_grads(rig, 1)
    pre, post, _norm, coef = rig.step()
    assert rig.opt._table is t0 and not rig.opt._retired
    assert len({g["lr"] for g in rig.opt.param_groups}) > 2
    verify(rig.opt, rig.params, pre, post, coef, "new rates")                 # verify() reads the param groups' current rates
    rig.opt.param_groups[5]["weight_decay"] = 0.02
    rig.opt.sync_hyperparameters()
    _new_grads(rig, 2)
    pre, post, _norm, coef = rig.step()
    assert rig.opt._table is t0
    verify(rig.opt, rig.params, pre, post, coef, "a new weight decay")


def test_a_first_gradient_at_a_later_step_rebuilds_the_table(dev):
    table = fresh(OR.TABLES["shape-257"], beta1=0.9, wd=0.01)
    late = 200
    rig = Rig(dev, table, zero_moments(OR.TABLES["shape-257"]), no_grad=(late,))
    for it in range(2):
        pre, post, _norm, coef = rig.step()
        verify(rig.opt, rig.params, pre, post, coef, "step %d" % (it + 1))
        _new_grads(rig, 10 + it)
    old = rig.opt._table
    q = rig.params[late]
    q.grad = torch.full_like(q, 0.25)
    pre, post, norm, coef = rig.step()
    assert rig.opt._table is not old and any(t is old for t in rig.opt._retired)
    assert len(pre.act) == 257 and pre.steps[late] == 0 and (np.delete(pre.steps, late) == 2).all()
    verify(rig.opt, rig.params, pre, post, coef, "step 3, the late parameter's first")
    assert float(rig.opt.state[q]["step"]) == 1 and (np.delete(post.steps, late) == 3).all()
    OR.check_norm(norm, rig.grads(pre), table.inv, pre.ns, rig.nchunk, "the rebuilt table")


def _plain_params(dev, seed, sizes=(5, 1027, 300, CHUNK + 1)):
    rng = np.random.default_rng(seed)
    ps = [torch.nn.Parameter(torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(dev)) for n in sizes]
    groups = [{"params": [q], "lr": (1e-3, 1e-4)[i % 2], "weight_decay": (0.0, 0.01)[i % 2]} for i, q in enumerate(ps)]
    return ps, groups


def _plain_grads(ps, seed):
    rng = np.random.default_rng(seed)
    for q in ps:
        q.grad = torch.from_numpy(rng.standard_normal(q.numel()).astype(np.float32)).to(q.device)


def test_resume_from_torch_adam_with_cpu_step_counts_and_back(dev):
    """load_state_dict from a torch.optim.Adam(capturable=False) (its `step` is a CPU tensor), then ONE ClipAdam step: the counts go
    on, the update is the reference's from the loaded moments.  And back: a torch.optim.Adam resumes from ClipAdam's state and
    steps; that step is torch's arithmetic in torch's order (the capturable form divides by the step size twice more), so it is
    held to 2 K x the bounds -- a misread moment or count is off by orders of magnitude, not by a rounding"""
    from cvc.optim import ClipAdam
    pa, ga = _plain_params(dev, 3)
    ref = torch.optim.Adam(ga, betas=(0.8, 0.99), capturable=False, foreach=False)
    for it in range(2):
        _plain_grads(pa, 20 + it)
        ref.step()
    assert not ref.state[pa[0]]["step"].is_cuda
    pb, gb = _plain_params(dev, 3)
    with torch.no_grad():
        for q, r in zip(pb, pa):
            q.copy_(r)
    opt = ClipAdam(gb, betas=(0.8, 0.99))
    opt.load_state_dict(ref.state_dict())
    assert not opt.state[pb[0]]["step"].is_cuda
    _plain_grads(pb, 30)
    pre = Snap(opt, pb)
    assert (pre.steps == 2).all() and all(same_bits(pre.seg("m", j), ref.state[r]["exp_avg"].cpu().numpy()) for j, r in enumerate(pa))
    opt.clip_and_step(1.0, 1.0)
    torch.cuda.synchronize()
    post = Snap(opt, pb)
    coef = float(opt._table[4][1])
    verify(opt, pb, pre, post, coef, "resumed from torch.optim.Adam")
    assert all(opt.state[q]["step"].is_cuda and float(opt.state[q]["step"]) == 3 for q in pb)
    # ... and back
    pc, gc = _plain_params(dev, 3)
    with torch.no_grad():
        for q, r in zip(pc, pb):
            q.copy_(r)
    back = torch.optim.Adam(gc, capturable=True)
    back.load_state_dict(opt.state_dict())
    _plain_grads(pc, 31)
    pre = Snap(back, pc)
    assert (pre.steps == 3).all() and same_bits(pre.m, post.m) and same_bits(pre.v, post.v)
    back.step()
    torch.cuda.synchronize()
    verify(back, pc, pre, Snap(back, pc), 1.0, "torch.optim.Adam resumed from ClipAdam", written="untouched", k=2 * OR.K)


def test_step_alone_is_the_unclipped_update(dev):
    table = OR.TABLES[BIG]
    (pre1, post1, norm1, coef1), (_pre2, post2, norm2, coef2) = Rig(dev, table).step(plain=True), Rig(dev, table).step(0.0, 1.0, write_grad=False)
    assert coef1 == coef2 == 1 and bits(np.array([norm1])).tolist() == bits(np.array([norm2])).tolist()
    assert all(same_bits(getattr(post1, k), getattr(post2, k)) for k in "pgmv") and same_bits(post1.g, pre1.g)


# ------------------------------------------------------------------------------------------------ argument checks
def test_bad_arguments_are_refused_before_any_launch(dev, L):
    from cvc import hip
    rig = Rig(dev, OR.TABLES["shape-1-1"])
    t = rig.own_scratch()
    good = dict(segs=t[1].data_ptr(), nseg=t[5], chunks=t[2].data_ptr(), nchunk=t[6], max_norm=1.0, inv_world=1.0, beta1=0.9, beta2=0.999,
                eps=1e-8, write_grad=1, partial=t[3].data_ptr(), norm_coef=t[4].data_ptr(), skip=None, stream=hip._stream())
    before = Snap(rig.opt, rig.params)
    for over in (dict(segs=None), dict(chunks=None), dict(partial=None), dict(norm_coef=None), dict(nseg=0), dict(nseg=-1), dict(nchunk=0),
                 dict(nchunk=-3), dict(inv_world=0.0), dict(inv_world=-1.0), dict(beta1=1.0), dict(beta1=-0.1), dict(beta2=1.0),
                 dict(beta2=-0.5), dict(beta2=1.5), dict(eps=-1e-8)):
        a = dict(good, **over)
        assert L.cvc_adam_clip_step(*a.values()) == BADARG, over
    torch.cuda.synchronize()
    after = Snap(rig.opt, rig.params)
    assert all(same_bits(getattr(after, k), getattr(before, k)) for k in "pgmv") and np.array_equal(after.steps, before.steps)
    assert not rig.nc[BAND:BAND + 2].cpu().numpy().any() and (rig.partial.cpu().numpy() == SENTINEL).all()
    rig.bands_intact()
    # the same arguments, all good: the step runs
    assert L.cvc_adam_clip_step(*good.values()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(Snap(rig.opt, rig.params).steps, before.steps + 1)
