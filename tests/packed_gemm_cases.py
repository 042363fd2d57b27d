"""Shared pieces of tests/test_gpu_packed_gemm.py and tests/test_packed_gemm_cpu.py (not collected: no test_ prefix): case
builders, torch fp64 restatements and C-ABI callers of the packed decode GEMM's entry points (csrc/gemm_packed.hip:
cvc_packed_lstm_fwd, cvc_packed_lstm_embgate_fwd, cvc_packed_lstm_embgate_ex_fwd, cvc_packed_lstm_late_fwd with early = NULL,
cvc_packed_lstm_step_fwd, cvc_packed_linear_fwd) and of cvc_top2_final (csrc/vocab.hip), which merges the linear form's records.

Everything above the "device side" line runs on the CPU (tests/test_packed_gemm_cpu.py checks the restatements against
torch.nn.LSTMCell, torch.log_softmax and topk); the callers below it pre-fill every output with NaN."""
import contextlib
import math
import os
import re

import torch

from attn_step_cases import all_nan, bits, close, nan_buf, same_bits, stream_handle  # noqa: F401  (re-exported to the tests)

OP_TOL = dict(rtol=2e-5, atol=2e-5)              # tests/test_gpu_parity.py, tests/attn_step_cases.py
E_BADARG = -1                                    # include/cvc_hip.h
NO_INDEX = 0x7FFFFFFF                            # index of an absent record entry (its value is -inf)
QUAD_BYTES = 64 * 4 * 4                          # one quad of the activation layout [K/4][64][4]

# K / 32 of the K-loop sweep (section 1 of the GPU file): see ring_path() and test_packed_gemm_cpu.py, which checks against the
# constants of the source that these reach every branch of the register ring in every mode.  (32 is there for the 4-wave forms:
# n_my = 8 everywhere, the one drain length of their single-pass range that the other sizes leave out.)
SWEEP_CHUNKS = (1, 6, 12, 14, 20, 26, 28, 32, 36, 42, 52, 60)


# ------------------------------------------------------------------ the K loop's paths, from the source's constants
def source_constants():
    """CVC_PACKED_DEPTH (4-wave forms, modes 0 / 1), CVC_PACKED_DEPTH8 (8-wave form, mode 2) and the rotation multiplier, read from
    csrc/gemm_packed.hip -> {mode: (NW, DEPTH)}, rot_mul"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "cyclical-visual-captioning_amd", "csrc", "gemm_packed.hip")).read()
    val = lambda name: int(re.search(r"#define\s+" + name + r"\s+(\d+)", src).group(1))
    d4, d8 = val("CVC_PACKED_DEPTH"), val("CVC_PACKED_DEPTH8")
    return {0: (4, d4), 1: (4, d4), 2: (8, d8)}, val("CVC_ROT_MUL")


def wave_counts(nchunk, nw):
    """n_my of wave kw = 0 .. nw - 1: chunks kw, kw + nw, ... of nchunk"""
    return [(nchunk - kw + nw - 1) // nw if nchunk > kw else 0 for kw in range(nw)]


def ring_path(n_my, depth):
    """the branch of the register ring a wave with n_my chunks takes: ("short", 0, n_my) below the ring's depth, else
    ("ring", passes of the steady loop, chunks left to the drain)"""
    if n_my < depth:
        return ("short", 0, n_my)
    j = 0
    while j + 2 * depth - 1 <= n_my:
        j += depth
    return ("ring", j // depth, n_my - j)


# ------------------------------------------------------------------ fp64 restatements
def lstm_ref(x, w, c_prev, terms=()):
    """fp64 LSTM cell on fp32 inputs cast up: pre = x @ w.T + sum(terms), gates in checkpoint order i, f, g, o.
    -> dict(gates [M, 4R] activated, c [M, R], h [M, R])"""
    pre = x.double() @ w.double().t()
    for t in terms:
        pre = pre + t.double()
    i, f, g, o = pre.chunk(4, 1)
    i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
    c = f * c_prev.double() + i * g
    return dict(gates=torch.cat([i, f, g, o], 1), c=c, h=o * torch.tanh(c))


def linear_ref(x, w, b=None):
    y = x.double() @ w.double().t()
    return y if b is None else y + b.double()


def block_records(y, V=None):
    """The per-block records of cvc_packed_linear_fwd(top2_part) restated on logits y [M, V] (any float dtype; values are kept in
    y's dtype, the sum in fp64): per 32-column block b and row m
    -> dict(v1, i1, v2, i2, mx [M, nblk] and se [M, nblk] fp64 = sum over the block's valid columns of exp(v - mx)).
    Equal values: the lower index first.  An absent second entry (one valid column) is (-inf, NO_INDEX)."""
    M, V = y.shape[0], (y.shape[1] if V is None else V)
    nblk = (V + 31) // 32
    pad = torch.full((M, nblk * 32), -math.inf, dtype=y.dtype, device=y.device)
    pad[:, :V] = y[:, :V]
    pad = pad.view(M, nblk, 32)
    vals, idx = torch.sort(pad, dim=2, descending=True, stable=True)             # stable: the lower column first among equals
    idx = idx + (torch.arange(nblk, device=y.device) * 32).view(1, nblk, 1)
    v1, v2 = vals[..., 0], vals[..., 1]
    i1 = idx[..., 0]
    i2 = torch.where(idx[..., 1] < V, idx[..., 1], torch.full_like(idx[..., 1], NO_INDEX))
    se = torch.exp(pad.double() - v1.double().unsqueeze(2)).sum(2)
    return dict(v1=v1, i1=i1, v2=v2, i2=i2, mx=v1.clone(), se=se)


def merge_records(rec, unk):
    """cvc_top2_final restated on the host in fp64: the best two of all record entries (value descending, index ascending), the
    log-sum-exp of the row from (mx, se), then the UNK rule -- UNK on top gives the runner-up and ITS log-prob.
    -> (word [M] int64, logprob [M] fp64, i1, i2)"""
    v = torch.cat([rec["v1"], rec["v2"]], 1).double()
    i = torch.cat([rec["i1"], rec["i2"]], 1).long()
    order = torch.argsort(i, dim=1, stable=True)
    v, i = v.gather(1, order), i.gather(1, order)
    v, order = torch.sort(v, dim=1, descending=True, stable=True)
    i = i.gather(1, order)
    mx = rec["mx"].double().max(1).values
    lse = mx + torch.log((rec["se"].double() * torch.exp(rec["mx"].double() - mx.unsqueeze(1))).sum(1))
    use2 = (i[:, 0] == unk) & (i[:, 1] != NO_INDEX)
    word = torch.where(use2, i[:, 1], i[:, 0])
    return word, torch.where(use2, v[:, 1], v[:, 0]) - lse, i[:, 0], i[:, 1]


def select_ref(y, unk):
    """word selection straight from the logits y [M, V] in fp64 -> (word, logprob, deciding margin [M]): the gap between the
    chosen word and the best word that is neither it nor UNK-on-top (what a perturbation has to cross to change the answer)"""
    y = y.double()
    V = y.shape[1]
    lsm = torch.log_softmax(y, 1)
    vals, idx = torch.sort(y, dim=1, descending=True, stable=True)
    use2 = (idx[:, 0] == unk) & (V > 1)
    word = torch.where(use2, idx[:, 1], idx[:, 0])
    # deciding margins: UNK on top -> the word is the runner-up, decided by (top - second: UNK stays on top) and (second - third);
    # otherwise by (top - second) alone
    m01 = vals[:, 0] - vals[:, 1]
    m12 = vals[:, 1] - vals[:, 2] if V > 2 else torch.full_like(m01, math.inf)
    margin = torch.where(use2, torch.minimum(m01, m12), m01)
    return word, lsm.gather(1, word.view(-1, 1)).view(-1), margin


# ------------------------------------------------------------------ case builders (CPU tensors, fixed seeds)
def lstm_case(seed, M, R, K, V=50):
    """w / sqrt(K) and x ~ N(0, 1): unit-scale pre-activations at every K; biases, the per-row gate term and the table rows at
    half that scale; words include 0 and V - 1"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    word = torch.randint(0, V, (M,), generator=g)
    word[0] = 0
    word[M - 1] = V - 1
    return dict(M=M, R=R, K=K, V=V, w=rn(4 * R, K) / math.sqrt(K), x=rn(M, K), c_prev=rn(M, R), b_ih=rn(4 * R) * 0.5, b_hh=rn(4 * R) * 0.5,
                gate_bias=rn(M, 4 * R) * 0.5, table=rn(V, 4 * R) * 0.5, word=word)


def lstm_terms(c, b=True, gb=False, tab=False):
    """the additive terms of lstm_ref for a choice of operands"""
    t = []
    if b:
        t += [c["b_ih"], c["b_hh"]]
    if gb:
        t.append(c["gate_bias"])
    if tab:
        t.append(c["table"][c["word"]])
    return t


def linear_case(seed, M, V, K, bias_scale=0.5):
    g = torch.Generator().manual_seed(seed)
    return dict(M=M, V=V, K=K, w=torch.randn(V, K, generator=g) / math.sqrt(K), x=torch.randn(M, K, generator=g),
                b=torch.randn(V, generator=g) * bias_scale)


def negative_vocab_case(seed, M, V, K=64):
    """every real logit negative: bias -5 on every word, weights of scale 0.1 / sqrt(K) (|x w| stays below 1 by a wide margin), so
    a zero row of the padded pack (logit 0, or the clamped bias) would win its block and enter its sum"""
    c = linear_case(seed, M, V, K)
    c["w"] *= 0.1
    c["b"] = torch.full((V,), -5.0)
    return c


# random cases of the merge: (V, seed), M = 64, K = 256, UNK = 1 with bias[UNK] += 3 so that the UNK rule decides many rows.  The
# seeds were chosen on the CPU so that every row's deciding margin is at least 1e-3 (asserted in both test files).
MERGE_CASES = ((300, 6300), (5000, 11000))


def merge_case(V, seed):
    c = linear_case(seed, 64, V, 256)
    c["b"][1] += 3.0
    return c, 1


# where the exact cases plant their ties: (name, V, K, (column a < column b))
#   one wave's share of a block: 32 / NW consecutive columns (8 with 4 waves, 4 with 8) -> columns 0 and 1 of block 1
#   two waves of one block: columns 1 and 9 of block 1 (waves 0 and 2 of 8, 0 and 1 of 4)
#   two blocks: blocks 0 and 2
#   blocks b and b + 256: one thread's stride in top2_final_kernel (WG = 256 threads) -> 257 blocks, V = 8224
TIE_PLACES = (("one_wave", 100, 64, (32, 33)), ("two_waves", 100, 64, (33, 41)), ("two_blocks", 100, 64, (3, 69)),
              ("thread_stride", 8224, 32, (7, 8192 + 3)))


def exact_case(seed, M, V, K, pair, t=None):
    """Integer-valued operands (w in -2..2, x in -1..1, integer bias): every product and every partial sum is an integer below
    2^24 in magnitude, exact in fp32 and in the three-way bf16 split, whatever the order of summation.  Columns a < b of `pair`
    and a third column t (b + 1 unless given) carry equal weight rows, so their logits differ by their biases only, which are planted per
    row scenario (row m runs scenario m % 4) through one extra input column that is 1 on the rows of the scenario:
      0: a and b tie at the row maximum              -> top-1 a, top-2 b
      1: t alone on top, a and b tie for second      -> top-1 t, top-2 a
      2: b alone on top, a second                    -> top-1 b, top-2 a
      3: a, b and t all tie on top                   -> top-1 a, top-2 b
    (a per-row bias does not exist in the linear form: input columns K - 4 .. K - 1 are the one-hot of the scenario and the three
    columns' weights there are the plants; every other output column has weight 0 there)"""
    g = torch.Generator().manual_seed(seed)
    a, b = pair
    t = b + 1 if t is None else t
    assert a < b and t not in (a, b) and max(b, t) < V
    w = torch.randint(-2, 3, (V, K), generator=g).float()
    x = torch.randint(-1, 2, (M, K), generator=g).float()
    bias = torch.randint(-3, 4, (V,), generator=g).float()
    w[b] = w[a]
    w[t] = w[a]
    bias[b] = bias[a]
    bias[t] = bias[a]
    w[:, K - 4:] = 0
    x[:, K - 4:] = 0
    for m in range(M):
        x[m, K - 4 + m % 4] = 1
    # The plant: large enough to put the three columns above every other one (the sort-order assertions of
    # tests/test_packed_gemm_cpu.py check that for the seeds in use), small enough for the log-prob: cvc_top2_final forms
    # v - (mx + log se) in fp32, so its error is half an ulp of the largest logit -- 3e-5 at logits of 1000 (observed on the
    # device: 2.9e-5), 4e-6 below 128.
    big = 64.0
    plants = {0: (big, big, 0), 1: (big, big, big + 1), 2: (big, big + 1, 0), 3: (big, big, big)}
    for s, (pa, pb, pt) in plants.items():
        w[a, K - 4 + s], w[b, K - 4 + s], w[t, K - 4 + s] = pa, pb, pt
    # (value descending, index ascending): with t = b + 1 that is 0: (a, b), 1: (t, a), 2: (b, a), 3: (a, b)
    want = {s: [i for _, i in sorted(((-pa, a), (-pb, b), (-pt, t)))][:2] for s, (pa, pb, pt) in plants.items()}
    top = torch.tensor([want[m % 4] for m in range(M)])
    return dict(M=M, V=V, K=K, w=w, x=x, b=bias, a=a, b_col=b, t=t, top1=top[:, 0], top2=top[:, 1])


# ================================================================== device side
@contextlib.contextmanager
def split_mode(hip, mode):
    """hip.gemm_packed_split is documented as a test hook: set inside try / finally, previous value restored"""
    prev = hip.gemm_packed_split(mode)
    try:
        yield
    finally:
        hip.gemm_packed_split(prev)


def dense_stride(K):
    return (K // 4) * 128                        # floats between the 32-row blocks of a dense pack


class QuadOut:
    """R / 4 quads of an h' / c' destination at quad offset `off` inside a larger NaN buffer (as qoff(XL_r, R) of path_packed.py)"""

    def __init__(self, R, dev, off=0, tail=3):
        self.off, self.nq = off, R // 4
        self.buf = nan_buf(off + self.nq + tail, 64, 4, dev=dev)

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.off * QUAD_BYTES

    def rows(self, M):
        from cvc.decode import from_quad
        return from_quad(self.buf[self.off:self.off + self.nq], M)

    def rest_is_nan(self, M):
        """the quads before and after, and rows >= M of the destination's own quads"""
        return all_nan(self.buf[:self.off]) and all_nan(self.buf[self.off + self.nq:]) and all_nan(self.buf[self.off:self.off + self.nq, M:])


def lstm_operands(c, dev, pad_nan=False):
    """device copies + packs of an lstm_case.  pad_nan: rows >= M of xq and of c_prev_q hold NaN instead of zero"""
    from cvc.decode import pack_weights, to_quad
    o = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in c.items()}
    o["wp"] = pack_weights(o["w"], c["R"])
    o["xq"], o["cq"] = to_quad(o["x"]), to_quad(o["c_prev"])
    if pad_nan:
        o["xq"][:, c["M"]:] = float("nan")
        o["cq"][:, c["M"]:] = float("nan")
    return o


def run_lstm(hip, o, entry="lstm", K=None, b=True, gb=False, tab=False, dst=(True, True), offs=(0, 0), stride=0, w_cached=0, wp=None):
    """One launch of a decode-form entry point on the operands `o` into NaN-filled quad buffers.
    entry: "lstm" | "embgate" | "embgate_ex" | "late" (cvc_packed_lstm_late_fwd, early = NULL).  -> (rc, h1, h2, c_out) QuadOut"""
    L = hip.lib()
    M, R = o["M"], o["R"]
    K = o["K"] if K is None else K
    dev = o["w"].device
    p = lambda t: t.data_ptr()
    h1, h2, co = QuadOut(R, dev, offs[0]), QuadOut(R, dev, offs[1]), QuadOut(R, dev, 0)
    b_ih, b_hh = (p(o["b_ih"]), p(o["b_hh"])) if b else (None, None)
    gbp = p(o["gate_bias"]) if gb else None
    wp = p(o["wp"] if wp is None else wp)
    d1, d2 = h1.ptr if dst[0] else None, h2.ptr if dst[1] else None
    st = stream_handle()
    if entry == "lstm":
        assert not tab
        rc = L.cvc_packed_lstm_fwd(wp, p(o["xq"]), K, b_ih, b_hh, gbp, p(o["cq"]), M, R, d1, d2, co.ptr, st)
    elif entry == "embgate":
        rc = L.cvc_packed_lstm_embgate_fwd(wp, p(o["xq"]), K, b_ih, b_hh, gbp, p(o["table"]), p(o["word"]), p(o["cq"]), M, R, d1, d2, co.ptr, st)
    elif entry == "embgate_ex":
        rc = L.cvc_packed_lstm_embgate_ex_fwd(wp, stride, p(o["xq"]), K, b_ih, b_hh, gbp, p(o["table"]), p(o["word"]), p(o["cq"]), M, R, d1, d2,
                                              co.ptr, w_cached, st)
    else:
        assert entry == "late" and not tab
        rc = L.cvc_packed_lstm_late_fwd(wp, stride, p(o["xq"]), K, b_ih, b_hh, gbp, p(o["cq"]), M, R, d1, d2, co.ptr, None, st)
    torch.cuda.synchronize()
    return rc, h1, h2, co


def check_lstm(tag, outs, ref, M, dst=(True, True)):
    """h' (every destination asked for) and c' against fp64 within OP_TOL; both h' destinations bitwise equal; nothing else
    written: a destination not asked for, the quads around a destination and rows >= M stay NaN.  -> max |err|"""
    h1, h2, co = outs
    err = 0.0
    for name, q, want, asked in (("h_dst1", h1, ref["h"], dst[0]), ("h_dst2", h2, ref["h"], dst[1]), ("c_out", co, ref["c"], True)):
        if not asked:
            assert all_nan(q.buf), (tag, name, "written although its pointer was null")
            continue
        got = q.rows(M)
        assert bool(torch.isfinite(got).all()), (tag, name, "unwritten or non-finite element")
        err = max(err, float((got.double() - want).abs().max()))
        close(got, want.float(), err_msg=f"{tag}: {name}", **OP_TOL)
        assert q.rest_is_nan(M), (tag, name, "wrote outside rows < M of its own quads")
    if dst[0] and dst[1]:
        assert same_bits(h1.rows(M), h2.rows(M)), (tag, "h_dst1 and h_dst2 differ")
    print(f"packed_gemm {tag}: max |err| = {err:.3e}")
    return err


def linear_operands(c, dev, pad_nan=False):
    from cvc.decode import pack_weights, to_quad
    o = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in c.items()}
    o["wp"], o["xq"] = pack_weights(o["w"]), to_quad(o["x"])
    if pad_nan:
        o["xq"][:, c["M"]:] = float("nan")
    return o


def run_linear(hip, o, ksplit=1, ldy=None, want_y=True, want_rec=False, bias=True):
    """cvc_packed_linear_fwd -> (rc, y [ksplit, M, ldy] or None, records [nblk, 64, 6] or None), NaN-filled"""
    L = hip.lib()
    M, V, K = o["M"], o["V"], o["K"]
    dev = o["w"].device
    ldy = V if ldy is None else ldy
    y = nan_buf(ksplit, M, ldy, dev=dev) if want_y else None
    rec = nan_buf((V + 31) // 32, 64, 6, dev=dev) if want_rec else None
    rc = L.cvc_packed_linear_fwd(o["wp"].data_ptr(), o["xq"].data_ptr(), K, o["b"].data_ptr() if bias else None, M, V, ksplit,
                                 None if y is None else y.data_ptr(), ldy, None if rec is None else rec.data_ptr(), stream_handle())
    torch.cuda.synchronize()
    return rc, y, rec


def decode_records(rec, M):
    """device records [nblk, 64, 6] -> the dict layout of block_records ([M, nblk]) for rows < M"""
    r = rec[:, :M].permute(1, 0, 2).contiguous()
    as_int = lambda t: t.contiguous().view(torch.int32).long()
    return dict(v1=r[..., 0], i1=as_int(r[..., 1]), v2=r[..., 2], i2=as_int(r[..., 3]), mx=r[..., 4], se=r[..., 5])


def check_records(tag, rec, y, M, V):
    """the records of a launch against the SAME launch's y [M, >= V]: values bitwise, indices lowest-first, mx == v1, se against
    fp64 within OP_TOL, rows >= M untouched.  -> max |se err|"""
    assert all_nan(rec[:, M:]), (tag, "record rows >= M were written")
    got, want = decode_records(rec, M), block_records(y[:, :V].contiguous())
    for k in ("v1", "v2"):
        if not same_bits(got[k], want[k]):
            d = (got[k].double() - want[k].double()).abs()
            d = d[torch.isfinite(d)]
            raise AssertionError(f"{tag}: record {k} is not bitwise the top of the same launch's y: max |diff| = {float(d.max()) if d.numel() else float('nan'):.3e}")
    for k in ("i1", "i2"):
        assert torch.equal(got[k], want[k]), (tag, k)
    assert same_bits(got["mx"], got["v1"]), (tag, "mx != v1")
    err = float((got["se"].double() - want["se"]).abs().max())
    print(f"packed_gemm {tag}: records se max |err| = {err:.3e}")
    close(got["se"], want["se"].float(), err_msg=f"{tag}: se", **OP_TOL)
    return err


def run_top2_final(hip, dev, rec, nblk, M, unk, word_stride=1, logprob=True, table=None, emb=None, emb_off=2):
    """cvc_top2_final on device records.  emb: None | "quad" (emb_ld = 0, at quad offset emb_off of a larger buffer) | int emb_ld
    (row-major).  -> (rc, word slots [M, word_stride] int64 pre-filled with -7, logprob or None, emb buffer or None)"""
    L = hip.lib()
    word = torch.full((M, word_stride), -7, dtype=torch.int64, device=dev)
    lp = nan_buf(M, dev=dev) if logprob else None
    E = 0 if table is None else table.shape[1]
    ebuf, eptr, eld = None, None, 0
    if emb == "quad":
        ebuf = nan_buf(emb_off + E // 4 + 2, 64, 4, dev=dev)
        eptr = ebuf.data_ptr() + emb_off * QUAD_BYTES
    elif emb is not None:
        ebuf, eld = nan_buf(M + 1, emb, dev=dev), emb
        eptr = ebuf.data_ptr()
    rc = L.cvc_top2_final(rec.data_ptr(), nblk, M, unk, word.data_ptr(), word_stride, None if lp is None else lp.data_ptr(),
                          None if table is None else table.data_ptr(), E, eptr, eld, stream_handle())
    torch.cuda.synchronize()
    return rc, word, lp, ebuf


STEP_OUTS = ("gates_out", "h_out", "h_out2", "h_drop_out", "h_dst1_q", "h_dst2_q")      # the nullable outputs of cvc_lstm_step


def run_step(hip, o, K=None, b=True, gate_pre=False, row_bias=False, row_index=True, outs=STEP_OUTS, rng=None, site=0, p=0.0, M=None,
             offs=(2, 1), w_cached=0):
    """cvc_packed_lstm_step_fwd with a cvc.hip.LstmStep filled field by field; c_prev row-major.  row_bias: the table of the case
    gathered by its word vector (which has repeats).  -> (rc, dict of outputs: row-major [M, *] tensors and QuadOut objects)"""
    L = hip.lib()
    R = o["R"]
    M = o["M"] if M is None else M
    K = o["K"] if K is None else K
    dev = o["w"].device
    Mb = min(M, o["M"])
    res = dict(c_out=nan_buf(Mb + 1, R, dev=dev), gates_out=nan_buf(Mb + 1, 4 * R, dev=dev), h_out=nan_buf(Mb + 1, R, dev=dev),
               h_out2=nan_buf(Mb + 1, R, dev=dev), h_drop_out=nan_buf(Mb + 1, R, dev=dev), h_dst1_q=QuadOut(R, dev, offs[0]),
               h_dst2_q=QuadOut(R, dev, offs[1]))
    s = hip.LstmStep()
    s.wp, s.xq, s.K, s.M, s.R = o["wp"].data_ptr(), o["xq"].data_ptr(), K, M, R
    s.b_ih, s.b_hh = (o["b_ih"].data_ptr(), o["b_hh"].data_ptr()) if b else (None, None)
    s.gate_pre = o["gate_bias"].data_ptr() if gate_pre else None
    s.row_bias = o["table"].data_ptr() if row_bias else None
    s.row_index = o["word"].data_ptr() if (row_bias and row_index) else None
    s.c_prev = o["c_prev"].data_ptr()
    s.c_out = res["c_out"].data_ptr()
    for name in STEP_OUTS:
        t = res[name]
        setattr(s, name, (t.ptr if isinstance(t, QuadOut) else t.data_ptr()) if name in outs else None)
    s.rng_state = None if rng is None else rng.data_ptr()
    s.site, s.p = site, p
    s.w_cached = w_cached
    rc = L.cvc_packed_lstm_step_fwd(s, stream_handle())
    torch.cuda.synchronize()
    return rc, res
