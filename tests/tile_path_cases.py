"""Shared pieces of tests/test_gpu_tile_path.py and tests/test_tile_path_cpu.py (not collected: no test_ prefix): the case tables
and host references of the decode engine's TILE path (csrc/gemm_tile.hip: cvc_tile_gemm, cvc_tile_linear_finish,
cvc_tile_lstm_finish(_embgate), cvc_tile_reorder_pack, cvc_tile_pack_rows(_any), cvc_tile_pack_cols) and of the beam bookkeeping
(csrc/beam.hip: cvc_beam_select(_parts), cvc_beam_backtrack, cvc_gather_rows).

Everything here runs on the CPU.  The arithmetic that sends a size to a branch of the source (chunk height MH, K-slice length,
XCD remap, form switch, NG / NP instantiation) is restated as small functions; tests/test_tile_path_cpu.py checks the tables
against them and the constants against the sources."""
import math
import os
import re

import torch

from attn_step_cases import all_nan, bits, close, nan_buf, same_bits, stream_handle  # noqa: F401  (re-exported to the tests)

OP_TOL = dict(rtol=2e-5, atol=2e-5)              # tests/test_gpu_parity.py
SCORE_TOL = dict(rtol=1e-5, atol=1e-5)           # test_beam_bookkeeping_ops_vs_bruteforce
E_BADARG = -1                                    # include/cvc_hip.h
FILL16 = 0x7FC0                                  # a bf16 NaN: the fill of every fragment buffer
KSTEP = 3 * 512                                  # bf16 elements of one (32-row block, k step): three term fragments of 512
GAP = 1e-3                                       # two beam candidates are exactly tied by construction or at least this far apart
# constants of the sources the tables below are built on (source_constants() reads them; the CPU test compares)
BEAM_MAX, ROW_CACHE, WG, WIDE_KSTEPS, FRAG = 8, 32, 256, 64, 512


def source_constants():
    """BEAM_MAX, ROW_CACHE of csrc/beam.hip and the WG it takes from csrc/row_block.h; FRAG and the k steps per workgroup from which
    the default form of cvc_tile_gemm is the wide one, of csrc/gemm_tile.hip"""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cyclical-visual-captioning_amd", "csrc")
    beam, blk, til = (open(os.path.join(csrc, f)).read() for f in ("beam.hip", "row_block.h", "gemm_tile.hip"))
    assert '#include "row_block.h"' in beam and not re.search(r"constexpr\s+int\s+WG\b", beam)      # no WG of its own
    ci = lambda src, name: int(re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)", src).group(1))
    wide = re.search(r"cvc_tile_loader_waves == 3 && a\.ksteps / ksplit >= (\d+)", til)
    return dict(BEAM_MAX=ci(beam, "BEAM_MAX"), ROW_CACHE=ci(beam, "ROW_CACHE"), WG=ci(blk, "WG"), FRAG=ci(til, "FRAG"),
                WIDE_KSTEPS=int(wide.group(1)))


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------ fragments (include/cvc_hip.h, "Tile path")
def bf16_bits(v):
    """the upper 16 bits of fp32 values, as int16"""
    return (v.contiguous().view(torch.int32) >> 16).to(torch.int16)


def split3(x):
    """fp32 [..] -> int16 [3, ..]: the bf16 terms hi, mid, lo of the split-product arithmetic (truncation; csrc/gemm_tile.hip::split3)"""
    top = lambda v: (v.contiguous().view(torch.int32) & -65536).view(torch.float32)
    hi = top(x)
    r1 = x - hi
    mid = top(r1)
    return torch.stack([bf16_bits(hi), bf16_bits(mid), bf16_bits(r1 - mid)], 0)


def planes_to_frag(planes):
    """[3, rows, K] int16 (rows % 32 == 0, K % 16 == 0) -> [rows / 32][K / 16][3][2 k halves][32 rows][8 k]: the to_frag permutation,
    applied to each term plane"""
    _, ra, k = planes.shape
    assert ra % 32 == 0 and k % 16 == 0
    return planes.view(3, ra // 32, 32, k // 16, 2, 8).permute(1, 3, 0, 4, 2, 5).contiguous()


def frag_to_planes(xb):
    """inverse of planes_to_frag -> [3, rows, K]"""
    nb, ks = xb.shape[0], xb.shape[1]
    return xb.permute(2, 0, 4, 1, 3, 5).reshape(3, nb * 32, ks * 16)


def fill_planes(rows, K, device="cpu"):
    return torch.full((3, rows, K), FILL16, dtype=torch.int16, device=device)


def rows_alloc(M):
    """cvc_tile_rows_alloc restated: rows an activation buffer must hold for ANY chunk height the GEMM may pick"""
    mblk = (M + 31) // 32
    if mblk <= 10:
        return 2 * (5 if mblk == 10 else (mblk + 1) // 2) * 32
    return max((mblk + 2 * mh - 1) // (2 * mh) * 2 * mh * 32 for mh in (3, 4, 5))


# ------------------------------------------------------------------ 1. cvc_tile_gemm: which branch a size takes
def chunk_mh(M):
    """accumulator tiles per wave (MH) for up to 320 rows: (mblk + 1) / 2, 5 at ten blocks; None above (device-dependent)"""
    mblk = (M + 31) // 32
    return (mblk + 1) // 2 if mblk < 10 else (5 if mblk == 10 else None)


def slice_range(ksteps, s, ksplit):
    return ksteps * s // ksplit, ksteps * (s + 1) // ksplit


def slice_lengths(K, ksplit):
    return [b - a for a, b in (slice_range(K // 16, s, ksplit) for s in range(ksplit))]


def xcd_remap(N, ksplit):
    ntile = (N + 127) // 128
    return ksplit > 1 and ksplit <= 8 and 8 % ksplit == 0 and ntile % (8 // ksplit) == 0


def wide_form(K, ksplit):
    """does the default setting (3) take the 4-wide-wave form?"""
    return (K // 16) // ksplit >= WIDE_KSTEPS


def big_form(M, N):
    return M % 256 == 0 and N % 256 == 0 and M >= 512


# (M, N, K, ksplit): the census cases.  Slice lengths in k steps, MH and the remap stand beside each.
CENSUS = [
    (1, 1, 16, 1),          # MH 1; one k step: prologue of one copy
    (33, 50, 32, 2),        # MH 1; slices 1 + 1; ksplit 2 with ntile 1 (1 % 4 != 0): no remap
    (64, 128, 32, 1),       # MH 1; slice 2: the prologue only, no copy from inside the loop
    (65, 130, 48, 1),       # MH 2; slice 3: the first copy issued from inside the loop; two weight tiles, the second with 2 columns
    (129, 384, 64, 1),      # MH 3; slice 4
    (161, 50, 80, 1),       # MH 3; slice 5
    (200, 130, 112, 1),     # MH 4 (7 blocks); slice 7
    (250, 512, 400, 2),     # MH 4 (8 blocks: 50 clips x beam 5); 25 k steps in 12 + 13; ksplit 2, ntile 4: remap
    (257, 256, 176, 3),     # MH 5 (9 blocks); 11 k steps in 3 + 4 + 4; ksplit 3: no remap
    (320, 256, 256, 4),     # MH 5 (10 blocks); ksplit 4, ntile 2: remap; slices of 4
    (250, 130, 256, 8),     # ksplit 8: remap with any N; slices of 2
    (129, 50, 240, 5),      # ksplit 5: no remap; slices of 3
    (65, 384, 192, 6),      # ksplit 6: no remap; slices of 2
    (33, 128, 256, 16),     # ksplit 16: no remap; slices of 1
    (161, 128, 128, 4),     # ksplit 4 with ntile 1 (1 % 2 != 0): no remap
    (64, 256, 64, 2),       # ksplit 2 with ntile 2 (2 % 4 != 0): no remap
    (352, 130, 64, 2),      # 11 row blocks: two row chunks, dead row blocks in the last
    (640, 384, 48, 1),      # 20 row blocks: chunk height from the plan
    (200, 128, 1024, 1),    # 64 k steps per workgroup: the wide form by default
    (65, 256, 2048, 2),     # 128 k steps in two slices of 64: wide
    (129, 1, 1008, 1),      # 63 k steps: stays on the 8-wave form
    (512, 256, 96, 2),      # whole 256 x 256 tiles: also the big form
    (512, 512, 64, 1),
]
# (M, N, K, ksplit) of the real-valued family (through the packers)
REAL = [(65, 50, 48, 1), (250, 384, 512, 3), (129, 130, 1024, 1), (320, 512, 2048, 2), (640, 256, 256, 2)]


def census_case(seed, M, N, K):
    """the three term planes of both operands as independent integers in [-7, 7] (exact in bf16): X [3, M, K], W [3, N, K] fp32"""
    g = gen(seed)
    return torch.randint(-7, 8, (3, M, K), generator=g).float(), torch.randint(-7, 8, (3, N, K), generator=g).float()


def census_ref(X, W, ksplit):
    """slab s = sum over p + q <= 2 of X_p[:, k range(s)] W_q[:, k range(s)]^T, fp64 [ksplit, M, N] (integers: exact)"""
    ksteps = X.shape[2] // 16
    out = []
    for s in range(ksplit):
        a, b = (16 * v for v in slice_range(ksteps, s, ksplit))
        acc = 0
        for p in range(3):
            for q in range(3 - p):
                acc = acc + X[p][:, a:b].double() @ W[q][:, a:b].double().t()
        out.append(acc)
    return torch.stack(out)


def census_frags(X, W):
    """-> (xb, wb) int16 fragments: activation rows [M, rows_alloc(M)) hold NaN patterns, weight rows beyond N are zero"""
    _, M, K = X.shape
    N = W.shape[1]
    xp = fill_planes(rows_alloc(M), K, X.device)
    xp[:, :M] = bf16_bits(X)
    wp = torch.zeros(3, (N + 127) // 128 * 128, K, dtype=torch.int16, device=W.device)
    wp[:, :N] = bf16_bits(W)
    return planes_to_frag(xp), planes_to_frag(wp)


def real_case(seed, M, N, K):
    g = gen(seed)
    x = torch.randn(M, K, generator=g) * torch.exp2(torch.randint(-6, 4, (M, 1), generator=g).float())
    return x, torch.randn(N, K, generator=g) / K ** 0.5


def ordered_sum(parts, *terms):
    """((p0 + p1) + ...) + term + ...: fp32, in that order (terms that are None are skipped)"""
    s = parts[0].clone()
    for p in parts[1:]:
        s = s + p
    for t in terms:
        if t is not None:
            s = s + t
    return s


# ------------------------------------------------------------------ 2. finishing kernels
LIN_NPARTS = (1, 2, 3, 4, 5, 6, 7, 8, 16, 17)      # templates 1, 2, 4, 6, 8, 16 and the loop
LIN_N = (1, 255, 256, 257, 513)
LIN_M = (1, 321)


def linear_cases():
    out = []
    for i, nparts in enumerate(LIN_NPARTS):
        for j, N in enumerate(LIN_N):
            t = i + j
            out.append(dict(nparts=nparts, N=N, M=LIN_M[t % 2], ld=N + (3 if t % 3 == 0 else 0), ldy=N + (5 if t % 3 == 1 else 0),
                            bias=bool(t & 1), bias2=bool(t & 2), seed=3000 + 10 * i + j))
    return out


def linear_inputs(c):
    g = gen(c["seed"])
    parts = torch.randn(c["nparts"], c["M"], c["ld"], generator=g)
    bias = torch.randn(c["N"], generator=g) if c["bias"] else None
    bias2 = torch.randn(c["N"], generator=g) if c["bias2"] else None
    return parts, bias, bias2


# (nparts, R, M, gb_div): <1> <2> <4> <8> and the loop <0> (3, 5, 6, 16) of tile_lstm_finish_kernel
LSTM_CASES = [(1, 16, 1, 1), (2, 48, 31, 5), (4, 64, 32, 1), (8, 256, 33, 5), (3, 16, 70, 5), (5, 48, 320, 1), (6, 64, 70, 1),
              (16, 16, 33, 5), (8, 64, 320, 5), (1, 256, 70, 5), (2, 16, 32, 1), (3, 48, 1, 1)]
LSTM_NULLABLE = ("b_ih", "b_hh", "gate_bias", "h_out", "frag1", "frag2")
LSTM_V = 23


def lstm_inputs(seed, nparts, R, M, gb_div, saturated=False):
    """parts [nparts, M, 4R] in the packed feature order (blk * 32 + gate * 8 + unit), everything else in checkpoint order"""
    g = gen(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    c = dict(nparts=nparts, R=R, M=M, gb_div=gb_div, parts=rn(nparts, M, 4 * R) * (0.7 / math.sqrt(nparts)), b_ih=rn(4 * R) * 0.2,
             b_hh=rn(4 * R) * 0.2, gate_bias=rn((M + gb_div - 1) // gb_div, 4 * R) * 0.3, c_prev=rn(M, R),
             emb_gate=rn(LSTM_V, 4 * R) * 0.4, word=torch.randint(0, LSTM_V, (M,), generator=g))
    # words outside [0, V) read row 0
    for m, w in zip(range(0, M, 3), (-1, LSTM_V, LSTM_V + 5, 0, LSTM_V - 1)):
        c["word"][m] = w
    if saturated:
        # pre-activations of +-30 / +-100 (slab 0 carries them, the other slabs and terms are zero) and cell states of +-1e4
        lv = torch.tensor([30.0, -30.0, 100.0, -100.0])
        c["parts"].zero_()
        c["parts"][0] = lv[torch.randint(0, 4, (M, 4 * R), generator=g)]
        for k in ("b_ih", "b_hh", "gate_bias", "emb_gate"):
            c[k].zero_()
        c["c_prev"] = torch.where(torch.rand(M, R, generator=g) < 0.5, 1e4, -1e4) * torch.ones(M, R)
    return c


def unpack_gates(pre_packed, R):
    """[M, 4R] packed feature order -> checkpoint order gate * R + hidden"""
    M = pre_packed.shape[0]
    return pre_packed.view(M, R // 8, 4, 8).permute(0, 2, 1, 3).reshape(M, 4 * R)


def lstm_finish_ref(c, emb, null=None):
    """fp64 -> (c', h') [M, R]"""
    M, R = c["M"], c["R"]
    pre = unpack_gates(c["parts"].double().sum(0), R)
    if null != "b_ih":
        pre = pre + c["b_ih"].double()
    if null != "b_hh":
        pre = pre + c["b_hh"].double()
    if null != "gate_bias":
        pre = pre + c["gate_bias"].double()[torch.arange(M) // c["gb_div"]]
    if emb:
        w = c["word"].clone()
        w[(w < 0) | (w >= LSTM_V)] = 0
        pre = pre + c["emb_gate"].double()[w]
    i, f, g, o = pre.chunk(4, 1)
    cn = torch.sigmoid(f) * c["c_prev"].double() + torch.sigmoid(i) * torch.tanh(g)
    return cn, torch.sigmoid(o) * torch.tanh(cn)


# ------------------------------------------------------------------ 3. packers and the beam-state reorder
# (E, parent given, beam, rows, R); rows is a multiple of beam (rows = clips x beam)
REORDER_CASES = [(0, True, 8, 320, 16), (0, False, 1, 1, 48), (16, True, 3, 33, 48), (32, True, 5, 70, 16), (0, True, 5, 70, 256),
                 (16, False, 5, 320, 48), (32, True, 1, 33, 256), (0, True, 3, 33, 16)]
REORDER_V = 19
PACK_ROWS_CASES = [(1, 16, 16, 0), (33, 48, 52, 1), (70, 64, 64, 2), (321, 32, 36, 0)]        # (M, K, ldx, k step offset)
PACK_ANY_BLK = [(1, 16, 16), (33, 48, 52), (70, 64, 64), (321, 32, 36)]                         # (M, K, ldx): K % 16 == 0, ldx % 4 == 0
PACK_ANY_SCALAR = [(1, 1, 1, 0), (33, 5, 7, 0), (70, 17, 17, 0), (321, 37, 41, 0), (33, 48, 51, 0), (70, 32, 32, 1)]   # (M, K, ldx, floats off)
PACK_COLS_S = (1, 15, 16, 17, 70)
PACK_COLS_C = (1, 31, 33, 130)


def reorder_inputs(seed, E, with_parent, beam, rows, R):
    g = gen(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    c = dict(E=E, beam=beam, rows=rows, R=R, h_att=rn(rows, R), c_att=rn(rows, R), h_lang=rn(rows, R), c_lang=rn(rows, R),
             table=rn(REORDER_V, E) if E else None, word=torch.randint(0, REORDER_V, (rows,), generator=g),
             parent=torch.randint(0, beam, (rows,), generator=g) if with_parent else None)
    for m, w in zip(range(0, rows, 2), (-1, REORDER_V, REORDER_V + 5, -2 ** 40)):
        c["word"][m] = w
    return c


def reorder_ref(c):
    """-> (xa [rows, 2R + E], h_lang[src], c_att[src], c_lang[src]) fp32, exact copies"""
    rows, beam = c["rows"], c["beam"]
    src = torch.arange(rows) if c["parent"] is None else (torch.arange(rows) // beam) * beam + c["parent"]
    segs = [c["h_lang"][src]]
    if c["E"]:
        w = c["word"].clone()
        w[(w < 0) | (w >= REORDER_V)] = 0
        segs.append(torch.relu(c["table"][w]))
    segs.append(c["h_att"][src])
    return torch.cat(segs, 1), c["h_lang"][src], c["c_att"][src], c["c_lang"][src]


# ------------------------------------------------------------------ 4. beam bookkeeping
def ng_of(V):
    """float4 groups per thread of beam_rowtop4_kernel"""
    return min((V + 4 * WG - 1) // (4 * WG), 8)


def fast_form(c):
    """does cvc_beam_select_parts take the float4 scan for this case?  (c['shift']: the logits start one float off alignment)"""
    aligned = c["V"] % 4 == 0 and not c.get("shift")
    slabs = aligned and c["nparts"] in (2, 4, 6, 8) and c["part_stride"] % 4 == 0 and not c.get("bias_shift")
    return (aligned and c["nparts"] == 1 and not c["bias"]) or slabs


def row_lse(x):
    """log-sum-exp of every row, fp64, with -inf entries"""
    m = x.max(1, keepdim=True).values
    return (m + torch.log(torch.exp(x - m).sum(1, keepdim=True))).view(-1)


def candidates(c):
    """[B, beam, V] fp64: score + log-softmax, UNK at -inf, a frozen row offers (k, 0) at its carried score, first step: row 0 only"""
    B, beam, V = c["B"], c["beam"], c["V"]
    x = c["logits"].double()
    cand = c["score"].double().view(-1, 1) + (x - row_lse(x).view(-1, 1))
    cand[:, c["unk"]] = -math.inf
    frozen = torch.full_like(cand, -math.inf)
    frozen[:, 0] = c["score"].double()
    cand = torch.where(c["done"].bool().view(-1, 1), frozen, cand).view(B, beam, V)
    if c["first"]:
        cand[:, 1:] = -math.inf
    return cand


def beam_ref(c):
    """full scan in fp64, stable sort over the flat (k, v) index -> dict(parent, word, score [B, beam], done, live)"""
    B, beam, V = c["B"], c["beam"], c["V"]
    v, i = torch.sort(candidates(c).view(B, beam * V), dim=1, descending=True, stable=True)
    v, i = v[:, :beam], i[:, :beam]
    parent, word = i // V, i % V
    done = c["done"].bool().view(B, beam).gather(1, parent) | (word == 0)
    return dict(parent=parent, word=word, score=v, done=done, live=torch.isfinite(v))


def gap_violations(c, every_pair=True):
    """Pairs of candidates of one clip that are neither at least GAP apart nor exactly tied by construction (the same row with
    equal logits; rows with identical logits and equal scores; a frozen row against a live candidate).  every_pair False: only
    among the best beam + 1 (the random-logit cases)."""
    B, beam, V = c["B"], c["beam"], c["V"]
    cand = candidates(c)
    bad = []
    for b in range(B):
        if not every_pair:
            v = torch.sort(cand[b].view(-1), descending=True).values[:beam + 1]
            v = v[torch.isfinite(v)]
            if bool(((v[:-1] - v[1:]) < GAP).any()):
                bad.append((b, "top"))
            continue
        vals, rows = [], []
        for k in range(beam):
            u = torch.unique(cand[b, k][torch.isfinite(cand[b, k])])
            vals.append(u)
            rows.append(torch.full_like(u, k, dtype=torch.int64))
        vals, rows = torch.cat(vals), torch.cat(rows)
        order = torch.argsort(vals)
        vals, rows = vals[order], rows[order]
        d = vals[1:] - vals[:-1]
        if bool(((d > 0) & (d < GAP)).any()):
            bad.append((b, "close"))
        for j in torch.nonzero(d == 0).view(-1).tolist():        # equal values of two rows (unique() removed those inside a row)
            k1, k2 = b * beam + int(rows[j]), b * beam + int(rows[j + 1])
            frozen = bool(c["done"][k1]) or bool(c["done"][k2])
            twins = torch.equal(c["logits"][k1], c["logits"][k2]) and float(c["score"][k1]) == float(c["score"][k2])
            if not (frozen or twins):
                bad.append((b, "tie"))
    return bad


def beam_case(name, B, beam, V, seed, plant=(), value=6.0, unk=1, first=False, nparts=1, bias=False, frozen=0.0, stride_pad=0,
              bias_shift=False, special=None, random_logits=False):
    """One beam-selection case.  Integer logits in [-8, 0] with `value` planted at the columns `plant` of every row; a live row's
    score is lse - 0.37 * rank - small integer with the ranks a permutation of the clip's rows, so candidates of different rows differ
    by a multiple of 0.37 plus an integer (>= 0.11 from a tie); a frozen row carries integer + 0.32 + 0.003 k."""
    g = gen(seed)
    rows = B * beam
    if random_logits:
        logits = torch.randn(rows, V, generator=g) * 2
    else:
        logits = torch.randint(-8, 1, (rows, V), generator=g).float()
        for p in plant:
            logits[:, p % V] = value
    done = torch.zeros(rows, dtype=torch.uint8)
    if frozen > 0 and not first:
        done = (torch.rand(rows, generator=g) < frozen).to(torch.uint8)
    rank = torch.argsort(torch.rand(B, beam, generator=g), 1).view(-1).double()
    score = None
    kk = torch.arange(rows) % beam
    if special == "twins" and beam > 1:                      # rows 0 and 1 of every clip identical, equal scores, the best two ranks
        logits.view(B, beam, V)[:, 1] = logits.view(B, beam, V)[:, 0]
        rank = rank.view(B, beam)
        rank[:, 2:] = torch.argsort(torch.rand(B, beam - 2, generator=g), 1).double() + 1
        rank[:, :2] = 0
        rank = rank.view(-1)
    if special == "neg_inf":                                  # fewer finite candidates than beam: two finite logits per row,
        keep = logits[:, [3, V - 2]].clone()                  # only rows 0 (and 1 when not the first step) carry a finite score
        logits[:] = -math.inf
        logits[:, 3], logits[:, V - 2] = keep[:, 0], keep[:, 1] + 1
    lse = row_lse(logits.double())
    if random_logits:
        score = torch.randn(rows, generator=g)
    else:
        score = (lse - 0.37 * rank - torch.randint(0, 3, (rows,), generator=g).double()).float()
        fz = (value - 1 - torch.randint(0, 4, (rows,), generator=g).double() + 0.32 + 0.003 * kk.double()).float()
        score = torch.where(done.bool(), fz, score)
    if special == "twins" and beam > 1:                      # ... and no integer below the lse: the twins lead the clip
        score.view(B, beam)[:, 0] = lse.view(B, beam)[:, 0].float()
        score.view(B, beam)[:, 1] = score.view(B, beam)[:, 0]
    if special == "all_done":
        done[:] = 1
        score = (0.32 + 0.003 * kk.double() - torch.argsort(torch.rand(B, beam, generator=g), 1).view(-1).double()).float()
    if special == "neg_inf" and not first:
        score[kk >= min(2, beam - 1)] = -math.inf
    if special in ("frozen_first", "live_first") and beam > 1:
        # a frozen row's carried score against a live candidate of EQUAL value: the live row is peaked (one 0, the rest <= -200:
        # its lse is exactly 0 in fp32 and fp64), both carry 7.5, above every other candidate of the clip
        lv, fr = (1, 0) if special == "frozen_first" else (0, 1)
        lg = logits.view(B, beam, V)
        lg[:, lv] = -200.0 - torch.randint(0, 50, (B, V), generator=g).float()
        lg[:, lv, V // 2] = 0.0
        done.view(B, beam)[:, fr] = 1
        done.view(B, beam)[:, lv] = 0
        score.view(B, beam)[:, lv] = 7.5
        score.view(B, beam)[:, fr] = 7.5
    if first:
        score[kk > 0] += 100.0                                 # rows k > 0 carry larger scores and must be ignored
    c = dict(name=name, B=B, beam=beam, V=V, unk=unk, first=first, nparts=nparts, bias=bias or bias_shift, logits=logits, score=score,
             done=done, part_stride=rows * V + stride_pad, bias_shift=bias_shift, exact=not random_logits)
    # the slabs: integer pieces whose sum is the logits in any order (random logits: the logits ARE the ordered fp32 sum)
    if nparts > 1 or c["bias"]:
        finite = torch.where(torch.isfinite(logits), logits, torch.zeros_like(logits))
        if random_logits:
            parts = torch.randn(nparts, rows, V, generator=g)
            b = torch.randn(V, generator=g) if c["bias"] else None
            c["logits"] = ordered_sum(parts, b)
        else:
            parts = torch.randint(-5, 6, (nparts, rows, V), generator=g).float()
            b = torch.randint(-5, 6, (V,), generator=g).float() if c["bias"] else None
            parts[0] = finite - (parts[1:].sum(0) + (b if b is not None else 0.0))
            parts[0][~torch.isfinite(logits)] = -math.inf
            assert torch.equal(ordered_sum(parts, b), logits)
        c["parts"], c["bias_v"] = parts, b
    else:
        c["parts"], c["bias_v"] = logits.view(1, rows, V), None
    return c


# where a tie for a row's maximum sits in the row scan: thread tid holds elements (tid + 256 g) * 4 + e of group g, in the float4
# form and in the general form alike; lane = tid & 63, wave = tid >> 6
TIE_PLACES = {
    "float4": (8, 9),                   # one thread's float4
    "lanes": (12, 160),                 # threads 3 and 40 of wave 0
    "waves": (20, 280),                 # threads 5 (wave 0) and 70 (wave 1)
    "groups": (40, 1064),               # v and v + 1024: groups 0 and 1 of thread 10
    "ends": (0, -1),                    # indices 0 and V - 1 (word 0 also ends a hypothesis: done_out)
    "rowcache": (5, 261),               # 256 apart: threads 1 (wave 0) and 65 (wave 1), elements 1 of their float4
    "many": (3, 7, 300, 1030, 1500, 2000, 2049, 2051, 90, 600, 1200),       # more tied values than beam
}
FAST_SWEEP = [(8, 1, 5, 3), (1024, 2, 2, 64), (1028, 4, 5, 3), (2048, 6, 8, 1), (2052, 8, 1, 3), (3072, 1, 5, 3), (4096, 2, 8, 3),
              (5000, 6, 5, 64), (5120, 4, 2, 1), (6144, 8, 5, 3), (7168, 1, 8, 1), (8192, 8, 8, 3)]          # (V, nparts, beam, B)
GENERAL_SWEEP = [(9, 1, 1, 3), (50, 3, 2, 64), (1025, 5, 5, 3), (5001, 7, 8, 1), (8191, 1, 5, 3), (1024, 3, 2, 3)]


def beam_specs():
    """(name, positional arguments of beam_case, keyword arguments): cheap to list, built on demand by shared_beam_case()"""
    cs = []
    add = lambda name, B, beam, V, seed, **kw: cs.append((name, (name, B, beam, V, seed), kw))
    for i, (place, cols) in enumerate(TIE_PLACES.items()):
        add("tie_" + place, 3, (2, 5, 8, 5, 2, 5, 8)[i], 2052, 100 + i, plant=cols)
    add("unk_unique_max", 3, 5, 2052, 120, plant=(1,), value=9.0)
    add("unk_tied_max", 3, 5, 2052, 121, plant=(1, 2, 1500))
    add("twins", 3, 5, 1028, 122, plant=(17, 600), special="twins")
    add("twins_beam2", 64, 2, 8, 123, plant=(5,), special="twins")
    add("frozen_first", 3, 5, 1028, 124, plant=(17,), special="frozen_first")
    add("live_first", 3, 5, 1028, 125, plant=(17,), special="live_first")
    add("frozen_mix", 64, 5, 1024, 126, plant=(0, 900), frozen=0.4)
    add("first_step", 3, 8, 2052, 127, plant=(30, 31), first=True)
    add("first_step_beam1", 1, 1, 8, 128, plant=(4,), first=True)
    add("all_done", 3, 5, 1028, 129, special="all_done")
    add("neg_inf_first", 3, 5, 1028, 130, special="neg_inf", first=True)
    add("neg_inf", 3, 5, 1028, 131, special="neg_inf")
    for i, (V, nparts, beam, B) in enumerate(FAST_SWEEP):
        add(f"fast_V{V}_np{nparts}", B, beam, V, 200 + i, plant=(V // 3, -1), nparts=nparts, bias=nparts > 1, frozen=0.2 if i % 2 else 0.0)
    for i, (V, nparts, beam, B) in enumerate(GENERAL_SWEEP):
        add(f"general_V{V}_np{nparts}", B, beam, V, 300 + i, plant=(V // 3, -1), nparts=nparts, bias=nparts > 1,
            frozen=0.2 if i % 2 else 0.0)
    # an aligned V that still falls back: a slab stride that is no multiple of 4, a bias 4 bytes off alignment
    add("fallback_stride", 3, 5, 1024, 320, plant=(100, 1023), nparts=2, bias=True, stride_pad=2)
    add("fallback_bias", 3, 5, 2048, 321, plant=(100, 2047), nparts=4, bias_shift=True)
    # (the seeds of the random-logit cases are chosen so that the best beam + 1 of every clip are >= GAP apart; the CPU test asserts it)
    add("random_engine_shape", 64, 5, 5000, 333, nparts=6, bias=True, frozen=0.2, random_logits=True)
    add("random_general", 3, 8, 97, 331, frozen=0.2, random_logits=True)
    return cs


BEAM_SPECS = beam_specs()
BEAM_NAMES = [n for n, _, _ in BEAM_SPECS]
_BEAM_CACHE = {}


def shared_beam_case(name):
    """the case and its reference, computed once per process and left unchanged"""
    if name not in _BEAM_CACHE:
        _, args, kw = next(s for s in BEAM_SPECS if s[0] == name)
        c = beam_case(*args, **kw)
        c["ref"] = beam_ref(c)
        _BEAM_CACHE[name] = c
    return _BEAM_CACHE[name]


def brute_force(c):
    """exhaustive enumeration in python (micro cases): every (k, v) with its value, best first, ties to the lowest flat index"""
    cand = candidates(c)
    B, beam, V = c["B"], c["beam"], c["V"]
    out = []
    for b in range(B):
        flat = [(float(cand[b, k, v]), k * V + v) for k in range(beam) for v in range(V)]
        flat.sort(key=lambda t: (-t[0], t[1]))
        out.append(flat[:beam])
    return out


BACKTRACK_CASES = [(1, 1, 1, 1), (3, 5, 2, 7), (64, 8, 20, 100), (3, 5, 256, 257), (1, 8, 256, 1), (64, 1, 2, 7)]     # (B, beam, T, N)
GATHER_CASES = [(4, 1), (64, 5), (1024, 8), (1028, 5), (2052, 8)]                                                        # (width, beam)


def backtrack_inputs(seed, B, beam, T, N):
    g = gen(seed)
    rows = B * beam
    parent = torch.randint(0, beam, (T, rows), generator=g)
    for b in range(B):                                    # parents outside [0, beam) ON the rank-0 path: clamped to the nearest slot
        parent[T - 1, b * beam] = (-1, beam, beam + 7, -5, 0)[b % 5]
    return dict(B=B, beam=beam, T=T, N=N, words=torch.randint(0, 5000, (T, rows), generator=g), parent=parent,
                att=torch.randn(T, rows, N, generator=g))


def backtrack_ref(c):
    """host indexing: the rank-0 hypothesis of every clip, walked back from the last step; the attention row of step t is the
    PARENT row's"""
    B, beam, T, N = c["B"], c["beam"], c["T"], c["N"]
    seq = torch.empty(B, T, dtype=torch.int64)
    att = torch.empty(B, T, N)
    for b in range(B):
        k = 0
        for t in range(T - 1, -1, -1):
            seq[b, t] = c["words"][t, b * beam + k]
            kp = min(max(int(c["parent"][t, b * beam + k]), 0), beam - 1)
            att[b, t] = c["att"][t, b * beam + kp]
            k = kp
    return seq, att
