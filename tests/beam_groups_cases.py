"""The block cases of diverse (group) beam search, shared by tests/test_beam_groups_cpu.py (which checks on the fp64 reference that
they can be compared exactly) and tests/test_gpu_beam_groups.py (which runs them): integer-logit cases of
tile_path_cases.beam_case with planted histories and 40 % frozen rows."""
import functools

import numpy as np
import torch

import tile_path_cases as T
import beam_groups_ref as GR

T_HIST = 65                                   # steps a history buffer holds: t <= 64 writes step t
# (V, nparts, bias, planted columns): V = 8 with five words banned (fewer finite candidates than bd in a group), the general scan,
# the float4 scan, the engine's shape (6 slabs + bias)
SHAPES = [(8, 1, False, (6,)), (50, 3, True, (0, 16, 49)), (1028, 1, False, (0, 30, 700, 1027)), (5000, 6, True, (0, 1666, 4999))]
GROUPINGS = [(6, 1), (6, 2), (6, 3), (6, 6), (8, 4)]          # (beam, G)
# (shape, beam, G): every pair but V = 8 with beam 8 -- the selection blocks need V >= beam + 1
BLOCK_CASES = [(si, beam, groups) for si in range(len(SHAPES)) for beam, groups in GROUPINGS if SHAPES[si][0] >= beam + 1]
B = 3
NGRAM = 2
STEPS = (0, 1, NGRAM, 63)
# The case's values lie on a grid: candidates of one row differ by integers, those of different live rows by 0.37 * (rank
# difference) + an integer, a frozen row carries integer + 0.32 + 0.003 k.  lambda = 0.7 (its fp32 value) times a count of at most 7
# is never an integer, so a penalised candidate ties with nothing by arithmetic, and it keeps every pair of the grid >= GAP apart:
# the smallest gap stays the 0.003 between two frozen rows (0.3 would bring a live candidate within 0.001 of a frozen one).  The
# CPU test checks both on the augmented values of every case.
LAMBDA = 0.7


@functools.lru_cache(maxsize=None)
def base_case(si, beam, first):
    V, nparts, bias, plant = SHAPES[si]
    return T.beam_case(f"groups{si}_{beam}", B, beam, V, 1700 + 10 * si + beam, plant=plant, first=first, nparts=nparts, bias=bias,
                       frozen=0.0 if first else 0.4)


@functools.lru_cache(maxsize=None)
def planted_history(si, beam):
    """[T_HIST, rows]: every row a random walk over a small pool of words, two thirds of them the planted maxima, so that bigrams
    repeat and the rule bans a planted maximum in part of the rows"""
    V, nparts, bias, plant = SHAPES[si]
    g = T.gen(1900 + 10 * si + beam)
    pool = list(plant) * 2 + [2, 3, V - 1]
    idx = torch.randint(0, len(pool), (T_HIST, B * beam), generator=g)
    return torch.tensor(pool, dtype=torch.int64)[idx].numpy()


def rules_of(si):
    r = dict(no_repeat_ngram=NGRAM)
    if SHAPES[si][0] == 8:                                      # five words banned: two candidates per row are left
        r["ban_words"] = [0, 2, 3, 4, 5]
    return r


@functools.lru_cache(maxsize=None)
def _block_ref(si, beam, t, groups, lam):
    c, hist = base_case(si, beam, t == 0), planted_history(si, beam)
    return GR.step(c["logits"], c["score"], c["done"], hist.T, t, c["B"], beam, c["unk"], groups, lam, **rules_of(si))


def block_ref(c, t, hist, rules, groups, lam):
    """the reference step of a case of this module, computed once per process and left unchanged"""
    si = next(i for i, s in enumerate(SHAPES) if s[0] == c["V"])
    assert c is base_case(si, c["beam"], t == 0) and hist is planted_history(si, c["beam"]) and rules == rules_of(si)
    return _block_ref(si, c["beam"], t, groups, float(lam))


def rank_case():
    """-> B, beam, T, hist [T, rows] int64, score [rows] fp32: histories without a 0, with a 0 at step 0, at step T - 1 and in
    between; scores on a coarse grid (the norms of a clip differ by >= 1e-3 or are exactly equal: equal score and equal length),
    -inf and NaN scores"""
    Bn, beam, Tn = 4, 6, 9
    g = T.gen(77)
    hist = torch.randint(1, 40, (Tn, Bn * beam), generator=g).numpy()
    first_zero = [[None, 0, Tn - 1, 3, 3, 5], [2, 2, None, None, 0, 7], [Tn - 1, 1, 4, None, 6, 0], [None, None, 3, 3, 3, 3]]
    score = np.array([[-3.5, -0.75, -9.25, -4.0, -4.0, -6.5], [-2.0, -2.0, -7.0, -7.0, -1.25, -np.inf],
                      [np.nan, -5.5, -np.inf, -8.0, np.nan, -0.5], [-6.0, -6.0, -1.5, -3.0, -1.5, -np.inf]], dtype=np.float32)
    for b in range(Bn):
        for k in range(beam):
            if first_zero[b][k] is not None:
                hist[first_zero[b][k], b * beam + k] = 0
                hist[min(first_zero[b][k] + 2, Tn - 1):, b * beam + k] = 0       # (later zeros do not matter)
    return Bn, beam, Tn, hist, score.reshape(-1)


ROUNDING_LAMBDA = 66.70001983642578           # an fp32 value whose product with 3 rounds UP in fp32: fl(3 l) = 200.10006713867188 > 3 l


@functools.lru_cache(maxsize=None)
def rounding_case():
    """A case whose selection is decided by the separately rounded product lambda * pen: beam 4 in 4 groups of one slot, t = 1, every
    row live and peaked (one logit 0 at word P, the others <= -250, so the row's log-sum-exp is exactly 0 in fp32 and fp64 and a
    candidate is exactly score + logit).  Groups 0, 1, 2 take P (at 0, -l, -2 l against <= -250), so group 3 sees pen(P) = 3.  Its
    row carries score 200: P's augmented value is 200 - fl(3 l) with the product rounded on its own (the subtraction is exact), and
    word Q < P has the logit -fl(3 l), so c(Q) = 200 - fl(3 l) EXACTLY: a tie, and the lower flat index Q wins.  A fused multiply-
    add gives P the value fl(200 - 3 l) > 200 - fl(3 l) (the product rounded up) and P wins instead.
    -> c (the dict of tile_path_cases.beam_case), t, hist [T_HIST, rows], lambda, P, Q"""
    Bn, beam, V, P, Q, t = 2, 4, 12, 7, 3, 1
    rows = Bn * beam
    g = T.gen(2100)
    lam = np.float32(ROUNDING_LAMBDA)
    p3 = np.float32(lam * np.float32(3))
    logits = -250.0 - torch.randint(0, 50, (rows, V), generator=g).float()
    logits[:, P] = 0.0
    score = torch.zeros(rows)
    for b in range(Bn):
        logits[b * beam + 3, Q] = -float(p3)
        score[b * beam + 3] = 200.0
    c = dict(name="rounding", B=Bn, beam=beam, V=V, unk=1, first=False, nparts=1, bias=False, logits=logits, score=score,
             done=torch.zeros(rows, dtype=torch.uint8), part_stride=rows * V, bias_shift=False, exact=True,
             parts=logits.view(1, rows, V), bias_v=None)
    hist = torch.full((T_HIST, rows), 2, dtype=torch.int64).numpy()
    return c, t, hist, float(lam), P, Q
