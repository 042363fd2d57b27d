"""The block cases of lexically constrained beam search, shared by tests/test_beam_forced_cpu.py (which checks on the fp64 reference
that they can be compared exactly and that they hold what they are meant to hold) and tests/test_gpu_beam_forced.py (which runs
them): the integer-logit cases of tile_path_cases.beam_case with planted histories, 40 % frozen rows and bigram blocking."""
import functools

import numpy as np
import torch

import tile_path_cases as T
import force_ref as FR

T_HIST = 65                                   # steps a history buffer holds: t <= 64 writes step t
# (V, nparts, bias, planted columns): V = 8 with five words banned, the general scan, the float4 scan, the engine's shape (6 slabs +
# bias).  The planted columns carry the row maximum in every row.
SHAPES = [(8, 1, False, (6,)), (50, 3, True, (0, 16, 49)), (1028, 1, False, (0, 30, 700, 1027)), (5000, 6, True, (0, 1666, 4999))]
BANKINGS = [(4, 1), (6, 2), (8, 3), (8, 1), (4, 3), (3, 2)]          # (beam, C)
# (shape, beam, C): every pair but V = 8 with beam 8 -- the selection blocks need V >= beam + 1
BLOCK_CASES = [(si, beam, C) for si in range(len(SHAPES)) for beam, C in BANKINGS if SHAPES[si][0] >= beam + 1]
B = 3
NGRAM = 2
STEPS = (0, 1, NGRAM, 63)
UNK = 1                                       # tile_path_cases.beam_case's


def force_of(si, C):
    """[B, C] int32.  near: the second planted maximum (inside the first entries of every live row's sorted list); far: a column with
    a drawn logit <= 0 high in the vocabulary (outside most rows' top-`beam`); mid: another drawn column.  Clip 0 forces (near,
    far, mid), clip 1 (far, unused, near), clip 2 (UNK, near, near again): with C = 1 it has no active entry at all.  V = 8: the
    two allowed words 6 and 7 and the banned word 2 -- an unmet forced word the ban set holds."""
    V, plant = SHAPES[si][0], SHAPES[si][3]
    near, far, mid = (6, 7, 2) if V == 8 else (plant[1], V - 3, V // 2 + 1)
    return np.array([[near, far, mid], [far, -1, near], [UNK, near, near]], dtype=np.int32)[:, :C].copy()


@functools.lru_cache(maxsize=None)
def base_case(si, beam, first):
    V, nparts, bias, plant = SHAPES[si]
    return T.beam_case(f"force{si}_{beam}", B, beam, V, 2300 + 10 * si + beam, plant=plant, first=first, nparts=nparts, bias=bias,
                       frozen=0.0 if first else 0.4)


@functools.lru_cache(maxsize=None)
def planted_history(si, beam):
    """[T_HIST, rows]: every row a random walk over a small pool of words -- the planted maxima, three plain words and the forced
    words -- so that bigrams repeat (the rule bans a forced word the row has met), rows of one clip have met different numbers of
    forced words after one or two steps and all of them after 63"""
    V, plant = SHAPES[si][0], SHAPES[si][3]
    g = T.gen(2500 + 10 * si + beam)
    pool = list(plant) * 2 + [2, 3, V - 1] + [int(w) for w in force_of(si, 3)[0]] * 2
    idx = torch.randint(0, len(pool), (T_HIST, B * beam), generator=g)
    return torch.tensor(pool, dtype=torch.int64)[idx].numpy()


def rules_of(si):
    r = dict(no_repeat_ngram=NGRAM)
    if SHAPES[si][0] == 8:                                      # five words banned: two candidates per row are left
        r["ban_words"] = [0, 2, 3, 4, 5]
    return r


@functools.lru_cache(maxsize=None)
def block_ref(si, beam, C, t):
    """the reference step of a case of this module, computed once per process and left unchanged"""
    c, hist = base_case(si, beam, t == 0), planted_history(si, beam)
    return FR.step(c["logits"], c["score"], c["done"], hist.T, t, B, beam, c["unk"], force_of(si, C), **rules_of(si))


def rank_case():
    """-> B, beam, T, V, hist [T, rows] int64, score [rows] fp32, force [B, C = 3] int32.  beam_groups_cases.rank_case's lengths and
    scores (equal norms, -inf, NaN) with forced words planted so that slots of one clip have met 0 .. 3 of them, a slot with a worse
    norm has met more than one with a better norm, a -inf slot and a NaN slot have met all, and an unused entry's word (UNK, a
    duplicate, -1) occurs in a history without counting."""
    import beam_groups_cases as GC
    Bn, beam, Tn, hist, score = GC.rank_case()
    hist = hist.copy()
    V = 40
    hist[hist >= 30] -= 20                                        # words 30 .. 39 occur only where they are planted below
    force = np.array([[31, 32, 33], [31, UNK, 31], [34, -1, 35], [36, 37, 38]], dtype=np.int32)
    plant = {0: {0: (), 1: (), 2: (31,), 3: (31, 32, 33), 4: (32,), 5: (33, 31)},
             1: {0: (31,), 1: (), 2: (31,), 3: (UNK,), 4: (), 5: (31,)},
             2: {0: (34, 35), 1: (34,), 2: (34, 35), 3: (), 4: (35,), 5: ()},
             3: {0: (36,), 1: (36,), 2: (), 3: (37, 38), 4: (36, 37, 38), 5: (36, 37, 38)}}
    for b in range(Bn):
        for k, ws in plant[b].items():
            r = b * beam + k
            free = [s for s in range(Tn) if hist[s, r] != 0][:len(ws)]
            assert len(free) == len(ws), (b, k)
            for s, w in zip(free, ws):
                hist[s, r] = w
    return Bn, beam, Tn, V, hist, score, force
