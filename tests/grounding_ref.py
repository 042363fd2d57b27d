"""The grounding scores of generated captions, restated in numpy (what csrc/grounding.hip computes; cvc.metrics): picks per object
word and sampled frame, the fp32 hit test operation by operation, the six per-class counters, the per-row counts and F1, and the
scores of a table in fp64.  Plain loops, no vectorisation: this file is the definition the kernel is compared with."""
import numpy as np

COLUMNS = ("gt", "gt_pred", "gt_hit", "pred", "pred_in_gt", "pred_hit")
KEYS = ("F1_all", "F1_loc", "Prec_all", "Recall_all", "Prec_loc", "Recall_loc", "F1_all_micro", "F1_loc_micro")
f32 = np.float32


def word_classes(row, word_cls, n_classes):
    """-> the class of every position: word_cls[id] for the positions before the first 0 whose id lies in [0, V) and whose class
    lies in [1, n_classes], 0 everywhere else"""
    out = [0] * len(row)
    for t, w in enumerate(row):
        w = int(w)
        if w == 0:
            break
        if 0 <= w < len(word_cls) and 1 <= int(word_cls[w]) <= n_classes:
            out[t] = int(word_cls[w])
    return out


def frame_pick(weights, f, n_per, P):
    """the slot f * n_per + j with the largest weight: the search starts at j = 0 and moves on a strict >; a slot >= P weighs -inf"""
    w = lambda j: f32(weights[f * n_per + j]) if f * n_per + j < P else f32(-np.inf)
    best, bj = w(0), 0
    for j in range(1, n_per):
        if w(j) > best:
            best, bj = w(j), j
    return f * n_per + bj


def hit(a, g):
    """the picked proposal a and the annotated box g (x1, y1, x2, y2): every operation in fp32 and rounded on its own"""
    a, g = [f32(x) for x in a], [f32(x) for x in g]
    w = f32(min(a[2], g[2]) - max(a[0], g[0]))
    h = f32(min(a[3], g[3]) - max(a[1], g[1]))
    if w <= 0 or h <= 0:
        return False
    inter = f32(w * h)
    area_a = f32(f32(a[2] - a[0]) * f32(a[3] - a[1]))
    area_g = f32(f32(g[2] - g[0]) * f32(g[3] - g[1]))
    union = f32(f32(area_a + area_g) - inter)
    return bool(f32(f32(2) * inter) > union)


def row_f1(counts):
    """the row's micro F1_all in fp64 from its six counts"""
    gt, _, gt_hit, pred, _, pred_hit = (float(x) for x in counts)
    if gt == 0 or pred == 0:
        return 0.0
    p, r = pred_hit / pred, gt_hit / gt
    return 2 * p * r / (p + r) if p + r > 0 else 0.0


def score_batch(seq, att, ppls, gt_bboxs, nbox, word_cls, frames, n_per, n_classes, per_clip=1, table=None):
    """seq [rows, T]; att [rows, T, P]; ppls [clips, P, >= 4]; gt_bboxs [clips, K, 6]; nbox [clips]
    -> dict(pick [rows, T, frames] int64, counts [rows, 6] int64, f1 [rows] fp64, table [n_classes + 1, 6] int64: the given one plus
    this batch)"""
    seq, att, ppls, gt_bboxs = np.asarray(seq), np.asarray(att, dtype=f32), np.asarray(ppls, dtype=f32), np.asarray(gt_bboxs, dtype=f32)
    rows, T = seq.shape
    P, K = att.shape[2], gt_bboxs.shape[1]
    table = np.zeros((n_classes + 1, 6), dtype=np.int64) if table is None else np.array(table, dtype=np.int64)
    pick = np.full((rows, T, frames), -1, dtype=np.int64)
    counts = np.zeros((rows, 6), dtype=np.int64)
    for r in range(rows):
        b = r // per_clip
        cls = word_classes(seq[r], word_cls, n_classes)
        rep = {}
        for t, c in enumerate(cls):
            if c > 0:
                rep.setdefault(c, t)
                for f in range(frames):
                    pick[r, t, f] = frame_pick(att[r, t], f, n_per, P)
        mine = np.zeros((n_classes + 1, 6), dtype=np.int64)
        hit_classes = set()
        gt_classes = set()
        for k in range(min(max(int(nbox[b]), 0), K)):
            c, f = int(gt_bboxs[b, k, 5]), int(gt_bboxs[b, k, 4])
            if not 1 <= c <= n_classes:
                continue
            gt_classes.add(c)
            mine[c, 0] += 1
            if c not in rep:
                continue
            mine[c, 1] += 1
            if 0 <= f < frames:
                slot = int(pick[r, rep[c], f])
                box = ppls[b, slot, :4] if slot < P else np.zeros(4, dtype=f32)
                if hit(box, gt_bboxs[b, k, :4]):
                    mine[c, 2] += 1
                    hit_classes.add(c)
        for c in rep:
            mine[c, 3] += 1
            mine[c, 4] += c in gt_classes
            mine[c, 5] += c in hit_classes
        counts[r] = mine.sum(0)
        table += mine
    return dict(pick=pick, counts=counts, f1=np.array([row_f1(c) for c in counts], dtype=np.float64), table=table)


def result(table):
    """the ten-line definition of the scores, fp64: means over the classes with gt > 0, the micro scores on the column sums"""
    t = np.asarray(table, dtype=np.float64).reshape(-1, 6)
    f1 = lambda p, r: 2 * p * r / (p + r) if p + r > 0 else 0.0
    mean = lambda xs: float(sum(xs) / len(xs)) if xs else 0.0
    S = [row for row in t if row[0] > 0]
    prec_all = mean([row[5] / row[3] if row[3] > 0 else 0.0 for row in S])
    rec_all = mean([row[2] / row[0] for row in S])
    prec_loc = mean([row[5] / row[4] for row in S if row[4] > 0])
    rec_loc = mean([row[2] / row[1] for row in S if row[1] > 0])
    s = t.sum(0)
    ratio = lambda a, b: float(a / b) if b > 0 else 0.0
    return {"F1_all": f1(prec_all, rec_all), "F1_loc": f1(prec_loc, rec_loc), "Prec_all": prec_all, "Recall_all": rec_all,
            "Prec_loc": prec_loc, "Recall_loc": rec_loc, "F1_all_micro": f1(ratio(s[5], s[3]), ratio(s[2], s[0])),
            "F1_loc_micro": f1(ratio(s[5], s[4]), ratio(s[2], s[1]))}


# ---------------------------------------------------------------------------------------------------------- seeded cases
# (rows, per_clip, T, F, Np, P, K, C, V): the GPU test's case list -- fewer weights than a wave, exactly a wave, a wave and a tail, the
# real size; P trimmed inside a frame and so that a whole frame is absent; T = 8, 20 and 63; 1, 5, 6 and 64 rows; per_clip 1 and 3
CASES = [
    (1, 1, 8, 2, 5, 10, 4, 6, 30),
    (5, 1, 8, 2, 5, 8, 100, 6, 30),               # P trimmed in the middle of frame 1
    (6, 3, 63, 3, 64, 192, 100, 12, 50),
    (5, 1, 8, 3, 64, 128, 7, 12, 50),             # frame 2 is absent
    (6, 3, 8, 2, 70, 140, 100, 12, 50),
    (5, 1, 63, 2, 70, 100, 9, 12, 50),            # P trimmed inside frame 1, behind its first wave
    (64, 1, 20, 10, 100, 1000, 100, 40, 200),
    (64, 1, 20, 10, 100, 930, 100, 40, 200),      # the real size, trimmed inside the last frame
]


def make_case(rows, per_clip, T, F, Np, P, K, C, V, seed=0):
    """Seeded inputs with integer box coordinates below 2048 (every fp32 product is exact).  Annotated boxes are made from proposals
    of their frame: a copy (IoU 1), a box of exactly half the proposal (IoU exactly 1/2: a miss), a shifted box, or a far one; about
    half of each clip's classes are predicted by its captions.  Special rows and boxes, where the sizes allow them: equal maxima in
    a frame, a frame of -inf, a caption without a 0, a caption that starts with 0, word ids >= V, nbox = 0, nbox = K, boxes with
    frame -1 and frame >= F."""
    rng = np.random.default_rng(seed + 1000 * rows + 10 * T + F + Np + P)
    clips = rows // per_clip
    word_cls = np.zeros(V, dtype=np.int32)
    obj_words = rng.choice(np.arange(1, V), size=min(V - 1, 2 * C), replace=False)
    for i, w in enumerate(obj_words):
        word_cls[w] = 1 + i % C                     # two words per class where the vocabulary allows it
    ppls = np.zeros((clips, P, 7), dtype=np.float32)
    xy = rng.integers(0, 1000, (clips, P, 2))
    wh = 2 * rng.integers(5, 400, (clips, P, 2))    # even widths and heights: half a box has integer coordinates
    ppls[:, :, 0:2], ppls[:, :, 2:4] = xy, xy + wh
    ppls[:, :, 4] = np.arange(P)[None, :] // Np
    ppls[:, :, 6] = rng.random((clips, P))
    att = rng.random((rows, T, P)).astype(np.float32)
    seq = np.zeros((rows, T), dtype=np.int64)
    for r in range(rows):
        n = int(rng.integers(1, T + 1))
        words = rng.integers(1, V, n)
        take = rng.random(n) < 0.45                                  # object words, some of them twice or of the same class
        words[take] = rng.choice(obj_words, int(take.sum()))
        seq[r, :n] = words
        if n < T:
            seq[r, n + 1:] = rng.integers(0, V, T - n - 1)          # what stands behind the end mark is ignored
    if rows >= 5:
        seq[1, :] = np.where(seq[1] == 0, obj_words[0], seq[1])      # a caption without a 0
        seq[2, 0] = 0                                                # a caption whose first word is 0
        seq[3, 0], seq[3, 1] = V, V + 7                              # ids >= V in front of the rest
        seq[3, 2] = obj_words[1]
    gt = np.zeros((clips, K, 6), dtype=np.float32)
    nbox = np.zeros(clips, dtype=np.int32)
    for b in range(clips):
        r0 = b * per_clip
        annotated = [c for c in range(1, C + 1) if c % 4 != b % 4]      # a quarter of the classes has no box in this clip
        predicted = sorted(({c for r in range(r0, r0 + per_clip) for c in word_classes(seq[r], word_cls, C)} - {0}) & set(annotated))
        nbox[b] = K if b == 0 else (0 if (b == 1 and clips > 2) else int(rng.integers(1, K + 1)))
        for k in range(K):
            c = int(predicted[int(rng.integers(0, len(predicted)))]) if (predicted and rng.random() < 0.6) \
                else int(annotated[int(rng.integers(0, len(annotated)))])
            f = int(rng.integers(0, F))
            lo, hi = f * Np, min((f + 1) * Np, P)
            kind = int(rng.integers(0, 4))
            if hi <= lo:                                             # an absent frame: no proposal to copy
                box = [3, 4, 50, 60]
            else:
                p = ppls[b, int(rng.integers(lo, hi)), :4]
                if kind == 0:
                    box = list(p)
                elif kind == 1:                                      # the left half: inter = area / 2, union = area: exactly 1/2
                    box = [p[0], p[1], p[0] + (p[2] - p[0]) / 2, p[3]]
                elif kind == 2:
                    box = [p[0] + 3, p[1] + 2, p[2] + 3, p[3] + 2]
                else:
                    box = [1500, 1500, 1600, 1700]
            gt[b, k, :4] = box
            gt[b, k, 4], gt[b, k, 5] = f, c
        if K >= 4:
            gt[b, 1, 4] = -1                                         # test mode: never hits
            gt[b, 2, 4] = F                                          # a frame that was not sampled
            gt[b, 3, 5] = 0                                          # no class: not counted
    # sharpen: the representative of every predicted class attends to the proposal one of the class's boxes was made from
    for r in range(rows):
        b = r // per_clip
        cls = word_classes(seq[r], word_cls, C)
        for t, c in enumerate(cls):
            if c == 0:
                continue
            for f in range(F):
                lo, hi = f * Np, min((f + 1) * Np, P)
                if hi <= lo:
                    continue
                mode = (r + t + f) % 4
                if mode == 0:                                        # equal maxima: the lowest slot wins
                    js = rng.choice(np.arange(lo, hi), size=min(3, hi - lo), replace=False)
                    att[r, t, js] = 2.0
                elif mode == 1:                                      # a frame of -inf
                    att[r, t, lo:hi] = -np.inf
                else:                                                # the proposal a box of this class and frame was made from
                    ks = [k for k in range(min(int(nbox[b]), K)) if int(gt[b, k, 5]) == c and int(gt[b, k, 4]) == f]
                    if ks:
                        g = gt[b, ks[0], :4]
                        d = np.abs(ppls[b, lo:hi, :4] - g[None, :]).sum(1)
                        att[r, t, lo + int(np.argmin(d))] = 3.0
    return dict(seq=seq, att=att, ppls=ppls, gt_bboxs=gt, nbox=nbox, word_cls=word_cls, frames=F, n_per=Np, n_classes=C, per_clip=per_clip)


_CACHE = {}


def case(key):
    """-> (inputs, restatement's outputs) of CASES[...] == key: built once, shared, left unchanged"""
    if key not in _CACHE:
        inp = make_case(*key)
        _CACHE[key] = (inp, score_batch(**inp))
    return _CACHE[key]
