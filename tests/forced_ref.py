"""Reference of the teacher-forced selection block (csrc/forced.hip, cvc_forced_select_parts) and of the forced decode, on the CPU.

The logits are formed in fp32 in the documented slab order (slab 0 + slab 1 + ... + bias: cvc_tile_linear_finish's, as
tests/sample_oracle.py forms them), the rank is computed exactly from that fp32 z, the log-prob in fp64."""
import numpy as np
import torch


def finished(parts: torch.Tensor, bias) -> torch.Tensor:
    """[nparts, M, V] fp32 slabs (+ bias [V]) -> z [M, V] fp32, summed in the finishing pass's order"""
    z = parts[0].clone()
    for k in range(1, parts.shape[0]):
        z = z + parts[k]
    return z + bias if bias is not None else z


def rank_of(z_row: np.ndarray, w: int) -> int:
    """#{v : z[v] > z[w]} + #{v < w : z[v] == z[w]} (NaN compares false)"""
    with np.errstate(invalid="ignore"):
        return int((z_row > z_row[w]).sum() + (z_row[:w] == z_row[w]).sum())


def forced_select(z: torch.Tensor, words) -> tuple:
    """z [M, V] fp32, words [M] -> (logprob [M] fp64, rank [M] int32).  A word outside [0, V): NaN / -1."""
    zn = z.numpy()
    M, V = zn.shape
    lp, rk = np.full(M, np.nan), np.full(M, -1, dtype=np.int32)
    for r in range(M):
        w = int(words[r])
        if not 0 <= w < V:
            continue
        rk[r] = rank_of(zn[r], w)
        zd = zn[r].astype(np.float64)
        if np.isnan(zd).any():
            continue                                          # a NaN logit poisons the log-sum-exp
        m = zd.max()
        lp[r] = zd[w] - (m + np.log(np.exp(zd - m).sum()))
    return lp, rk


def forced_decode(P, feats, words: torch.Tensor, n: int, frame_mask=None, softattn_type: str = "additive", temp: float = 1.0):
    """The oracle's decoder over given words [B * n, T] (row b * n + j = caption j of clip b): a loop of O.decoder_step +
    O.logits_logsoftmax.  -> log-softmax [rows, T, V], att [rows, T, N], frame-masked pre-softmax scores [rows, T, N] or None."""
    from oracle import ref_cpu as O
    rep = lambda x: x.repeat_interleave(n, 0)
    fc, conv, pconv = rep(feats["fc_feats"]), rep(feats["conv_feats"]), rep(feats["p_conv_feats"])
    pool, ppool, mask = rep(feats["pool_feats"]), rep(feats["p_pool_feats"]), rep(feats["pnt_mask"][:, 1:])
    rows, T = words.shape
    state = O.init_hidden(rows, fc.size(1))
    prev = torch.zeros(rows, dtype=torch.long)
    lps, atts, fms = [], [], []
    with torch.no_grad():
        for t in range(T):
            out, state, a_r, fm, _ = O.decoder_step(P, O.embed(P, prev), fc, conv, pconv, pool, ppool, mask, state,
                                                    None if frame_mask is None else frame_mask[t], softattn_type=softattn_type,
                                                    temp=temp)
            lps.append(O.logits_logsoftmax(P, out))
            atts.append(a_r)
            fms.append(fm)
            prev = words[:, t]
    return torch.stack(lps, 1), torch.stack(atts, 1), (None if frame_mask is None else torch.stack(fms, 1))


def rank_band(lp_row: np.ndarray, w: int, tol: float):
    """the ranks of word w that a log-softmax within `tol` of lp_row allows: [#{v != w : lp[v] > lp[w] + 2 tol},
    #{v != w : lp[v] >= lp[w] - 2 tol}]"""
    others = np.delete(lp_row, w)
    return int((others > lp_row[w] + 2 * tol).sum()), int((others >= lp_row[w] - 2 * tol).sum())


# ---------------------------------------------------------------- grounding on given sentences: the arithmetic of Trainer.ground_gt
def ground_picks(weights: np.ndarray, frm_mask_output: np.ndarray, roi_labels: np.ndarray):
    """weights [B, T, N], frm_mask_output [B, T, N + 1] bool, roi_labels [B, T, N] bool -> pick [B, T] (arg-max over the proposals
    that are not frame-masked, lowest index on ties; -1 without such a proposal) and hit [B, T] bool."""
    B, T, N = weights.shape
    pick, hit = np.full((B, T), -1, dtype=np.int64), np.zeros((B, T), dtype=bool)
    for b in range(B):
        for t in range(T):
            best = None
            for i in range(N):
                if frm_mask_output[b, t, 1 + i]:
                    continue
                if best is None or weights[b, t, i] > weights[b, t, best]:
                    best = i
            if best is not None:
                pick[b, t], hit[b, t] = best, bool(roi_labels[b, t, best])
    return pick, hit


def ground_accuracy(hit: np.ndarray, input_seq: np.ndarray, box_mask: np.ndarray, vocab_size: int):
    """hit [B, T]; input_seq [B, 1, T + 1, 4]; box_mask [B, 1, K, T + 1] -> (accuracy over the annotated object words, mean of the
    per-class accuracies, number of such words)"""
    B, T = hit.shape
    cls = input_seq[:, 0, 1:T + 1, 0] - vocab_size
    per = {}
    for b in range(B):
        for t in range(T):
            if cls[b, t] >= 1 and (~box_mask[b, 0, :, t + 1]).any():
                per.setdefault(int(cls[b, t]), []).append(bool(hit[b, t]))
    allh = [h for v in per.values() for h in v]
    if not allh:
        return 0.0, 0.0, 0
    return float(np.mean(allh)), float(np.mean([np.mean(v) for v in per.values()])), len(allh)
