"""The entropy regulariser of the vocabulary criterion restated (include/cvc_hip_blocks.h, cvc_vocab_head_nll_ent_fwd): for a row with
logits z [V], target t, NLL weight w (the 0 / 1 loss mask, or advantage x mask: any sign), entropy weight m (the 0 / 1 loss mask),
label smoothing eps, coefficient beta, lse = logsumexp(z) and p[v] = exp(z[v] - lse)

    H        = sum_v p[v] (lse - z[v])                                  every term >= 0; a column at -inf adds exactly 0
    row_loss = w (lse - (1 - eps) z[t] - (eps / V) sum_v z[v])  -  beta m H
    pre[v]   = w (p[v] - (1 - eps) [v == t] - eps / V)  +  beta m p[v] (z[v] - lse + H)         exactly 0 at z[v] = -inf
    row_ent  = m H
    row_nll  = w (lse - z[t])                                           (the unsmoothed value, without the entropy term)

H is summed from its non-negative terms, never formed as lse - sum p z (which cancels when H is small).

`restate(logits, target, w, m, eps, beta, dtype)` evaluates exactly these expressions in `dtype`: in fp64 it is the reference of the GPU
tests (cross-checked against torch autograd in tests/test_entropy_cpu.py), in fp32 it is their yardstick -- a kernel's largest error may
be 4 x the yardstick's largest error on the same case, with a floor of 2^-20 (the rule of tests/test_gpu_label_smoothing.py)."""
import torch

FLOOR = 2.0 ** -20
SIZES = (5, 97, 257, 1000, 8192)          # the vocabulary sizes of the issue's CPU cross-check and of the kernel cases
HEAD_CASES = [(1, 5, 1), (7, 97, 3), (9, 257, 2), (33, 1000, 2), (5, 8192, 1)]          # (M, V, slabs)
SETTINGS = [(0.0, 0.05), (0.1, 0.05), (0.0, -0.02)]                                       # (eps, beta)


def entropy(logits, dtype=torch.float64):
    """H [M] of the rows' softmax, and (p, lse)"""
    z = logits.to(dtype)
    lse = torch.logsumexp(z, 1)
    p = torch.exp(z - lse[:, None])
    gone = torch.isneginf(z)
    terms = torch.where(gone, torch.zeros_like(z), p * (lse[:, None] - torch.where(gone, torch.zeros_like(z), z)))
    return terms.sum(1), p, lse


def restate(logits, target, w, m, eps, beta, dtype=torch.float64):
    """-> dict(row_loss, row_nll, row_ent, H [M], loss_sum, nll_sum, ent_sum (), pre [M, V], argmax [M] (ties -> the lowest index)), all
    in `dtype` (argmax int64); a row with w == 0 and m == 0 is exact zeros"""
    z = logits.to(dtype)
    wv, mv = w.to(dtype), m.to(dtype)
    M, V = z.shape
    H, p, lse = entropy(logits, dtype)
    gone = torch.isneginf(z)
    zt = z.gather(1, target[:, None]).squeeze(1)
    eps_t, beta_t = torch.tensor(eps, dtype=dtype), torch.tensor(beta, dtype=dtype)
    live, counted = wv != 0, mv != 0
    zero = torch.zeros_like(wv)
    if eps == 0:
        base = wv * (lse - zt)
    else:
        base = wv * (lse - (1 - eps_t) * zt - (eps_t / V) * z.sum(1))
    base = torch.where(live, base, zero)
    row_nll = torch.where(live, wv * (lse - zt), zero)
    row_ent = torch.where(counted, mv * H, zero)
    row_loss = torch.where(counted, base - beta_t * mv * H, base)
    onehot = torch.nn.functional.one_hot(target, V).to(dtype)
    pre = wv[:, None] * (p - (1 - eps_t) * onehot - eps_t / V)
    pre = torch.where(live[:, None], pre, torch.zeros_like(pre))
    zf = torch.where(gone, torch.zeros_like(z), z)
    ent_g = (beta_t * mv)[:, None] * p * (zf - lse[:, None] + H[:, None])
    ent_g = torch.where(gone | ~counted[:, None], torch.zeros_like(ent_g), ent_g)
    mx = z.max(1, keepdim=True)[0]
    amax = torch.where(z == mx, torch.arange(V)[None], torch.full((1, V), V)).min(1)[0]
    return dict(row_loss=row_loss, row_nll=row_nll, row_ent=row_ent, H=H, loss_sum=row_loss.sum(), nll_sum=row_nll.sum(),
                ent_sum=row_ent.sum(), pre=pre + ent_g, argmax=amax)


def masked_mean(logits, target, w, mask, eps, beta, dtype=torch.float64):
    """the criteria's values: the means over sum(mask) of rows [M, V] -> (loss, nll, entropy)"""
    r = restate(logits, target, w.to(dtype), mask.to(dtype), eps, beta, dtype)
    count = mask.to(dtype).sum()
    return r["loss_sum"] / count, r["nll_sum"] / count, r["ent_sum"] / count


def text_mask(target):
    """LMCriterion's loss mask of a [B, T] target: the steps up to and including the first 0"""
    k = target.gt(0)
    return torch.cat([torch.ones_like(k[:, :1]), k[:, :-1]], 1)


def case(M, V, seed, scale=4.0):
    """logits of scale `scale`; targets that include the last column and a column of the last, partly filled register slot (the fused
    kernel keeps column v in slot v // 256); NLL weights 0, 1, negative and others; entropy weights 0 and 1 -- among them a padding
    row (w = m = 0) and a row with w = 0 and m = 1 (a rollout step whose advantage is 0)
    -> (logits fp32 [M, V], target [M], w [M], m [M])"""
    g = torch.Generator().manual_seed(1000 * V + 10 * M + seed)
    logits = torch.randn(M, V, generator=g) * scale
    target = torch.randint(0, V, (M,), generator=g)
    w = torch.rand(M, generator=g) * 2.5 + 0.1
    m = torch.ones(M)
    target[0] = V - 1                                        # the last column
    if M > 1:
        target[1] = (V - 1) // 256 * 256                     # first column of the last register slot
        w[1] = 1.0
    if M > 2:
        w[2], m[2], target[2] = 0.0, 0.0, 0                  # a padding row
    if M > 3:
        w[3] = -0.7                                          # a negative advantage
    if M > 4:
        w[4] = 0.0                                           # advantage 0 on a step that counts: the entropy term alone
    if M > 5:
        w[5], m[5] = 0.0, 0.0                                # a dead row with a live-looking target
    return logits, target, w, m


def minus_inf_columns(V, target):
    """columns to put at -inf (a banned word's bias): two that no row has as its target, none at V < 8"""
    if V < 8:
        return []
    taken = set(int(t) for t in target)
    return [c for c in (1, V // 2, V - 2, 3, V // 3) if c not in taken][:2]
