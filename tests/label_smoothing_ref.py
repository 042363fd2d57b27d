"""The label-smoothed vocabulary criterion restated (ISSUE: torch.nn.functional.cross_entropy(label_smoothing=eps)): for a row with
logits z [V], target t, weight w and lse = logsumexp(z)

    row_loss = w (lse - (1 - eps) z[t] - (eps / V) sum_v z[v])
    pre[v]   = w (softmax(z)[v] - (1 - eps) [v == t] - eps / V)         (d row_loss / d z)
    row_nll  = w (lse - z[t])                                           (the unsmoothed value)

`restate(logits, target, w, eps, dtype)` evaluates exactly these expressions in `dtype`: in fp64 it is the reference of the GPU tests
(cross-checked against torch's cross_entropy in tests/test_label_smoothing_cpu.py), in fp32 it is their yardstick -- a kernel's largest
error may be 4 x the yardstick's largest error on the same case, with a floor of 2^-20 (the convention of tests/test_gpu_cider.py)."""
import torch

FLOOR = 2.0 ** -20
SIZES = (5, 97, 257, 1000, 8192)          # the vocabulary sizes of the issue's CPU cross-check and of the kernel cases


def restate(logits, target, w, eps, dtype=torch.float64):
    """-> dict(row_loss [M], row_nll [M], loss_sum (), nll_sum (), pre [M, V], argmax [M] (ties -> the lowest index)), all in `dtype`
    (argmax int64); rows with w == 0 are exact zeros"""
    z = logits.to(dtype)
    wv = w.to(dtype)
    M, V = z.shape
    lse = torch.logsumexp(z, 1)
    zt = z.gather(1, target[:, None]).squeeze(1)
    eps_t = torch.tensor(eps, dtype=dtype)
    live = wv != 0
    row_loss = torch.where(live, wv * (lse - (1 - eps_t) * zt - (eps_t / V) * z.sum(1)), torch.zeros_like(wv))
    row_nll = torch.where(live, wv * (lse - zt), torch.zeros_like(wv))
    onehot = torch.nn.functional.one_hot(target, V).to(dtype)
    pre = wv[:, None] * (torch.exp(z - lse[:, None]) - (1 - eps_t) * onehot - eps_t / V)
    pre = torch.where(live[:, None], pre, torch.zeros_like(pre))
    mx = z.max(1, keepdim=True)[0]
    amax = torch.where(z == mx, torch.arange(V)[None], torch.full((1, V), V)).min(1)[0]
    return dict(row_loss=row_loss, row_nll=row_nll, loss_sum=row_loss.sum(), nll_sum=row_nll.sum(), pre=pre, argmax=amax)


def masked_mean(logits, target, mask, eps, dtype=torch.float64):
    """the criteria's value: the smoothed and the unsmoothed mean over sum(mask) of rows [M, V] -> (loss, nll)"""
    r = restate(logits, target, mask.to(dtype), eps, dtype)
    return r["loss_sum"] / mask.to(dtype).sum(), r["nll_sum"] / mask.to(dtype).sum()


def text_mask(target):
    """LMCriterion's loss mask of a [B, T] target: the steps up to and including the first 0"""
    m = target.gt(0)
    return torch.cat([torch.ones_like(m[:, :1]), m[:, :-1]], 1)


def case(M, V, seed, scale=4.0):
    """logits of scale `scale`, targets that include the last column and a column of the last, partly filled register slot (the
    fused kernel keeps column v in slot v // 256), weights 0, 1 and others -> (logits fp32 [M, V], target [M], w [M])"""
    g = torch.Generator().manual_seed(1000 * V + 10 * M + seed)
    logits = torch.randn(M, V, generator=g) * scale
    target = torch.randint(0, V, (M,), generator=g)
    w = torch.rand(M, generator=g) * 2.5 + 0.1
    target[0] = V - 1                                        # the last column
    if M > 1:
        target[1] = (V - 1) // 256 * 256                     # first column of the last register slot
        w[1] = 1.0
    if M > 2:
        w[2], target[2] = 0.0, 0                             # a padding row
    if M > 4:
        w[4] = 0.0                                           # a dead row with a live-looking target
    return logits, target, w
