"""Word-level distillation in the vocabulary criterion restated (Hinton et al. 2015; Kim & Rush 2016): for a row with student logits
z [V], teacher scores s [V] (any log-scale row, normalised or not), target t, weight w, alpha in [0, 1] and tau > 0, with
p = softmax(z), p_tau = softmax(z / tau), q = softmax(s / tau)

    row_nll  = w (lse(z) - z[t])                                                  (unmixed)
    row_kd   = w tau^2 sum_v q[v] (log q[v] - log p_tau[v])                       (unmixed; a term with q[v] = 0 is 0)
    row_loss = (1 - alpha) row_nll + alpha row_kd
    pre[v]   = w ((1 - alpha) (p[v] - [v == t]) + alpha tau (p_tau[v] - q[v]))    (d row_loss / d z[v])

`restate(logits, teacher, target, w, alpha, tau, dtype)` evaluates exactly these expressions in `dtype`: in fp64 it is the reference of
the GPU tests (its `pre` cross-checked against torch autograd in tests/test_distill_cpu.py), in fp32 it is their yardstick -- a kernel's
largest error may be 4 x the yardstick's largest error on the same case, with a floor of 2^-20 (the convention of
tests/test_gpu_label_smoothing.py and tests/test_gpu_cider.py)."""
import torch

FLOOR = 2.0 ** -20
HEAD_CASES = [(1, 5, 1), (7, 97, 3), (9, 257, 2), (33, 1000, 2), (5, 8192, 1)]          # (M, V, nparts): the label-smoothing tests' shapes
SETTINGS = [(0.3, 1.0), (0.3, 2.0), (1.0, 1.0), (1.0, 2.0)]                              # (alpha, tau)


def restate(logits, teacher, target, w, alpha, tau, dtype=torch.float64):
    """-> dict(row_loss [M], row_nll [M], row_kd [M], loss_sum (), nll_sum (), kd_sum (), pre [M, V], argmax [M] (ties -> the lowest
    index)), all in `dtype` (argmax int64); rows with w == 0 are exact zeros whatever the teacher row holds"""
    z, s, wv = logits.to(dtype), teacher.to(dtype), w.to(dtype)
    M, V = z.shape
    a, t = torch.tensor(alpha, dtype=dtype), torch.tensor(tau, dtype=dtype)
    live = wv != 0
    logp = torch.log_softmax(z, 1)
    logpt = torch.log_softmax(z / t, 1)
    logq = torch.log_softmax(s / t, 1)
    q = logq.exp()
    terms = torch.where(q > 0, q * (logq - logpt), torch.zeros_like(q))
    zero = torch.zeros_like(wv)
    row_nll = torch.where(live, wv * -logp.gather(1, target[:, None]).squeeze(1), zero)
    row_kd = torch.where(live, wv * (t * t) * terms.sum(1), zero)
    row_loss = torch.where(live, (1 - a) * row_nll + a * row_kd, zero)
    onehot = torch.nn.functional.one_hot(target, V).to(dtype)
    pre = wv[:, None] * ((1 - a) * (logp.exp() - onehot) + a * t * (logpt.exp() - q))
    pre = torch.where(live[:, None], pre, torch.zeros_like(pre))
    mx = z.max(1, keepdim=True)[0]
    amax = torch.where(z == mx, torch.arange(V)[None], torch.full((1, V), V)).min(1)[0]
    return dict(row_loss=row_loss, row_nll=row_nll, row_kd=row_kd, loss_sum=row_loss.sum(), nll_sum=row_nll.sum(), kd_sum=row_kd.sum(),
                pre=pre, argmax=amax)


def mixed_mean(logits, teacher, target, mask, alpha, tau, dtype=torch.float64):
    """the criteria's value: the mixed loss, the unmixed NLL and the unmixed KD as means over sum(mask) of rows [M, V] -> (loss, nll, kd)"""
    r = restate(logits, teacher, target, mask.to(dtype), alpha, tau, dtype)
    n = mask.to(dtype).sum()
    return r["loss_sum"] / n, r["nll_sum"] / n, r["kd_sum"] / n


def case(M, V, seed, scale=4.0):
    """student logits of scale `scale`, teacher scores of another draw (unnormalised: a row offset is added), targets that include the
    last column and a column of the last, partly filled register slot (the fused kernel keeps column v in slot v // 256), weights 0,
    1 and others -> (logits fp32 [M, V], teacher fp32 [M, V], target [M], w [M])"""
    g = torch.Generator().manual_seed(1000 * V + 10 * M + seed)
    logits = torch.randn(M, V, generator=g) * scale
    teacher = torch.randn(M, V, generator=g) * scale + torch.randn(M, 1, generator=g) * 3.0
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
    return logits, teacher, target, w


def smoothed_teacher(target, V, eps):
    """s = log((1 - eps) onehot + eps / V) in fp64: the teacher row whose distillation at alpha = 1, tau = 1 is label smoothing up to
    the row's constant, row_kd + w H(q) = the smoothed row loss -> (s fp64 [M, V], q fp64 [M, V])"""
    q = (1.0 - eps) * torch.nn.functional.one_hot(target, V).double() + eps / V
    return q.log(), q


def entropy(q):
    """H(q) per row in fp64, 0 log 0 = 0"""
    q = q.double()
    return -torch.where(q > 0, q * q.clamp_min(1e-300).log(), torch.zeros_like(q)).sum(1)
