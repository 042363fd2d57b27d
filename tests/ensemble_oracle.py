"""Reference of ensemble decoding on the CPU: the combine of csrc/ensemble.hip restated in numpy (an fp32 form in the kernel's order
and an fp64 form), and a joint greedy decoder that steps M CPU models (oracle.ref_cpu) and picks every word from the fp64 mixture
without UNK."""
import numpy as np
import torch

f32 = np.float32


def finished(parts, bias):
    """slab 0 + slab 1 + ... + bias in fp32: the selection blocks' row loader"""
    z = np.array(parts[0], dtype=f32, copy=True)
    for k in range(1, len(parts)):
        z = (z + parts[k]).astype(f32)
    return z if bias is None else (z + bias.astype(f32)).astype(f32)


def combine32(xs, logw, geometric):
    """the kernel's definition in fp32 numpy, members in index order (another expf / logf and another reduction tree than the
    device's).  xs: M finished [rows, V] fp32 matrices"""
    acc = None
    with np.errstate(over="ignore", invalid="ignore"):
        for m, x in enumerate(xs):
            x = x.astype(f32)
            mx = x.max(1, keepdims=True)
            lse = (mx + np.log(np.exp((x - mx).astype(f32)).astype(f32).sum(1, keepdims=True, dtype=f32)).astype(f32)).astype(f32)
            if geometric:
                a = (np.exp(f32(logw[m])).astype(f32) * (x - lse).astype(f32)).astype(f32)
                acc = a if acc is None else (acc + a).astype(f32)
            else:
                a = ((x - lse).astype(f32) + f32(logw[m])).astype(f32)
                acc = a if acc is None else (np.maximum(acc, a) + np.log1p(np.exp(-np.abs(acc - a).astype(f32)).astype(f32)).astype(f32)).astype(f32)
    return acc


def combine64(xs, logw, geometric):
    """the same in fp64 (log-weights as given: the fp32 values the kernel reads)"""
    logw = np.asarray(logw, dtype=np.float64)
    lps = []
    for x in xs:
        x = x.astype(np.float64)
        mx = x.max(1, keepdims=True)
        lps.append(x - (mx + np.log(np.exp(x - mx).sum(1, keepdims=True))))
    if geometric:
        return sum(np.exp(lw) * lp for lw, lp in zip(logw, lps))
    a = np.stack([lp + lw for lw, lp in zip(logw, lps)])
    mx = a.max(0)
    return mx + np.log(np.exp(a - mx).sum(0))


def mixture_logp(logps, weights, combine):
    """fp64 log of the combined distribution, NORMALISED in both forms, from the members' log-softmax rows [M][rows, V] and the
    normalised weights"""
    lp = np.stack([np.asarray(x, dtype=np.float64) for x in logps])
    w = np.asarray(weights, dtype=np.float64).reshape(-1, 1, 1)
    if combine == "prob":
        mx = lp.max(0)
        return mx + np.log((w * np.exp(lp - mx)).sum(0))
    g = (w * lp).sum(0)
    mx = g.max(1, keepdims=True)
    return g - (mx + np.log(np.exp(g - mx).sum(1, keepdims=True)))


def joint_greedy(Ps, feats, T, unk_idx, weights, combine="prob", given=None):
    """M CPU models in lock-step: every step's word is the arg-max without UNK of the fp64 mixture (given [rows, T]: the words to
    follow instead).  -> (seq [B, T], att [M][B, T, N] per member, logprob [B, T] of the word under the mixture, mix [B, T, V] the fp64
    mixture log-probs, logps [M][B, T, V] the members' log-probs)"""
    from oracle import ref_cpu as O
    w = np.asarray(weights, dtype=np.float64)
    w = w / w.sum()
    M, B = len(Ps), feats[0]["fc_feats"].size(0)
    states = [O.init_hidden(B, f["fc_feats"].size(1)) for f in feats]
    word = torch.zeros(B, dtype=torch.long)
    seq, atts, lps, mixes, member_lp = [], [[] for _ in range(M)], [], [], [[] for _ in range(M)]
    with torch.no_grad():
        for t in range(T):
            step = []
            for m, (P, f) in enumerate(zip(Ps, feats)):
                out, states[m], a_r, _, _ = O.decoder_step(P, O.embed(P, word), f["fc_feats"], f["conv_feats"], f["p_conv_feats"],
                                                           f["pool_feats"], f["p_pool_feats"], f["pnt_mask"][:, 1:], states[m], None)
                step.append(O.logits_logsoftmax(P, out).double().numpy())
                atts[m].append(a_r)
                member_lp[m].append(step[-1])
            mix = mixture_logp(step, w, combine)
            pick = mix.copy()
            pick[:, unk_idx] = -np.inf
            nxt = pick.argmax(1) if given is None else np.asarray(given[:, t])
            seq.append(nxt)
            lps.append(mix[np.arange(B), nxt])
            mixes.append(mix)
            word = torch.from_numpy(np.asarray(nxt, dtype=np.int64))
    return (np.stack(seq, 1), [torch.stack(a, 1).numpy() for a in atts], np.stack(lps, 1), np.stack(mixes, 1),
            [np.stack(x, 1) for x in member_lp])
