"""fp64 restatement of the recurrent half of nn.GRU(batch_first=True, bias=True) with h0 = 0 (gate order r, z, n; direction 1 walks
the sequence from the end): the forward keeping what the HIP training forwards save per step -- (r, z, n, hn) with hn = W_hn h + b_hn,
n = tanh(W_in x + b_in + r * hn), h' = (1 - z) n + z h -- and the backward written out from those saved tensors, returning the
pre-activation gradients dgi / dgh the backward kernels produce next to the parameter gradients.  tests/test_gru_ref_cpu.py proves it
against nn.GRU(...).double() and its autograd; it is the reference for element-wise GPU tests of the GRU kernels."""
import torch


def _sfx(bidir):
    return ["", "_reverse"] if bidir else [""]


def _param(params, name, l, s):
    return params[f"{name}_l{l}{s}"].detach().double()


def gru_recurrence(gi, w_hh, b_ih, b_hh, reverse):
    """gi [B, F, 3H] = x W_ih^T WITHOUT bias (fp64; what the kernels take) -> y [B, F, H], gates [B, F, 4, H] (r, z, n, hn)"""
    B, F, _ = gi.shape
    H = w_hh.shape[1]
    h = gi.new_zeros(B, H)
    y, gates = gi.new_zeros(B, F, H), gi.new_zeros(B, F, 4, H)
    for s in range(F):
        t = F - 1 - s if reverse else s
        gi_t = (gi[:, t] + b_ih).view(B, 3, H)
        gh = (h @ w_hh.T + b_hh).view(B, 3, H)
        r, z = torch.sigmoid(gi_t[:, 0] + gh[:, 0]), torch.sigmoid(gi_t[:, 1] + gh[:, 1])
        hn = gh[:, 2]
        n = torch.tanh(gi_t[:, 2] + r * hn)
        h = (1 - z) * n + z * h
        y[:, t] = h
        gates[:, t] = torch.stack((r, z, n, hn), 1)
    return y, gates


def gru_layer_forward(x, w_ih, w_hh, b_ih, b_hh, reverse):
    """x [B, F, in] (fp64) -> y [B, F, H], gates [B, F, 4, H] (r, z, n, hn)"""
    return gru_recurrence(x @ w_ih.T, w_hh, b_ih, b_hh, reverse)


def gru_layer_backward(dy, x, y, gates, w_ih, w_hh, reverse):
    """-> dx, dw_ih, dw_hh, db_ih, db_hh, dgi [B, F, 3H], dgh [B, F, 3H] (the pre-activation gradients of the input / hidden side:
    dgh carries dn * r where dgi carries dn)"""
    B, F, H = y.shape
    carry = dy.new_zeros(B, H)
    dgi, dgh = dy.new_zeros(B, F, 3 * H), dy.new_zeros(B, F, 3 * H)
    hprev = torch.zeros_like(y)
    for s in reversed(range(F)):
        t = F - 1 - s if reverse else s
        tp = t + 1 if reverse else t - 1
        if 0 <= tp < F:
            hprev[:, t] = y[:, tp]
        r, z, n, hn = gates[:, t, 0], gates[:, t, 1], gates[:, t, 2], gates[:, t, 3]
        dh = dy[:, t] + carry
        dn = dh * (1 - z) * (1 - n * n)
        dz = dh * (hprev[:, t] - n) * z * (1 - z)
        dr = dn * hn * r * (1 - r)
        dgi[:, t] = torch.cat((dr, dz, dn), 1)
        dgh[:, t] = torch.cat((dr, dz, dn * r), 1)
        carry = dh * z + dgh[:, t] @ w_hh
    fi, fh = dgi.reshape(B * F, 3 * H), dgh.reshape(B * F, 3 * H)
    return dgi @ w_ih, fi.T @ x.reshape(B * F, -1), fh.T @ hprev.reshape(B * F, H), fi.sum(0), fh.sum(0), dgi, dgh


def gru_forward(x, params, layers, bidir, masks=None):
    """params: name -> tensor (nn.GRU's names); masks: per inter-layer site l a multiplier tensor [B, F, ndir*H] (dropout), or None.
    -> y of the last layer (fp64), saved: per layer (input, [per direction (y, gates)])"""
    cur = x.double()
    saved = []
    for l in range(layers):
        per = []
        for d, s in enumerate(_sfx(bidir)):
            per.append(gru_layer_forward(cur, *[_param(params, n, l, s) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")],
                                         d == 1))
        saved.append((cur, per))
        cur = torch.cat([p[0] for p in per], 2)
        if masks is not None and l + 1 < layers and masks[l] is not None:
            cur = cur * masks[l].double()
    return cur, saved


def gru_backward(dy, saved, params, layers, bidir, masks=None):
    """-> dx, {name: gradient}"""
    grads = {}
    d_out = dy.double()
    for l in reversed(range(layers)):
        if masks is not None and l + 1 < layers and masks[l] is not None:
            d_out = d_out * masks[l].double()
        x, per = saved[l]
        H = per[0][0].shape[2]
        dx = torch.zeros_like(x)
        for d, s in enumerate(_sfx(bidir)):
            y, gates = per[d]
            dxi, dwi, dwh, dbi, dbh, _, _ = gru_layer_backward(d_out[:, :, d * H:(d + 1) * H], x, y, gates,
                                                               _param(params, "weight_ih", l, s), _param(params, "weight_hh", l, s), d == 1)
            dx = dx + dxi
            grads[f"weight_ih_l{l}{s}"], grads[f"weight_hh_l{l}{s}"] = dwi, dwh
            grads[f"bias_ih_l{l}{s}"], grads[f"bias_hh_l{l}{s}"] = dbi, dbh
        d_out = dx
    return d_out, grads


def make_gru(inp, H, layers, bidir, seed, dropout=0.0):
    """nn.GRU with its parameters scaled by 1.5 (as test_encoder._gru does): the gates leave the linear region"""
    torch.manual_seed(seed)
    g = torch.nn.GRU(inp, H, layers, dropout=dropout, bidirectional=bidir, batch_first=True)
    with torch.no_grad():
        for p in g.parameters():
            p.mul_(1.5)
    return g
