"""fp64 restatement of the recurrent half of nn.LSTM(batch_first=True, bias=True) with h0 = c0 = 0 (gate order i, f, g, o; direction 1
walks the sequence from the end): the forward keeping every step's activated gates and c_t, and the backward written out from those
saved tensors.  tests/test_lstm_seq_cpu.py proves it against nn.LSTM(...).double() and its autograd; the GPU tests use it as their
reference (tests/test_gpu_lstm_seq.py, tests/test_gpu_lstm_seq_kernels.py through tests/lstm_seq_cases.py)."""
import torch


def _sfx(bidir):
    return ["", "_reverse"] if bidir else [""]


def lstm_recurrence(gi, w_hh, b_ih, b_hh, reverse):
    """the recurrence alone, from the input projections gi = x W_ih^T [B, F, 4H] (fp64, no bias) -> y [B, F, H], gates [B, F, 4, H]
    (activated i, f, g, o), c [B, F, H]"""
    B, F, _ = gi.shape
    H = w_hh.shape[1]
    h = gi.new_zeros(B, H)
    c = gi.new_zeros(B, H)
    y, gates, cs = gi.new_zeros(B, F, H), gi.new_zeros(B, F, 4, H), gi.new_zeros(B, F, H)
    for s in range(F):
        t = F - 1 - s if reverse else s
        z = (gi[:, t] + b_ih + h @ w_hh.T + b_hh).view(B, 4, H)
        i, f, g, o = torch.sigmoid(z[:, 0]), torch.sigmoid(z[:, 1]), torch.tanh(z[:, 2]), torch.sigmoid(z[:, 3])
        c = f * c + i * g
        h = o * torch.tanh(c)
        y[:, t], cs[:, t] = h, c
        gates[:, t] = torch.stack((i, f, g, o), 1)
    return y, gates, cs


def lstm_layer_forward(x, w_ih, w_hh, b_ih, b_hh, reverse):
    """x [B, F, in] (fp64) -> y [B, F, H], gates [B, F, 4, H] (activated i, f, g, o), c [B, F, H]"""
    return lstm_recurrence(x @ w_ih.T, w_hh, b_ih, b_hh, reverse)


def lstm_layer_backward(dy, x, y, gates, cs, w_ih, w_hh, reverse):
    """-> dx, dw_ih, dw_hh, db (= db_ih = db_hh), dz [B, F, 4H] (the pre-activation gradients)"""
    B, F, H = y.shape
    dh_c = dy.new_zeros(B, H)
    dc_c = dy.new_zeros(B, H)
    dz = dy.new_zeros(B, F, 4 * H)
    hprev = torch.zeros_like(y)
    for s in reversed(range(F)):
        t = F - 1 - s if reverse else s
        tp = t + 1 if reverse else t - 1
        has_prev = 0 <= tp < F
        i, f, g, o = gates[:, t, 0], gates[:, t, 1], gates[:, t, 2], gates[:, t, 3]
        c_prev = cs[:, tp] if has_prev else torch.zeros_like(cs[:, t])
        if has_prev:
            hprev[:, t] = y[:, tp]
        tc = torch.tanh(cs[:, t])
        dh = dy[:, t] + dh_c
        dc = dh * o * (1 - tc * tc) + dc_c
        d = torch.cat((dc * g * i * (1 - i), dc * c_prev * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)), 1)
        dz[:, t] = d
        dh_c = d @ w_hh
        dc_c = dc * f
    flat = dz.reshape(B * F, 4 * H)
    return dz @ w_ih, flat.T @ x.reshape(B * F, -1), flat.T @ hprev.reshape(B * F, H), flat.sum(0), dz


def lstm_forward(x, params, layers, bidir, masks=None):
    """params: name -> tensor (nn.LSTM's names); masks: per inter-layer site l a multiplier tensor [B, F, ndir*H] (dropout), or None.
    -> y of the last layer (fp64), saved: per layer (input, [per direction (y, gates, c)])"""
    cur = x.double()
    saved = []
    for l in range(layers):
        per = []
        for d, s in enumerate(_sfx(bidir)):
            g = lambda n: params[f"{n}_l{l}{s}"].detach().double()
            per.append(lstm_layer_forward(cur, g("weight_ih"), g("weight_hh"), g("bias_ih"), g("bias_hh"), d == 1))
        saved.append((cur, per))
        cur = torch.cat([p[0] for p in per], 2)
        if masks is not None and l + 1 < layers and masks[l] is not None:
            cur = cur * masks[l].double()
    return cur, saved


def lstm_backward(dy, saved, params, layers, bidir, masks=None):
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
            g = lambda n: params[f"{n}_l{l}{s}"].detach().double()
            y, gates, cs = per[d]
            dxi, dwi, dwh, db, _ = lstm_layer_backward(d_out[:, :, d * H:(d + 1) * H], x, y, gates, cs, g("weight_ih"), g("weight_hh"), d == 1)
            dx = dx + dxi
            grads[f"weight_ih_l{l}{s}"], grads[f"weight_hh_l{l}{s}"] = dwi, dwh
            grads[f"bias_ih_l{l}{s}"], grads[f"bias_hh_l{l}{s}"] = db, db
        d_out = dx
    return d_out, grads


def make_lstm(inp, H, layers, bidir, seed, dropout=0.0, scale=1.0):
    """nn.LSTM at its own initialisation; scale = 1.5 (as gru_ref.make_gru has it) takes the gates out of their linear region"""
    torch.manual_seed(seed)
    lstm = torch.nn.LSTM(inp, H, layers, dropout=dropout, bidirectional=bidir, batch_first=True)
    if scale != 1.0:
        with torch.no_grad():
            for p in lstm.parameters():
                p.mul_(scale)
    return lstm
