"""Frame-context LSTM of the once-per-clip encoder on the HIP kernels: the `--t_attn_mode bilstm` counterpart of cvc/gru.py
(reference backbone.py:94-106 builds `nn.LSTM(R, R/2, 2, dropout=0.2, bidirectional=True, batch_first=True)`, :335-338 runs it over
the F sampled frames).

A layer is
  1. ONE dense GEMM for the input projections of all F steps and both directions (the tile GEMM, csrc/gemm_tile.hip), and
  2. the recurrence (csrc/lstm_seq.hip), in one of two forms with interchangeable results (equal within rounding, not in bits:
     they sum k in different orders):
     - persistent (cvc_lstm_seq_persistent_fwd; H % 128 == 0, H <= 1024): one launch for the whole sequence, W_hh held in
       registers, the cell state c in the registers of the workgroup that owns the unit, steps separated by a bounded barrier;
     - per step (cvc_lstm_seq_fwd): F launches, any H % 8 == 0 -- the fallback when the persistent form refuses a shape or reports
       a barrier time-out, and the only form for config 5's width (rnn_size 4096 -> H = 2048).
`lstm_forward` is the inference path (no autograd).  `lstm_forward_train` is the same recurrence under autograd: the forward keeps
every step's activated gates and c_t, the backward walks the sequence backwards (cvc_lstm_seq_bwd: gate gradients + dgates W_hh per
step) and takes dX, dW_ih, dW_hh and the biases from dense products over all steps on the tile GEMM.  b_ih and b_hh enter the same
sum, so one gate-gradient matrix serves the input side and the hidden side."""
from __future__ import annotations

import torch
import torch.nn as nn

from . import hip
from .decode import pack_weights

PERSISTENT = True       # False: always the per-step form (A/B switch)
last_form = None        # "persistent" / "steps": which form produced the last inference call (tests, bench)
last_train_form = None  # ... the last autograd layer's forward


def pack_lstm_weights(w_hh: torch.Tensor, H: int) -> torch.Tensor:
    """[4H, H] (i, f, g, o) -> the packed gate tiles [H/8][Kp/4][32][4], columns zero-padded to a multiple of 32: block b, row
    8 g + u = gate g of hidden unit 8 b + u."""
    assert w_hh.shape == (4 * H, H) and H % 8 == 0
    Kp = (H + 31) // 32 * 32
    if Kp != H:
        w = w_hh.new_zeros(4 * H, Kp)
        w[:, :H] = w_hh
        w_hh = w
    return pack_weights(w_hh, lstm_R=H)


def supported(lstm: nn.Module, x: torch.Tensor) -> bool:
    """Shapes / modules the inference path takes."""
    return (isinstance(lstm, nn.LSTM) and lstm.batch_first and lstm.bias and getattr(lstm, "proj_size", 0) == 0
            and lstm.hidden_size % 8 == 0 and x.dim() == 3 and x.is_cuda and x.dtype == torch.float32)


def supported_train(lstm: nn.Module, x: torch.Tensor) -> bool:
    """... the autograd path takes: the same (persistent forward where it exists, the per-step form for every other width)."""
    return supported(lstm, x)


def _sfx(lstm):
    return [""] if not lstm.bidirectional else ["", "_reverse"]


def _layer_operands(lstm: nn.LSTM):
    """Per layer: (W_ih of both directions as a tile operand, packed W_hh [ndir][...], b_ih [ndir, 4H], b_hh [ndir, 4H]);
    rebuilt when any parameter changed."""
    params = list(lstm.parameters())
    # (the generation covers updates that leave _version alone: fused Adam, graph replays -- hip.bump_weights_generation)
    stamp = (hip.weights_generation(),) + tuple((p.data_ptr(), p._version) for p in params)
    ent = getattr(lstm, "_cvc_lstm_pack", None)        # lives on the module (no table keyed by ids / addresses)
    if ent is not None and ent[0] == stamp:
        return ent[1]
    H, sfx = lstm.hidden_size, _sfx(lstm)
    layers = []
    with torch.no_grad():
        for l in range(lstm.num_layers):
            g = lambda n: [getattr(lstm, f"{n}_l{l}{s}").detach().float() for s in sfx]
            w_ih = torch.cat(g("weight_ih"), 0).contiguous()
            layers.append((hip.TileOperand(w_ih, kmajor=False), torch.stack([pack_lstm_weights(w, H) for w in g("weight_hh")]),
                           torch.stack(g("bias_ih")).contiguous(), torch.stack(g("bias_hh")).contiguous()))
    lstm._cvc_lstm_pack = (stamp, layers)
    return layers


def _kp(H: int) -> int:
    return (H + 31) // 32 * 32


def _persistent_shape(H: int) -> bool:
    return H % 128 == 0 and H <= 1024


def lstm_forward(lstm: nn.LSTM, x: torch.Tensor) -> torch.Tensor:
    """x [B, F, in] -> [B, F, ndir * H], the first output of `lstm(x)` (h0 = c0 = 0)."""
    assert supported(lstm, x), "shape / module outside the HIP LSTM's range"
    B, F, _ = x.shape
    H, ndir = lstm.hidden_size, 2 if lstm.bidirectional else 1
    layers = _layer_operands(lstm)
    out = torch.empty(B, F, ndir * H, device=x.device, dtype=torch.float32)
    L, st = hip.lib(), hip._stream()
    global last_form
    # (under capture the error words cannot be read by the host: persistent only in deferred mode)
    try_persistent = PERSISTENT and _persistent_shape(H) and (hip.errors_deferred() or not torch.cuda.is_current_stream_capturing())

    def run(persistent: bool):
        """All chunks and layers in one go; returns the persistent launches' error words (device tensors, not read here)."""
        words = []
        for b0 in range(0, B, 64):
            m = min(64, B - b0)
            cur = x[b0:b0 + m].transpose(0, 1).contiguous().view(F * m, -1)            # time-major rows (t, clip)
            for l, (w_ih, wp, b_ih, b_hh) in enumerate(layers):
                gi = hip.tile_mm(cur, w_ih)                                              # [F*m, ndir*4H], no bias
                if l == len(layers) - 1:
                    y, ld_m, ld_t = out[b0:b0 + m], F * ndir * H, ndir * H
                else:
                    y = torch.empty(F * m, ndir * H, device=x.device, dtype=torch.float32)
                    ld_m, ld_t = ndir * H, m * ndir * H
                head = (wp.data_ptr(), gi.data_ptr(), ndir * 4 * H, m * ndir * 4 * H, b_ih.data_ptr(), b_hh.data_ptr(), m, F, H, ndir)
                if persistent:
                    sync = torch.empty(int(L.cvc_lstm_persistent_sync_words()), device=x.device, dtype=torch.int32)
                    slots = torch.empty((F + 1) * ndir * H * 64, device=x.device, dtype=torch.float32)     # one state slot per step
                    if L.cvc_lstm_seq_persistent_fwd(*head, slots.data_ptr(), y.data_ptr(), ld_m, ld_t, sync.data_ptr(), st) != 0:
                        return None                                                    # launch refused (shape / residency): per-step form
                    words.append(sync[4:5])
                else:
                    hq = torch.empty(3 * ndir * _kp(H) * 64, device=x.device, dtype=torch.float32)
                    hip._check(L.cvc_lstm_seq_fwd(*head, hq.data_ptr(), y.data_ptr(), ld_m, ld_t, st), "cvc_lstm_seq_fwd")
                cur = y
        return words

    if try_persistent:
        # every layer (and 64-clip chunk) is enqueued before the error words are looked at: ONE host read per call; a barrier
        # time-out anywhere leaves its word set and the whole call is redone in the per-step form
        words = run(True)
        if words is not None and hip.error_word_ok(torch.cat(words).abs().sum(dtype=torch.int32).view(1)):
            last_form = "persistent"
            return out
    run(False)
    last_form = "steps"
    return out


# ------------------------------------------------------------------------------------------------ training (autograd)
class _LstmLayer(torch.autograd.Function):
    """One LSTM layer over time-major rows (t * m + clip): x [F*m, in] -> y [F*m, ndir*H]."""

    @staticmethod
    def forward(ctx, x, w_ih, w_hh, b_ih, b_hh, m, F):
        # w_ih [ndir*4H, in], w_hh [ndir, 4H, H], b_ih / b_hh [ndir, 4H]
        ndir, H = w_hh.shape[0], w_hh.shape[2]
        L, st = hip.lib(), hip._stream()
        x, w_ih, w_hh = x.contiguous(), w_ih.contiguous(), w_hh.contiguous()
        b_ih, b_hh = b_ih.contiguous(), b_hh.contiguous()
        gi = hip.tile_mm(x, w_ih)
        wp = torch.stack([pack_lstm_weights(w_hh[d], H) for d in range(ndir)])
        y = torch.empty(F * m, ndir * H, device=x.device, dtype=torch.float32)
        c = torch.empty_like(y)
        gates = torch.empty(F * m, ndir * 4 * H, device=x.device, dtype=torch.float32)
        head = (wp.data_ptr(), gi.data_ptr(), ndir * 4 * H, m * ndir * 4 * H, b_ih.data_ptr(), b_hh.data_ptr(), m, F, H, ndir)
        tail = (y.data_ptr(), ndir * H, m * ndir * H, gates.data_ptr(), ndir * 4 * H, m * ndir * 4 * H, c.data_ptr(), ndir * H, m * ndir * H)
        global last_train_form
        done = False
        if PERSISTENT and _persistent_shape(H):
            sync = torch.empty(int(L.cvc_lstm_persistent_sync_words()), device=x.device, dtype=torch.int32)
            slots = torch.empty((F + 1) * ndir * H * 64, device=x.device, dtype=torch.float32)
            rc = L.cvc_lstm_seq_persistent_train_fwd(*head, slots.data_ptr(), *tail, sync.data_ptr(), st)
            # (eagerly a host read: a barrier time-out repeats the layer in the per-step form; in deferred mode -- captured training
            # steps, cvc.hip.defer_errors -- the word is OR-ed into the step's status word and the step is re-run later if it was set)
            done = rc == 0 and hip.error_word_ok(sync[4:5])
        if not done:
            hq = torch.empty(3 * ndir * _kp(H) * 64, device=x.device, dtype=torch.float32)
            hip._check(L.cvc_lstm_seq_train_fwd(*head, hq.data_ptr(), *tail, st), "cvc_lstm_seq_train_fwd")
        last_train_form = "persistent" if done else "steps"
        ctx.save_for_backward(x, w_ih, w_hh, gates, c, y)
        ctx.dims = (m, F, H, ndir)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w_ih, w_hh, gates, c, y = ctx.saved_tensors
        m, F, H, ndir = ctx.dims
        L, st = hip.lib(), hip._stream()
        dy = dy.contiguous()
        dg = torch.empty(F * m, ndir * 4 * H, device=x.device, dtype=torch.float32)
        work = torch.empty(int(L.cvc_lstm_seq_bwd_work(m, H, ndir)), device=x.device, dtype=torch.float32)
        hip._check(L.cvc_lstm_seq_bwd(dy.data_ptr(), ndir * H, m * ndir * H, gates.data_ptr(), ndir * 4 * H, m * ndir * 4 * H, c.data_ptr(),
                                      ndir * H, m * ndir * H, w_hh.data_ptr(), m, F, H, ndir, dg.data_ptr(), work.data_ptr(), st),
                   "cvc_lstm_seq_bwd")
        ni = ctx.needs_input_grad
        d_x = hip.tile_mm(dg, w_ih, b_kmajor=True) if ni[0] else None          # [F*m, in]
        d_w_ih = hip.tile_mm(hip.TileOperand(dg, kmajor=True), x, b_kmajor=True) if ni[1] else None      # [ndir*4H, in]
        d_w_hh = None
        if ni[2]:
            zeros = y.new_zeros(m, H)
            parts = []
            for d in range(ndir):
                yd = y[:, d * H:(d + 1) * H]
                hp = torch.cat((zeros, yd[:-m]), 0) if d == 0 else torch.cat((yd[m:], zeros), 0)     # h_{t-1} of this direction
                parts.append(hip.tile_mm(dg[:, d * 4 * H:(d + 1) * 4 * H], hp, a_kmajor=True, b_kmajor=True))
            d_w_hh = torch.stack(parts)
        d_b = dg.sum(0).view(ndir, 4 * H) if (ni[3] or ni[4]) else None
        return d_x, d_w_ih, d_w_hh, (d_b if ni[3] else None), (d_b if ni[4] else None), None, None


def lstm_forward_train(lstm: nn.LSTM, x: torch.Tensor) -> torch.Tensor:
    """`lstm(x)[0]` under autograd on the HIP kernels (h0 = c0 = 0; inter-layer dropout as the module has it)."""
    assert supported_train(lstm, x), "shape / module outside the HIP LSTM's autograd range"
    B, F, _ = x.shape
    H, ndir = lstm.hidden_size, 2 if lstm.bidirectional else 1
    sfx = _sfx(lstm)
    outs = []
    for b0 in range(0, B, 64):
        m = min(64, B - b0)
        cur = x[b0:b0 + m].transpose(0, 1).reshape(F * m, -1)                       # time-major rows (t, clip)
        for l in range(lstm.num_layers):
            g = lambda n: [getattr(lstm, f"{n}_l{l}{s}") for s in sfx]
            cur = _LstmLayer.apply(cur, torch.cat(g("weight_ih"), 0), torch.stack(g("weight_hh")), torch.stack(g("bias_ih")),
                                   torch.stack(g("bias_hh")), m, F)
            if lstm.training and lstm.dropout > 0 and l + 1 < lstm.num_layers:
                # nn.LSTM's inter-layer dropout with the mask of site enc.lstm.<l> from the in-kernel generator (cvc/dropout.py)
                from . import dropout as _dropout
                cur = _dropout.apply_p(cur, lstm.dropout, "enc.lstm.%d" % l)
        outs.append(cur.view(F, m, ndir * H).transpose(0, 1))
    return torch.cat(outs, 0) if len(outs) > 1 else outs[0].contiguous()
