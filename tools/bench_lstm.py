#!/usr/bin/env python3
"""The `bilstm` frame encoder's recurrence against the library module, measured in one process (GPU box) at config-2 encoder size
(B = 64 clips, F = 480 frames, R = 2048 -> H = 1024, 2 layers, both directions):

  inference   cvc.lstm_seq.lstm_forward in its persistent form, in its per-step form, and nn.LSTM (MIOpen);
  training    forward + backward of cvc.lstm_seq.lstm_forward_train and of nn.LSTM under autograd.

The contenders of a group are timed in alternating rounds (median of the rounds), so clock and cache drift fall on all alike.
Also: the per-step time of the persistent kernel alone (cvc_lstm_seq_persistent_fwd, input projections excluded).
Prints one JSON line.

  python tools/bench_lstm.py [--rounds 5] [--B 64 --F 480 --R 2048 --layers 2]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "cyclical-visual-captioning_amd"))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternate(fns, rounds):
    for f in fns.values():                  # warm-up (weight packs, MIOpen's find step, allocator)
        f()
        f()
    res = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            res[k].append(timed(f))
    return {k: float(np.median(v)) for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--F", type=int, default=480)
    ap.add_argument("--R", type=int, default=2048)
    ap.add_argument("--layers", type=int, default=2)
    args = ap.parse_args()
    from cvc import hip, lstm_seq as LS
    dev = torch.device("cuda:0")
    B, F, R, H = args.B, args.F, args.R, args.R // 2
    torch.manual_seed(1)
    lstm = torch.nn.LSTM(R, H, args.layers, dropout=0.2, bidirectional=True, batch_first=True).to(dev).eval()
    x = torch.randn(B, F, R, device=dev)
    out = {"metric": "ms per call, bilstm frame encoder vs nn.LSTM (MIOpen)", "unit": "ms", "lib": hip.version(),
           "shape": dict(B=B, F=F, R=R, H=H, layers=args.layers, ndir=2)}

    # ---- inference
    forms = {}

    def hip_fwd(persistent):
        def f():
            LS.PERSISTENT = persistent
            try:
                with torch.no_grad():
                    LS.lstm_forward(lstm, x)
                forms[persistent] = LS.last_form
            finally:
                LS.PERSISTENT = True
        return f

    def lib_fwd():
        with torch.no_grad():
            lstm(x)
    lstm.flatten_parameters()
    inf = alternate({"persistent": hip_fwd(True), "steps": hip_fwd(False), "library": lib_fwd}, args.rounds)
    out["inference"] = dict({k: round(v, 3) for k, v in inf.items()}, forms=[forms.get(True), forms.get(False)],
                            hip_over_library=round(inf["persistent"] / inf["library"], 3))       # (default path: see forms[0])

    # ---- the persistent kernel alone: us per step
    L, st = hip.lib(), hip._stream()
    m = min(B, 64)
    wp = torch.stack([LS.pack_lstm_weights(torch.randn(4 * H, H, device=dev) / H ** 0.5, H) for _ in range(2)])
    gi = torch.randn(F * m, 2 * 4 * H, device=dev)
    b1, b2 = torch.randn(2, 4 * H, device=dev) * 0.1, torch.randn(2, 4 * H, device=dev) * 0.1
    y = torch.empty(F * m, 2 * H, device=dev)
    slots = torch.empty((F + 1) * 2 * H * 64, device=dev)
    sync = torch.empty(int(L.cvc_lstm_persistent_sync_words()), device=dev, dtype=torch.int32)

    def kernel():
        rc = L.cvc_lstm_seq_persistent_fwd(wp.data_ptr(), gi.data_ptr(), 8 * H, m * 8 * H, b1.data_ptr(), b2.data_ptr(), m, F, H, 2,
                                           slots.data_ptr(), y.data_ptr(), 2 * H, m * 2 * H, sync.data_ptr(), st)
        assert rc == 0, rc
    if H % 128 == 0 and H <= 1024:
        k = alternate({"kernel": kernel}, args.rounds)["kernel"]
        assert int(sync[4]) == 0
        out["persistent_kernel_us_per_step"] = round(k * 1e3 / F, 2)

    # ---- training: forward + backward
    lstm.train()
    xg = x.clone().requires_grad_(True)
    probe = torch.randn(B, F, 2 * H, device=dev)

    def clear():
        xg.grad = None
        for p in lstm.parameters():
            p.grad = None

    def hip_train():
        clear()
        (LS.lstm_forward_train(lstm, xg) * probe).sum().backward()

    def lib_train():
        clear()
        (lstm(xg)[0] * probe).sum().backward()
    tr = alternate({"hip": hip_train, "library": lib_train}, args.rounds)
    out["train_fwd_bwd"] = dict({k: round(v, 3) for k, v in tr.items()}, form=LS.last_train_form,
                                hip_over_library=round(tr["hip"] / tr["library"], 3))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
