#!/usr/bin/env python3
"""Vocabulary head: launch time of cvc_packed_linear_fwd (records form) against per-workgroup ingest (M = 32 / 64 batch rows) and grid
size (V), K = 2048 / 1024 -- the measurement behind DESIGN section 4, "Vocabulary head, block shape chosen per launch".
Prints one dict per shape; --out FILE also writes them as JSON.  Usage: python tools/head_probe.py [--out FILE]"""
import os, sys, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cyclical-visual-captioning_amd")]
import torch
from cvc import hip
from cvc.decode import pack_weights, to_quad
L = hip.lib(); dev = torch.device("cuda:0")
st = torch.cuda.current_stream().cuda_stream
res = []
for K in (2048, 1024):
    for V in (5000, 6400, 8000, 8192, 10000):
        w = torch.randn(V, K, device=dev) / K ** 0.5
        wp = pack_weights(w); b = torch.randn(V, device=dev)
        for M in (32, 64):
            xq = to_quad(torch.randn(M, K, device=dev))
            rec = torch.zeros((V + 31) // 32, 64, 6, device=dev)
            call = lambda: L.cvc_packed_linear_fwd(wp.data_ptr(), xq.data_ptr(), K, b.data_ptr(), M, V, 1, None, V, rec.data_ptr(), st)
            for _ in range(20): assert call() == 0
            torch.cuda.synchronize()
            ts = []
            for rep in range(5):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(100): call()
                e1.record(); torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1) * 10.0)      # us per launch
            nwg = (V + 31) // 32
            r = dict(K=K, V=V, M=M, workgroups=nwg, ingest_MB=round(4 * K * (32 + M) / 1e6, 3), us_min=round(min(ts), 2), us_med=round(sorted(ts)[2], 2))
            print(r, flush=True); res.append(r)
if "--out" in sys.argv:
    json.dump(res, open(sys.argv[sys.argv.index("--out") + 1], "w"), indent=1)
