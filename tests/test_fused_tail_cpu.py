"""Host side of the fused greedy tail's tests: the key encoding that tests/test_gpu_fused_tail.py builds its hand-made keys with
(csrc/sel_keys.h restated in Python) orders candidates as the device code documents.  No GPU."""
import math

from test_gpu_fused_tail import host_key


def test_host_key_order():
    vals = [-3e38, -3.5, -1e-30, -0.0, 0.0, 1e-30, 2.0, math.inf]
    ks = [host_key(v, 5) for v in vals]
    assert ks == sorted(ks) and ks[3] == ks[4] and ks[0] > 0
    assert host_key(math.nan, 5) == 0 and host_key(-math.inf, 5) == 0
    assert host_key(1.0, 3) > host_key(1.0, 4) > host_key(0.5, 0)
