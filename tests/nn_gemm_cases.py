"""Shared pieces of tests/test_gpu_nn_gemm.py and tests/test_nn_gemm_cpu.py (not collected: no test_ prefix): the K-loop and
K-slice arithmetic of csrc/gemm_nn.hip (the backward-data GEMM dX[M <= 64, N] = dY[M, K] W[K, N]) restated from its constants,
case builders, fp64 restatements, and C-ABI callers of its four entry points cvc_linear_nn_fwd, cvc_linear_nn_planes_fwd,
cvc_linear_nn_planes2_fwd and cvc_pack_quad, as cvc/hip.py, csrc/train_driver.hip and the sequence backwards call them.

Everything above the "device side" line runs on the CPU; the callers below it pre-fill every output with NaN and give every
output one row and four columns (a plane workspace: one plane) more than the contract writes."""
import math
import os
import re

import torch

from packed_gemm_cases import OP_TOL, all_nan, close, nan_buf, same_bits, split_mode, stream_handle, wave_counts  # noqa: F401  (re-exported)
from skinny_gemm_cases import mixed_magnitude_case  # noqa: F401  (re-exported)

E_BADARG = -1                                    # include/cvc_hip.h
MAXSEG = 6                                       # NN_MAX_SEG
ROWS = (1, 32, 33, 64)                           # one row tile (MT = 1) and two (MT = 2): the tile boundary and its far ends
MODES = (0, 1, 2)                                # cvc_gemm_packed_split: 0 = fp32-MFMA kernel, 1 and 2 = the split-product kernel

# K / 8 of the K-loop sweep (section 1 of the GPU file), ksplit = 1.  Wave w of NW = 4 takes the 8-row groups w, w + 4, ...:
# n_my = ceil((K / 8 - w) / 4), so 1 -> (1, 0, 0, 0) and 8 n + 6 -> (2 n + 2, 2 n + 2, 2 n + 1, 2 n + 1): together every n_my in 0 .. 24.
#   fp32 kernel (ring depth 3 over n_my): simple 0, 1, 2 | ring without a pass, rest 3, 4 | one pass, rest 2, 3, 4 | two passes, ...
#   split kernel (ring depth 4 over n_my >> 1, n_my & 1 on the fp32 MFMA): simple 0 .. 3 | no pass, rest 4, 5, 6 | one pass, rest
#     3 .. 6 | two passes, rest 3 -- each with both parities of n_my
#   128-row kernel (ring depth 3 over n_my >> 1): simple 0 .. 2 | no pass, rest 3, 4 | one pass, rest 2, 3, 4 | two passes, rest 2 --
#     each with both parities
# tests/test_nn_gemm_cpu.py checks all of it against the constants of the source.
SWEEP_GROUPS = (1, 6, 14, 22, 30, 38, 46, 54, 62, 70, 78, 86, 94)

# (K / 8, requested ksplit) of the K-slice cases (section 2 of the GPU file); (3, 64) is clamped to 3 slices
SLICE_CASES = ((5, 5), (11, 3), (23, 4), (47, 2), (94, 3), (3, 64))
SLICE_WIDTHS = (132, 36)
SIX_WIDTHS = (4, 128, 132, 256, 36, 260)         # NN_MAX_SEG segments: one quad, one full slab, ragged second / third slabs


# ------------------------------------------------------------------ the K loop's and the K slices' arithmetic, from the source
def source_path():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return os.path.join(root, "cyclical-visual-captioning_amd", "csrc", "gemm_nn.hip")


def source_constants(path=None):
    """NN_MAX_SEG, the three ring depths (the defaults of CVC_NN_DEPTH, CVC_NNS_DEPTH and CVC_NN128_DEPTH, and that each kernel
    takes its depth from its own macro) and the waves per workgroup of the three GEMM kernels, read from csrc/gemm_nn.hip"""
    src = open(path or source_path()).read()
    define = lambda name: int(re.search(r"#ifndef\s+" + name + r"\s*\n\s*#define\s+" + name + r"\s+(\d+)", src).group(1))
    nw = lambda kern: int(re.search(kern + r"\(NNArgs a\)\s*\{\s*constexpr\s+int\s+NW\s*=\s*(\d+)\s*[,;]", src).group(1))
    assert re.search(r"constexpr\s+int\s+NN_DEPTH\s*=\s*CVC_NN_DEPTH\s*;", src)
    assert re.search(r"skinny_gemm_nn_split_kernel\(NNArgs a\)\s*\{\s*constexpr\s+int\s+NW\s*=\s*\d+\s*;\s*constexpr\s+int\s+D\s*=\s*CVC_NNS_DEPTH\s*;", src)
    assert re.search(r"skinny_gemm_nn_split128_kernel\(NNArgs a\)\s*\{\s*constexpr\s+int\s+NW\s*=\s*\d+\s*,\s*MT\s*=\s*4\s*,\s*D\s*=\s*CVC_NN128_DEPTH\s*;", src)
    return dict(NN_MAX_SEG=int(re.search(r"constexpr\s+int\s+NN_MAX_SEG\s*=\s*(\d+)\s*;", src).group(1)),
                CVC_NN_DEPTH=define("CVC_NN_DEPTH"), CVC_NNS_DEPTH=define("CVC_NNS_DEPTH"), CVC_NN128_DEPTH=define("CVC_NN128_DEPTH"),
                NW_FP32=nw("skinny_gemm_nn_kernel"), NW_SPLIT=nw("skinny_gemm_nn_split_kernel"), NW_SPLIT128=nw("skinny_gemm_nn_split128_kernel"))


def ring_branch(n, depth):
    """what a register ring of `depth` does with n steps: ("simple", n) below the depth (load, multiply, one step at a time), else
    ("ring", passes of the steady loop, steps left to the tail): j advances by depth while j + 2 depth - 1 <= n"""
    if n < depth:
        return ("simple", n)
    j = 0
    while j + 2 * depth - 1 <= n:
        j += depth
    return ("ring", j // depth, n - j)


def fp32_branch(n_my, cs):
    """skinny_gemm_nn_kernel: the ring runs over the wave's 8-row groups"""
    return ring_branch(n_my, cs["CVC_NN_DEPTH"])


def split_branch(n_my, cs):
    """skinny_gemm_nn_split_kernel: the ring runs over double groups, an odd last group takes the fp32-MFMA step -> (ring, n_my & 1)"""
    return (ring_branch(n_my >> 1, cs["CVC_NNS_DEPTH"]), n_my & 1)


def split128_branch(n_my, cs):
    """skinny_gemm_nn_split128_kernel: as the split kernel, with its own depth"""
    return (ring_branch(n_my >> 1, cs["CVC_NN128_DEPTH"]), n_my & 1)


def sweep_branches(cs, groups=SWEEP_GROUPS):
    """the branches SWEEP_GROUPS reaches at ksplit = 1 -> dict(fp32=set, split=set, split128=set)"""
    seen = dict(fp32=set(), split=set(), split128=set())
    for G in groups:
        seen["fp32"] |= {fp32_branch(n, cs) for n in wave_counts(G, cs["NW_FP32"])}
        seen["split"] |= {split_branch(n, cs) for n in wave_counts(G, cs["NW_SPLIT"])}
        seen["split128"] |= {split128_branch(n, cs) for n in wave_counts(G, cs["NW_SPLIT128"])}
    return seen


def wanted_branches():
    """what the sweep has to reach (the issue's list; the kernels have no other branches below three passes)"""
    both = lambda rings: {(r, odd) for r in rings for odd in (0, 1)}
    simple = lambda ns: [("simple", n) for n in ns]
    ring = lambda passes, rests: [("ring", passes, r) for r in rests]
    return dict(fp32=set(simple((0, 1, 2)) + ring(0, (3, 4)) + ring(1, (2, 3, 4)) + ring(2, (2,))),
                split=both(simple((0, 1, 2, 3)) + ring(0, (4, 5, 6)) + ring(1, (3, 4, 5, 6)) + ring(2, (3,))),
                split128=both(simple((0, 1, 2)) + ring(0, (3, 4)) + ring(1, (2, 3, 4)) + ring(2, (2,))))


def slice_groups(G, ksplit):
    """[g_lo, g_hi) of every K slice of G = K / 8 groups: a requested ksplit > G is clamped to G, then slice s owns the groups
    [G s / ksplit, G (s + 1) / ksplit)"""
    eff = min(ksplit, G)
    return [(G * s // eff, G * (s + 1) // eff) for s in range(eff)]


def plane_layout(widths):
    """the slab-padded columns of a plane -> (ntot = 128 * sum of ceil(ncols / 128), first column of every segment = 128 * slab0)"""
    starts, slab = [], 0
    for n in widths:
        starts.append(128 * slab)
        slab += (n + 127) // 128
    return 128 * slab, starts


# ------------------------------------------------------------------ cases and fp64 restatements (CPU tensors, fixed seeds)
def nn_case(seed, M, K, N):
    """dY [M, K] ~ N(0, 1), W [K, N] ~ N(0, 1) / sqrt(K): unit-scale outputs at every K"""
    g = torch.Generator().manual_seed(seed)
    return dict(M=M, K=K, N=N, dy=torch.randn(M, K, generator=g), w=torch.randn(K, N, generator=g) / math.sqrt(K))


def nn_ref(dy, w):
    return dy.double() @ w.double()


def slice_refs(dy, w, ksplit):
    """fp64 restatement of the plane form: plane s is the product over the K rows [8 g_lo, 8 g_hi) of slice s -> [ksplit_eff] of [M, N]"""
    return [dy[:, 8 * lo:8 * hi].double() @ w[8 * lo:8 * hi].double() for lo, hi in slice_groups(dy.shape[1] // 8, ksplit)]


def host_quad(x):
    """row-major [M <= 64, K] -> the quad layout [K/4][64][4], rows >= M exactly +0.0 (what cvc_pack_quad has to write)"""
    M, K = x.shape
    q = torch.zeros(K // 4, 64, 4, dtype=x.dtype)
    q[:, :M] = x.reshape(M, K // 4, 4).permute(1, 0, 2)
    return q


def mixed_nn_case(M, K, N):
    """mixed_magnitude_case in this product's operand order: its stripes are on the K index of both operands already
    (dY[:, 5::13] * 1e18 against W[5::13, :] * 1e-18, and so on), the signed-zero row is row 0 of dY"""
    c = mixed_magnitude_case(M, K, N)
    return dict(M=M, K=K, N=N, dy=c["x"], w=c["w"].t().contiguous())


# ================================================================== device side
def device_quad(hip, x):
    """cvc_pack_quad on a contiguous device tensor [M, K] -> [K/4][64][4]"""
    M, K = x.shape
    xq = nan_buf(K // 4, 64, 4, dev=x.device)
    rc = hip.lib().cvc_pack_quad(x.data_ptr(), x.stride(0), M, K, xq.data_ptr(), stream_handle())
    torch.cuda.synchronize()
    assert rc == 0, rc
    return xq


def run_pack_quad(hip, dev, x):
    """cvc_pack_quad reading x [M, K] (CPU) as columns 4 .. K + 4 of a NaN-filled [M + 1, K + 8] tensor (ldx = K + 8) into a
    NaN-filled [K/4 + 1][64][4] buffer -> (rc, buffer)"""
    M, K = x.shape
    src = nan_buf(M + 1, K + 8, dev=dev)
    src[:M, 4:4 + K] = x.to(dev)
    xq = nan_buf(K // 4 + 1, 64, 4, dev=dev)
    rc = hip.lib().cvc_pack_quad(src[:, 4:].data_ptr(), src.stride(0), M, K, xq.data_ptr(), stream_handle())
    torch.cuda.synchronize()
    return rc, xq


class Weights:
    """The weight side of a call: segment s (width widths[s]) is columns 8 + c0_s .. of matrix s % nmat, c0_s the segment's first
    column in w [K, sum(widths)]; every matrix is [K, sum(widths) + 16] and NaN wherever no segment of its own lies (ldw > sum of
    all widths, non-zero column offsets, and a read outside a segment's columns poisons the output)."""

    def __init__(self, dev, w, widths, nmat=1):
        K, N = w.shape
        assert N == sum(widths) and len(widths) <= MAXSEG
        self.widths, self.ld = tuple(widths), N + 16
        self.mats = [nan_buf(K, N + 16, dev=dev) for _ in range(nmat)]
        self.views, self.c0, c0 = [], [], 0
        for s, n in enumerate(widths):
            m = self.mats[s % nmat]
            m[:, 8 + c0:8 + c0 + n] = w[:, c0:c0 + n].to(dev)
            self.views.append(m[:, 8 + c0:8 + c0 + n])
            self.c0.append(c0)
            c0 += n


def run_nn(hip, entry, dyq, K, M, wts, ksplit=1, dyq2=None, M2=None, reduce=1, null_ws=False):
    """One launch of cvc_linear_nn_fwd ("fwd"), cvc_linear_nn_planes_fwd ("planes") or cvc_linear_nn_planes2_fwd ("planes2").
    Every segment's dst is columns 0 .. ncols of its own NaN-filled [rows + 1, ncols + 4] tensor (rows = M, or 128 in the 128-row
    form); the workspace, passed whenever the requested ksplit > 1 (null_ws: never), is NaN-filled and holds one plane more than
    the REQUESTED ksplit.  -> (rc, [dst buffers], workspace [ksplit + 1, rows, ntot] or None)"""
    dev = dyq.device
    rows = 128 if entry == "planes2" else M
    ntot, _ = plane_layout(wts.widths)
    dsts = [nan_buf(rows + 1, n + 4, dev=dev) for n in wts.widths]
    arr = (hip.NNSeg * len(wts.widths))()
    for s, (v, d, n) in enumerate(zip(wts.views, dsts, wts.widths)):
        arr[s] = hip.NNSeg(v.data_ptr(), d.data_ptr(), v.stride(0), n, d.stride(0))
    ws = None if (ksplit <= 1 or null_ws) else nan_buf(ksplit + 1, rows, ntot, dev=dev)
    wsp = None if ws is None else ws.data_ptr()
    L, st = hip.lib(), stream_handle()
    if entry == "fwd":
        rc = L.cvc_linear_nn_fwd(dyq.data_ptr(), K, M, arr, len(wts.widths), ksplit, wsp, st)
    elif entry == "planes":
        rc = L.cvc_linear_nn_planes_fwd(dyq.data_ptr(), K, M, arr, len(wts.widths), ksplit, wsp, st)
    else:
        assert entry == "planes2"
        rc = L.cvc_linear_nn_planes2_fwd(dyq.data_ptr(), dyq2.data_ptr(), K, M, M2, arr, len(wts.widths), ksplit, wsp, reduce, st)
    torch.cuda.synchronize()
    return rc, dsts, ws


def _err(tag, got, ref, tol):
    assert bool(torch.isfinite(got).all()), (tag, "unwritten or non-finite element")
    err = float((got.double() - ref.to(got.device)).abs().max())
    close(got, ref.float(), err_msg=tag, **tol)
    return err


def check_dsts(tag, dsts, ref, M, wts, tol=OP_TOL, row0=0, rows_nan=None):
    """the dst buffers of a launch against fp64 ref [M, sum(widths)]: rows row0 .. row0 + M of every segment written and within
    tol, columns >= ncols still NaN, and so are the rows rows_nan = (lo, hi) (default: everything from row M on).  -> max |err|"""
    err = 0.0
    lo, hi = rows_nan or (row0 + M, None)
    for s, (d, n, c0) in enumerate(zip(dsts, wts.widths, wts.c0)):
        assert all_nan(d[:, n:]) and all_nan(d[lo:hi]), (tag, s, "wrote outside the rows and columns of dst it owns")
        err = max(err, _err(f"{tag} segment {s}", d[row0:row0 + M, :n], ref[:, c0:c0 + n], tol))
    print(f"nn_gemm {tag}: max |err| = {err:.3e}")
    return err


def dst_values(dsts, wts, M, row0=0):
    """the written part of every dst buffer, for the bitwise comparisons"""
    return [d[row0:row0 + M, :n] for d, n in zip(dsts, wts.widths)]


def dsts_untouched(dsts):
    return all(all_nan(d) for d in dsts)


def check_planes(tag, ws, refs, M, wts, rows=None, row0=0, tol=OP_TOL):
    """the workspace [ksplit requested + 1, rows, ntot] of a plane launch, read as the contract lays it out -- [ksplit_eff][rows][ntot]
    from its start -- against the fp64 slice products refs ([ksplit_eff] of [M, sum(widths)]) on rows row0 .. row0 + M; the
    slab-padding columns of these rows are still NaN.  What lies behind plane ksplit_eff - 1, and the rows nobody owns, are the
    caller's to check (planes_rest_is_nan).  -> (planes view [ksplit_eff, rows, ntot], max |err|)"""
    rows = M if rows is None else rows
    eff = len(refs)
    ntot, starts = plane_layout(wts.widths)
    planes = ws.reshape(-1)[:eff * rows * ntot].view(eff, rows, ntot)
    err = 0.0
    for k in range(eff):
        own = planes[k, row0:row0 + M]
        for s, (n, c0, p0) in enumerate(zip(wts.widths, wts.c0, starts)):
            p1 = starts[s + 1] if s + 1 < len(starts) else ntot
            assert all_nan(own[:, p0 + n:p1]), (tag, k, s, "slab padding was written")
            err = max(err, _err(f"{tag} plane {k} segment {s}", own[:, p0:p0 + n], refs[k][:, c0:c0 + n], tol))
    print(f"nn_gemm {tag}: planes max |err| = {err:.3e}")
    return planes, err


def planes_rest_is_nan(ws, eff, rows, ntot):
    """everything behind the ksplit_eff planes the contract writes"""
    return all_nan(ws.reshape(-1)[eff * rows * ntot:])


def plane_sum(planes, wts, M, row0=0):
    """the consumer's sum, in plane order and in fp32 (v = p0; v += p1; ...) -> per segment [M, ncols]"""
    _, starts = plane_layout(wts.widths)
    out = []
    for n, p0 in zip(wts.widths, starts):
        v = planes[0, row0:row0 + M, p0:p0 + n].clone()
        for k in range(1, planes.shape[0]):
            v += planes[k, row0:row0 + M, p0:p0 + n]
        out.append(v)
    return out


def all_same_bits(xs, ys):
    return len(xs) == len(ys) and all(same_bits(x, y) for x, y in zip(xs, ys))
