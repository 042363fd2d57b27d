"""CPU cross-checks of the fp64 references tests/test_gpu_train_kernels.py holds the training kernels to: each reference against
torch's own module or functional form of the same operation."""
import torch
import torch.nn.functional as F

from test_gpu_train_kernels import attn_fwd_ref, lstm_cell_state, lstm_gates_bwd_ref, nll_head_ref


def test_gate_gradient_reference_matches_lstmcell_autograd():
    """lstm_gates_bwd_ref (gradients w.r.t. the pre-activations z and c_prev) against nn.LSTMCell autograd: its z is the cell's
    x W_ih^T + b_ih + h W_hh^T + b_hh, so dz summed over rows is the bias gradient, dz W_ih the input gradient, and dc_prev is
    the cell state's gradient"""
    torch.manual_seed(0)
    M, E, R = 5, 6, 7
    cell = torch.nn.LSTMCell(E, R).double()
    x, h0, c0 = torch.randn(M, E, dtype=torch.float64, requires_grad=True), torch.randn(M, R, dtype=torch.float64), \
        torch.randn(M, R, dtype=torch.float64, requires_grad=True)
    dh, dc = torch.randn(M, R, dtype=torch.float64), torch.randn(M, R, dtype=torch.float64)
    h, c = cell(x, (h0, c0))
    torch.autograd.backward([h, c], [dh, dc])
    with torch.no_grad():
        z = x @ cell.weight_ih.t() + cell.bias_ih + h0 @ cell.weight_hh.t() + cell.bias_hh
        gates, c_new = lstm_cell_state(z, c0)
    torch.testing.assert_close(c_new, c.detach())
    torch.testing.assert_close(gates[:, 3 * R:] * torch.tanh(c_new), h.detach())
    dz, dcp = lstm_gates_bwd_ref(z, c0, dh, dc)
    torch.testing.assert_close(dz.sum(0), cell.bias_ih.grad)
    torch.testing.assert_close(dz.t() @ x.detach(), cell.weight_ih.grad)
    torch.testing.assert_close(dz @ cell.weight_ih.detach(), x.grad)
    torch.testing.assert_close(dcp, c0.grad)


def test_attention_reference_matches_loop_form():
    """attn_fwd_ref's einsum forms against a per-clip, per-query loop of the formulas (additive w_a . tanh(proj + q), dot
    (proj . q) * inv_temp; softmax over n; the contexts summed over the sets)"""
    torch.manual_seed(1)
    nclip, nq, A, R = 3, 2, 8, 5
    q = torch.randn(nclip, nq, A, dtype=torch.float64)
    w = torch.randn(A, dtype=torch.float64)
    sets = [(torch.randn(nclip, n, A, dtype=torch.float64), torch.randn(nclip, n, R, dtype=torch.float64)) for n in (4, 7)]
    for kind in (0, 1):
        scores, attns, ctx = attn_fwd_ref(kind, q, w, 0.6, sets)
        for c in range(nclip):
            for t in range(nq):
                total = torch.zeros(R, dtype=torch.float64)
                for (proj, cf), s, a in zip(sets, scores, attns):
                    e = torch.tanh(proj[c] + q[c, t]) @ w if kind == 0 else (proj[c] @ q[c, t]) * 0.6
                    torch.testing.assert_close(s[c, t], e)
                    torch.testing.assert_close(a[c, t], torch.softmax(e, 0))
                    total = total + torch.softmax(e, 0) @ cf[c]
                torch.testing.assert_close(ctx[c, t], total)


def test_head_criterion_reference_matches_autograd():
    """nll_head_ref's pre = w * (softmax - onehot) is the gradient of its loss w.r.t. the logits; its argmax takes the lowest of
    tied indices"""
    torch.manual_seed(2)
    M, V = 6, 11
    logits = torch.randn(M, V, dtype=torch.float64, requires_grad=True)
    target = torch.randint(0, V, (M,))
    w = torch.tensor([1.0, 0.0, 0.5, 1.0, 0.0, 2.0])
    loss, amax, pre = nll_head_ref(logits, target, w)
    loss.backward()
    torch.testing.assert_close(pre.detach(), logits.grad)
    torch.testing.assert_close(loss.detach(), F.nll_loss(torch.log_softmax(logits.detach(), 1), target, reduction="none").mul(w.double()).sum())
    tied = torch.zeros(2, 5, dtype=torch.float64)
    tied[0, 3] = tied[0, 1] = 1.0
    assert nll_head_ref(tied, torch.zeros(2, dtype=torch.int64), torch.ones(2))[1].tolist() == [1, 0]
