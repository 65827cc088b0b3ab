"""GPU: the two self-critical-training kernels alone - acvae_scst_loss_fwd (mask, coef, loss in a fixed order) and
acvae_logprob_bwd (d sampled_logprobs -> d logits) - against float64 torch autograd of the reference's loss line
``-(lp.gather(w) * reward[:, None] * mask).sum(1).mean()`` (utils/train_util.py:401-409).

Bounds: the close(rtol, atol) pairs tests/test_ops_gpu.py::test_g3_ce_golden_and_backward applies to the same arithmetic
(softmax minus one-hot times a row weight): 1e-6 / 1e-5 on the loss (acvae_ls_ce_fwd), 1e-4 / 1e-7 on d_logits
(acvae_ls_ce_bwd), 1e-5 / 1e-6 on coef."""
import pytest
import torch

import acvae_oracle as O
from acvae_amd import _lib
from parity_util import close

pytestmark = pytest.mark.gpu
END = O.END_IDX


def S():
    return _lib.current_stream()


def _case(V, seed, N=7, T=9):
    """Rows that finish at step 0, at step 1 and never, a reward of exactly 0, rewards in [-1, 1]."""
    g = torch.Generator().manual_seed(seed)
    logits = 3 * torch.randn(N, T, V, generator=g)
    seqs = torch.randint(3, V, (N, T), generator=g)
    seqs[0, 0:] = END                                   # <end> at step 0: only step 0 counts
    seqs[1, 1:] = END                                   # <end> at step 1
    seqs[2, 4:] = END
    seqs[5, T - 1] = END                                # <end> as the last word: every step counts
    reward = torch.rand(N, generator=g) * 2 - 1
    reward[3] = 0.0
    reward[4], reward[6] = 1.0, -1.0
    return logits, seqs, reward


def _reference(logits, seqs, reward):
    x = logits.double().requires_grad_(True)
    lp = torch.log_softmax(x, -1)
    mask = (seqs != END).double()
    mask = torch.cat([torch.ones(mask.size(0), 1, dtype=torch.double), mask[:, :-1]], 1)
    slp = lp.gather(2, seqs.unsqueeze(-1)).squeeze(-1)
    loss = -(slp * reward.double()[:, None] * mask).sum(1).mean()
    loss.backward()
    coef = -(reward.double()[:, None] * mask) / logits.shape[0]
    return loss.detach(), coef, x.grad, slp.detach()


def _run(logits_d, seqs_d, reward_d, N, T, V):
    lse, slp = torch.empty(N, T, device="cuda"), torch.empty(N, T, device="cuda")
    am = torch.empty(N, T, dtype=torch.long, device="cuda")
    _lib.call("acvae_row_logsoftmax_argmax", logits_d, T * V, V, am, None, lse, T, 1, N, T, V, S())
    slp = (logits_d.gather(2, seqs_d.unsqueeze(-1)).squeeze(-1) - lse).contiguous()     # the rollout's sampled_logprobs
    coef, loss = torch.empty(N, T, device="cuda"), torch.empty(1, device="cuda")
    _lib.call("acvae_scst_loss_fwd", slp, seqs_d, reward_d, END, coef, loss, N, T, S())
    dl = torch.full((N, T, V), float("nan"), device="cuda")
    _lib.call("acvae_logprob_bwd", logits_d, V, lse, seqs_d, coef, dl, N * T, V, S())
    return loss, coef, dl


@pytest.mark.parametrize("V", [50, 4367, 5000])
def test_scst_loss_and_logprob_backward_vs_float64_autograd(V):
    logits, seqs, reward = _case(V, seed=V)
    N, T, _ = logits.shape
    want_loss, want_coef, want_dl, _ = _reference(logits, seqs, reward)
    dead = want_coef == 0
    assert bool(dead[0, 1:].all()) and not bool(dead[0, 0]) and bool(dead[1, 2:].all()) and not bool(dead[1, :2].any())
    assert bool(dead[3].all()) and not bool(dead[4].any()) and not bool(dead[5].any())
    # rows whose coef is 0 hold NaN logits: they must come out as zeros, and the loss must not see them
    poisoned = logits.clone()
    poisoned[dead] = float("nan")
    lg, sq, rw = poisoned.cuda(), seqs.cuda(), reward.cuda()
    loss, coef, dl = _run(lg, sq, rw, N, T, V)
    torch.cuda.synchronize()
    print(f"V={V}: loss {float(loss):.7f} (float64 {float(want_loss):.7f}), max |d_logits err| "
          f"{float((dl.cpu().double() - want_dl).abs().max()):.2e}, max |coef err| {float((coef.cpu().double() - want_coef).abs().max()):.2e}")
    close(coef, want_coef, 1e-5, 1e-6, what="coef")
    assert bool((coef.cpu()[dead] == 0).all())
    close(loss[0], want_loss, 1e-6, 1e-5, what="loss")
    assert bool(torch.isfinite(dl).all()), "a coef == 0 row over NaN logits must be written as zeros"
    assert bool((dl.cpu()[dead] == 0).all())
    close(dl, want_dl, 1e-4, 1e-7, what="d_logits")
    # two runs bit-identical
    loss2, coef2, dl2 = _run(lg, sq, rw, N, T, V)
    torch.cuda.synchronize()
    assert torch.equal(loss, loss2) and torch.equal(coef, coef2) and torch.equal(dl, dl2)


def test_logprob_backward_with_a_row_stride_and_unaligned_rows():
    """Row stride above V (a column slice of a wider buffer) on the 16-byte path, and an odd base offset on the scalar one."""
    V, N, T = 200, 7, 4
    logits, seqs, reward = _case(V, seed=9, N=N, T=T)
    _, want_coef, want_dl, _ = _reference(logits, seqs, reward)
    for ld, shift in ((V + 8, 0), (V + 8, 1)):
        buf = torch.zeros(N * T * ld + 4, device="cuda")
        src = buf[shift:shift + N * T * ld].view(N * T, ld)
        src[:, :V] = logits.reshape(N * T, V).cuda()
        lse = torch.logsumexp(src[:, :V], -1).contiguous()
        out = torch.full((N * T * ld + 4,), 7.0, device="cuda")
        dst = out[shift:shift + N * T * ld].view(N * T, ld)
        _lib.call("acvae_logprob_bwd", src, ld, lse, seqs.cuda().reshape(-1), want_coef.float().cuda().reshape(-1), dst,
                  N * T, V, S())
        torch.cuda.synchronize()
        close(dst[:, :V].reshape(N, T, V), want_dl, 1e-4, 1e-7, what=f"d_logits ld={ld} shift={shift}")
        assert bool((dst[:, V:] == 7.0).all()), "columns beyond V must not be written"
        assert float(out[:shift].sum()) == 7.0 * shift and bool((out[shift + N * T * ld:] == 7.0).all())
