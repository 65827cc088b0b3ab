"""GPU: the stacked posterior (PosteriorRNN_hybrid with num_layers > 1, acvae_posterior_stack_fwd / _bwd) against torch's
nn.GRU(num_layers, bidirectional, dropout) on the CPU in fp64 - the reference's own module, as
tests/test_kernels_gpu.py::test_bigru_seq_and_posterior_golden_g5 - forward and backward, in eval mode and with the
inter-layer dropout of training mode; the persistent against the per-step recurrence; the one-layer case of the new entry
points against acvae_posterior_fwd / _bwd; and a stacked model trained end to end through TrainStep.

The widths are parameters: the posterior called on its own takes any GRU width Hq beside the embed width E
(widths_util.POSTERIOR_SETS: Hq below, above and no multiple of E, and one that is no multiple of 32 and so runs per step).
The direct acvae_posterior_* calls get their buffers 4 KiB longer than declared, with a sentinel in the tail that must be
untouched afterwards."""
import copy
import io
import random

import numpy as np
import pytest
import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

from acvae_amd import _lib
from acvae_amd import text_encoder as TE
from acvae_amd.encoder import ptr_table
from widths_util import POSTERIOR_SETS

pytestmark = pytest.mark.gpu
E, HQ, VQ = 64, 64, 30


def _caption_batch(N, seed):
    """caps [N, Tc+1] and cap_lens (descending, as pack_padded_sequence wants them) with length-1 rows (cap_lens 2)."""
    g = np.random.default_rng(seed)
    lens1 = np.sort(g.integers(1, 10, size=N))[::-1].copy()
    lens1[0], lens1[-1] = 9, 1
    if N > 2:
        lens1[-2] = 1
    cap_lens = lens1 + 1
    caps = torch.from_numpy(g.integers(1, VQ, size=(N, int(cap_lens.max())))).float()
    return caps, cap_lens


def _posterior(L, p, E=E, HQ=HQ):
    torch.manual_seed(11)
    q = TE.PosteriorRNN_hybrid(E, E, VQ, hidden_size=HQ, num_layers=L, dropout=p)
    with torch.no_grad():
        for prm in q.parameters():            # magnitudes that keep every gate away from saturation
            prm.uniform_(-0.3, 0.3)
    return q


def _torch_posterior(q, caps, cap_lens, eps, train, seed, E=E):
    """PosteriorRNN_hybrid.forward (models/text_encoder.py:182-216) in fp64 on the CPU with torch's nn.GRU; the dropout
    masks come from the CPU generator under `seed`, inside self.network(...), as in the reference."""
    ref = copy.deepcopy(q).cpu().double()
    ref.train(train)
    lens1 = torch.as_tensor(cap_lens - 1)
    Tc = int(lens1.max())
    x = ref.word_embedding(caps[:, :Tc].long())
    torch.manual_seed(seed)
    out = ref.network(pack_padded_sequence(x, lens1, batch_first=True))[0]
    h = pad_packed_sequence(out, batch_first=True)[0]
    ml = ref.token_mean_log(h)
    mean, log = ml[..., :E], ml[..., E:]
    z = eps.double() * torch.exp(0.5 * log) + mean
    mask = (torch.arange(Tc)[None, :] < lens1[:, None])[..., None]
    utt = (h * mask).sum(1) / lens1[:, None].double() + h.masked_fill(~mask, float("-inf")).max(1)[0]
    return ref, (mean, log, z, utt)


WORST = {}                 # worst error / tolerance per tensor group ("outputs", "gradients"), printed when the module is through


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for k in sorted(WORST):
        print(f"\nPOSTERIOR worst error / tolerance, {k}: {WORST[k]:.3f}", end="")


def _close(a, b, rtol, atol, what):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = (a - b).abs()
    group = "gradients" if what.startswith("d ") else "outputs"
    WORST[group] = max(WORST.get(group, 0.0), float((err / (atol + rtol * b.abs())).max()))
    ok = err <= atol + rtol * b.abs()
    assert bool(ok.all()), f"{what}: max abs err {float(err.max()):.3e} (ref max {float(b.abs().max()):.3e})"


def _run(q, caps, cap_lens, eps, seed, ups):
    """forward under `seed` (the masks are drawn inside it) and backward with the upstream gradients `ups`"""
    for prm in q.parameters():
        prm.grad = None
    torch.manual_seed(seed)
    out = q(caps.cuda(), cap_lens, eps=eps)
    outs = [out[k] for k in ("q_means", "q_logs", "q_z", "q_means_utt")]
    torch.autograd.backward(outs, [u.cuda() for u in ups])
    torch.cuda.synchronize()
    return [o.detach().clone() for o in outs], {n: prm.grad.detach().clone() for n, prm in q.named_parameters()}


def _upstream(N, Tc, seed, E=E, HQ=HQ):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(N, Tc, E, generator=g) for _ in range(3)] + [torch.randn(N, 2 * HQ, generator=g)]


@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("N", [5, 32, 33])
@pytest.mark.parametrize("L", [2, 3])
def test_stacked_posterior_matches_torch_gru(L, N, mode):
    """q_means, q_logs, q_z, q_means_utt and the gradient of every posterior parameter (embedding, each layer's eight
    tensors, token_mean_log) against torch autograd in fp64, for random upstream gradients of all four outputs.  N = 33 runs
    the per-step recurrence, N <= 32 the persistent one; train mode applies nn.GRU's dropout (p = 0.3) between layers."""
    train = mode == "train"
    q = _posterior(L, 0.3).cuda().train(train)
    caps, cap_lens = _caption_batch(N, seed=N + L)
    Tc = int(cap_lens.max()) - 1
    eps = torch.randn(N, Tc, E, generator=torch.Generator().manual_seed(5))
    ups = _upstream(N, Tc, 6)
    outs, grads = _run(q, caps, cap_lens, eps, 21, ups)
    ref, routs = _torch_posterior(q, caps, cap_lens, eps, train, 21)
    for got, want, key in zip(outs, routs, ("q_means", "q_logs", "q_z", "q_means_utt")):
        _close(got, want, 1e-4, 1e-5, f"{key} L={L} N={N} {mode}")
    torch.autograd.backward(list(routs), [u.double() for u in ups])
    names = [n for n, _ in ref.named_parameters()]
    assert len(names) == 3 + 8 * L and any(n.endswith(f"_l{L - 1}_reverse") for n in names)
    for n, prm in ref.named_parameters():
        want = prm.grad
        assert float(want.abs().max()) > 0, n
        _close(grads[n], want, 1e-4, 2e-5 * float(want.abs().max()), f"d {n} L={L} N={N} {mode}")


def test_persistent_and_per_step_recurrences_agree_bit_for_bit():
    """L = 2, N = 32, training mode: the persistent launches and the per-step loop give the same outputs and gradients."""
    q = _posterior(2, 0.3).cuda().train()
    caps, cap_lens = _caption_batch(32, seed=3)
    Tc = int(cap_lens.max()) - 1
    eps = torch.randn(32, Tc, E, generator=torch.Generator().manual_seed(5))
    ups = _upstream(32, Tc, 7)
    o1, g1 = _run(q, caps, cap_lens, eps, 4, ups)
    with _lib.override(persist=False):
        o2, g2 = _run(q, caps, cap_lens, eps, 4, ups)
    for a, b in zip(o1, o2):
        assert torch.equal(a, b)
    bad = [n for n in g1 if not torch.equal(g1[n], g2[n])]
    assert not bad, bad


TAIL = 4096


def _with_tail(nbytes, fill):
    """A buffer of `nbytes` declared bytes with TAIL more behind them that hold a sentinel: (declared view, whole buffer)."""
    whole = torch.full((nbytes + TAIL,), fill, dtype=torch.uint8, device="cuda")
    whole[nbytes:] = 0xA5
    return whole[:nbytes], whole


def _tail_untouched(whole, what):
    tail = whole[-TAIL:]
    assert bool((tail == 0xA5).all()), f"{what}: {int((tail != 0xA5).sum())} bytes behind the declared size were written"


def _one_layer_entries(N, E=E, HQ=HQ):
    q = _posterior(1, 0.0, E, HQ).cuda()
    caps, cap_lens = _caption_batch(N, seed=9)
    lens1 = torch.as_tensor(cap_lens - 1).cuda()
    Tc = int(cap_lens.max()) - 1
    caps_d = caps.long().cuda().contiguous()
    eps = torch.randn(N, Tc, E, generator=torch.Generator().manual_seed(5)).cuda()
    ups = [u.cuda() for u in _upstream(N, Tc, 8, E, HQ)]
    params = q._text_table()
    dims = (N, Tc, E, HQ, VQ)
    s = _lib.current_stream()
    results = []
    for stacked in (False, True):
        sb = _lib.call("acvae_posterior_saved_bytes", *dims)
        cb = _lib.call("acvae_posterior_scratch_bytes", *dims)
        assert sb > 0 and cb > 0
        assert sb == _lib.call("acvae_posterior_stack_saved_bytes", *dims, 1)
        assert cb == _lib.call("acvae_posterior_stack_scratch_bytes", *dims, 1)
        saved, saved_whole = _with_tail(sb, 0x00)
        scratch, scratch_whole = _with_tail(cb, 0x7F)
        qm, ql, qz = (torch.empty(N, Tc, E, device="cuda") for _ in range(3))
        utt = torch.empty(N, 2 * HQ, device="cuda")
        grads = [torch.empty_like(p) if p is not None and 10 <= i <= 20 else None for i, p in enumerate(params)]
        _lib.persist_status(torch.device("cuda"))
        if stacked:
            _lib.call("acvae_posterior_stack_fwd", ptr_table(params), None, 1, None, 0.0, caps_d, caps_d.stride(0), lens1,
                      eps, qm, ql, qz, utt, saved, sb, scratch, cb, *dims, s, _lib.call_flags())
            _lib.call("acvae_posterior_stack_bwd", ptr_table(params), ptr_table(grads), None, None, 1, None, 0.0, lens1, eps,
                      ql, *ups, saved, sb, scratch, cb, *dims, s, _lib.call_flags())
        else:
            _lib.call("acvae_posterior_fwd", ptr_table(params), caps_d, caps_d.stride(0), lens1, eps, qm, ql, qz, utt, saved,
                      sb, scratch, cb, *dims, s, _lib.call_flags())
            _lib.call("acvae_posterior_bwd", ptr_table(params), ptr_table(grads), lens1, eps, ql, *ups, saved, sb, scratch,
                      cb, *dims, s, _lib.call_flags())
        torch.cuda.synchronize()
        _lib.check_persist_status(torch.device("cuda"))
        _tail_untouched(saved_whole, f"saved (stacked={stacked}, E={E}, Hq={HQ}, N={N})")
        _tail_untouched(scratch_whole, f"scratch (stacked={stacked}, E={E}, Hq={HQ}, N={N})")
        results.append([qm, ql, qz, utt] + [g for g in grads if g is not None])
    assert len(results[0]) == 4 + 11
    assert all(bool(torch.isfinite(t).all()) for t in results[0])
    for k, (a, b) in enumerate(zip(*results)):
        assert torch.equal(a, b), k


@pytest.mark.parametrize("N", [5, 33])
def test_one_layer_stack_entry_is_the_one_layer_call(N):
    """acvae_posterior_stack_fwd / _bwd with num_layers = 1 (no upper table, no mask) reproduce acvae_posterior_fwd / _bwd
    bit for bit, outputs and every gradient; neither writes behind the sizes it declares."""
    _one_layer_entries(N)


# ------------------------------------------------------------------------------------------------- unequal widths
def _matches_torch_gru(Ew, Hw, L, N, mode):
    train = mode == "train"
    q = _posterior(L, 0.3 if L > 1 else 0.0, Ew, Hw).cuda().train(train)
    assert q.network.weight_ih_l0.shape == (3 * Hw, Ew) and q.token_mean_log.weight.shape == (2 * Ew, 2 * Hw)
    caps, cap_lens = _caption_batch(N, seed=N + L)
    Tc = int(cap_lens.max()) - 1
    eps = torch.randn(N, Tc, Ew, generator=torch.Generator().manual_seed(5))
    ups = _upstream(N, Tc, 6, Ew, Hw)
    outs, grads = _run(q, caps, cap_lens, eps, 21, ups)
    _lib.check_persist_status(torch.device("cuda"))
    ref, routs = _torch_posterior(q, caps, cap_lens, eps, train, 21, Ew)
    tag = f"E={Ew} Hq={Hw} L={L} N={N} {mode}"
    for got, want, key in zip(outs, routs, ("q_means", "q_logs", "q_z", "q_means_utt")):
        _close(got, want, 1e-4, 1e-5, f"{key} {tag}")
    torch.autograd.backward(list(routs), [u.double() for u in ups])
    assert len(list(ref.named_parameters())) == 3 + 8 * L
    for n, prm in ref.named_parameters():
        want = prm.grad
        assert float(want.abs().max()) > 0, n
        _close(grads[n], want, 1e-4, 2e-5 * float(want.abs().max()), f"d {n} {tag}")


@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("N", [5, 32, 33])
@pytest.mark.parametrize("L", [1, 2, 3])
@pytest.mark.parametrize("Ew,Hw", POSTERIOR_SETS, ids=[f"E{e}_Hq{h}" for e, h in POSTERIOR_SETS])
def test_posterior_widths_match_torch_gru(Ew, Hw, L, N, mode):
    """test_stacked_posterior_matches_torch_gru, same bounds, with the embed width E and the GRU width Hq apart, and with one
    layer as well: the input projection is [3 Hq, E], the upper layers' [3 Hq, 2 Hq], token_mean_log [2 E, 2 Hq].  N <= 32 and
    Hq % 32 == 0 run the persistent recurrence (grid 2 Hq / 32), everything else goes per step."""
    _matches_torch_gru(Ew, Hw, L, N, mode)


@pytest.mark.parametrize("L", [1, 2])
@pytest.mark.parametrize("Ew,Hw", POSTERIOR_SETS, ids=[f"E{e}_Hq{h}" for e, h in POSTERIOR_SETS])
def test_posterior_widths_persistent_and_per_step_agree_bit_for_bit(Ew, Hw, L):
    """N = 32, training mode: the persistent launches and the per-step loop give the same outputs and gradients at every
    width (at Hq % 32 != 0 both runs go per step: the plan refuses the width)."""
    q = _posterior(L, 0.3 if L > 1 else 0.0, Ew, Hw).cuda().train()
    caps, cap_lens = _caption_batch(32, seed=3)
    Tc = int(cap_lens.max()) - 1
    eps = torch.randn(32, Tc, Ew, generator=torch.Generator().manual_seed(5))
    ups = _upstream(32, Tc, 7, Ew, Hw)
    o1, g1 = _run(q, caps, cap_lens, eps, 4, ups)
    _lib.check_persist_status(torch.device("cuda"))
    with _lib.override(persist=False):
        o2, g2 = _run(q, caps, cap_lens, eps, 4, ups)
    for a, b in zip(o1, o2):
        assert torch.equal(a, b)
    bad = [n for n in g1 if not torch.equal(g1[n], g2[n])]
    assert not bad, bad


@pytest.mark.parametrize("N", [5, 32, 33])
@pytest.mark.parametrize("Ew,Hw", POSTERIOR_SETS[1:], ids=[f"E{e}_Hq{h}" for e, h in POSTERIOR_SETS[1:]])
def test_posterior_widths_one_layer_stack_entry_is_the_one_layer_call(Ew, Hw, N):
    _one_layer_entries(N, Ew, Hw)


# ------------------------------------------------------------------------------------------------- end to end
def _model(seed=0):
    """Hybrid_VAEModel with posterior_args={"num_layers": 2, "dropout": 0.3}; every tensor but the upper layer's from the
    closed-form state of tests/test_optim_gpu.py, the upper layer from torch's init under `seed`."""
    from acvae_amd.decoder import VAERNNBahdanauAttnDecoder
    from acvae_amd.encoder import Cnn10
    from acvae_amd.vae_model import Hybrid_VAEModel
    from test_optim_gpu import E as EM, V as VM, _state
    torch.manual_seed(seed)
    dec = VAERNNBahdanauAttnDecoder(vocab_size=VM, enc_mem_size=EM, embed_size=EM, hidden_size=EM, dropout=0.0,
                                    num_layers=1, rnn_type="GRU", attn_size=EM)
    m = Hybrid_VAEModel(Cnn10(64, 512), dec, posterior_model="PosteriorRNN_hybrid",
                        posterior_args={"hidden_size": EM, "num_layers": 2, "dropout": 0.3},
                        prior_model="PriorRNN", prior_args={"hidden_size": EM, "dropout": 0.0})
    missing, unexpected = m.load_state_dict({k: v.clone() for k, v in _state().items()}, strict=False)
    assert not unexpected and missing and all(k.startswith("qnet.network.") and "_l1" in k for k in missing)
    m = m.cuda().train()
    m.encoder.p_block = m.encoder.p_fc = 0.0
    return m


def test_train_step_matches_autograd_adam_twin():
    """Three TrainStep steps of the stacked model against the same model driven by autograd, clip_grad_norm_ and
    torch.optim.Adam (the twin of tests/test_optim_gpu.py, same bounds); the upper layers are in the posterior's gradient
    bucket and are updated."""
    from acvae_amd.trainer import TrainStep
    from test_optim_gpu import compare_params, one, sync_params, twin_step
    m1, m3 = _model(), _model()
    t1, t3 = TrainStep(m1, 40), TrainStep(m3, 40)
    up = m1.qnet.network.weight_ih_l1
    off, q_start = t1._offsets()[up], t1.n_text_dec
    assert q_start <= off < t1.n_text, "the upper layer is outside the posterior bucket"
    opt = torch.optim.Adam([p for p in m3.parameters() if p.requires_grad], lr=5e-4)
    before = up.detach().clone()
    for k in range(3):
        if k:
            sync_params(m1, m3)
        one(t1, seed=3 + k)
        twin_step(t3, m3, opt, seed=3 + k)
        compare_params(m1, m3, f"stacked posterior step {k + 1}")
        assert m3.qnet.network.weight_ih_l1_reverse.grad is not None
        assert float(m3.qnet.network.weight_ih_l1_reverse.grad.abs().max()) > 0
    torch.cuda.synchronize()
    assert not torch.equal(before, up.detach())


def test_checkpoint_round_trip():
    from acvae_amd.trainer import TrainStep
    from test_optim_gpu import one
    m1 = _model()
    t1 = TrainStep(m1, 40)
    one(t1)
    buf = io.BytesIO()
    torch.save({"model": m1.state_dict(), "optimizer": t1.optimizer.state_dict()}, buf)
    one(t1, seed=4)
    ck = torch.load(io.BytesIO(buf.getvalue()), weights_only=False)
    assert "qnet.network.weight_hh_l1_reverse" in ck["model"]
    assert len(ck["optimizer"]["state"]) == sum(1 for p in m1.parameters() if p.grad is not None)
    m2 = _model(seed=1)
    t2 = TrainStep(m2, 40)
    m2.load_state_dict(ck["model"])
    t2.optimizer.load_state_dict(ck["optimizer"])
    one(t2, seed=4)
    torch.cuda.synchronize()
    for (k, a), (_, b) in zip(m1.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k


def test_backward_is_bit_reproducible_from_the_first_run():
    """As tests/test_fullsize_gpu.py: forward + loss + backward four times on fresh gradients with the side streams on, the
    posterior's dropout masks replayed through model.noise["q_keep"]: every gradient equals the first run's bit for bit."""
    import acvae_oracle as O
    from acvae_amd.train_util import LabelSmoothingLoss, MSELoss, Normal_kl_loss
    model = _model()
    model.use_side_stream = True
    B, V, EM = 3, 40, 64
    feats, caps, fl, cl = O.synthetic_batch(B, 64, V, 7, seed=4, ragged=True)
    Tc = int(max(cl)) - 1
    g = torch.Generator().manual_seed(3)
    torch.manual_seed(8)
    keep = TE.posterior_keep_masks(np.asarray(cl) - 1, Tc, EM, 2, 0.3)
    noise = dict(eps_q=torch.randn(B, Tc, EM, generator=g), eps_p=torch.randn(Tc, B, EM, generator=g), q_keep=keep)
    ref = None
    for run in range(4):
        for p in model.parameters():
            p.grad = None
        model.noise = dict(noise)
        random.seed(9)
        out = model(feats.cuda(), fl.copy(), caps, cl, ss_ratio=1.0, dis_ratio=0)
        lens1 = np.asarray(cl) - 1
        loss = (LabelSmoothingLoss(V, 0.1).masked(out["logits"], caps[:, 1:].to(torch.long), lens1)
                + 0.5 * Normal_kl_loss()(out["q_means"], out["q_logs"], out["p_means"], out["p_logs"])
                + MSELoss()(out["q_means_utt"], out["p_means_utt"]))
        loss.backward()
        torch.cuda.synchronize()
        cur = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
        cur["loss"] = loss.detach().clone()
        if ref is None:
            ref = cur
            assert "qnet.network.weight_ih_l1" in cur
            assert all(bool(torch.isfinite(v).all()) for v in cur.values())
            continue
        bad = [n for n in ref if not torch.equal(cur[n], ref[n])]
        assert not bad, (run, bad[:8])
