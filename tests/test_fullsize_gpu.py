"""GPU: BASELINE.json's full sizes.  Properties that need no oracle (batch-independence in eval mode, run-to-run bitwise
determinism of the training step, conservation properties of the attention weights and of the losses, the T=3000
long-audio configuration (C4), the N=5 z-samples-per-clip inference twin (C5)), and one oracle step per shape for the loss
triplet, the greedy tokens and the global gradient norm.  Every parameter gradient against the oracle at these shapes:
test_fullsize_grads_gpu.py."""
import random

import numpy as np
import pytest
import torch

from acvae_amd import _lib
from acvae_amd.decoder import VAERNNBahdanauAttnDecoder
from acvae_amd.encoder import Cnn10
from acvae_amd.trainer import TrainStep
from acvae_amd.vae_model import Hybrid_VAEModel

pytestmark = pytest.mark.gpu
V, E, L = 5000, 512, 22


def build(seed=1):
    torch.manual_seed(seed)
    dec = VAERNNBahdanauAttnDecoder(vocab_size=V, enc_mem_size=E, embed_size=E, hidden_size=E, attn_size=E)
    m = Hybrid_VAEModel(Cnn10(64, 512), dec, posterior_model="PosteriorRNN_hybrid", posterior_args={"hidden_size": E},
                        prior_model="PriorRNN", prior_args={"hidden_size": E})
    return m.cuda()


def batch(B, T, seed=3, ragged=False):
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(B, T, 64, generator=g)
    caps = torch.zeros(B, L)
    lens = np.full(B, L)
    if ragged:
        lens = np.sort(np.random.RandomState(seed).randint(8, L + 1, B))[::-1].copy(); lens[0] = L
    for b in range(B):
        n = int(lens[b])
        caps[b, 0] = 1; caps[b, 1:n - 1] = torch.randint(4, V, (n - 2,), generator=g).float(); caps[b, n - 1] = 2
    return feats, caps, np.full(B, T), lens


def test_eval_forward_is_batch_independent_config2():
    """BN in eval mode + no dropout: clip n's outputs must not depend on its batch mates (B=32 vs 2 x 16)."""
    model = build().eval()
    feats, caps, fl, cl = batch(32, 1000)
    eps_q = torch.randn(32, L - 1, E); eps_p = torch.randn(L - 1, 32, E)
    f = feats.cuda()

    def run(sl):
        model.noise = dict(eps_q=eps_q[sl], eps_p=eps_p[:, sl])
        random.seed(0)
        with torch.no_grad():
            return model(f[sl], fl[sl].copy(), caps[sl], cl[sl], ss_ratio=1.0, dis_ratio=0)
    full = run(slice(0, 32)); a = run(slice(0, 16)); b = run(slice(16, 32))
    for k in ("logits", "p_means", "q_means", "outputs", "p_means_utt", "attn_weights"):
        cat = torch.cat([a[k], b[k]], 0)
        assert torch.allclose(full[k], cat, rtol=1e-5, atol=1e-5), (k, float((full[k] - cat).abs().max()))
    assert torch.equal(full["seqs"], torch.cat([a["seqs"], b["seqs"]], 0))
    w = full["attn_weights"]                                  # [N,S,Tc]: softmax rows sum to 1, masked tail is 0
    assert torch.allclose(w.sum(1), torch.ones_like(w.sum(1)), atol=1e-5) and float(w.min()) >= 0.0


def test_train_step_is_bitwise_deterministic_config2():
    """Same seeds -> identical loss, gradient norm and updated weights (all reductions are fixed-order)."""
    feats, caps, fl, cl = batch(32, 1000, ragged=True)
    res = []
    for _ in range(2):
        model = build(7).train()
        model.encoder._seed_base = 1234                      # dropout Philox key
        ts = TrainStep(model, V)
        torch.manual_seed(11); random.seed(11)
        p = ts.step(feats.cuda(), fl.copy(), caps, cl, ss_ratio=1.0, dis_ratio=0, kl_weight=0.5)
        torch.cuda.synchronize()
        res.append((float(p["loss"]), float(p["grad_norm"]), ts.flat_p.clone()))
    assert res[0][0] == res[1][0] and res[0][1] == res[1][1]
    assert torch.equal(res[0][2], res[1][2])
    assert np.isfinite(res[0][0]) and 7.0 < res[0][0] < 40.0  # ~ln(5000) + KL/MSE terms at random init


def test_loss_decreases_over_steps_config1_shape():
    feats, caps, fl, cl = batch(8, 500)
    model = build(3).train()
    ts = TrainStep(model, V, lr=5e-4)
    losses = []
    for i in range(12):
        random.seed(i)
        losses.append(float(ts.step(feats.cuda(), fl.copy(), caps, cl, 1.0, 0, 0.5)["loss"]))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0] - 0.5, losses


def test_long_audio_config4_t3000():
    """C4: T=3000 frames, B=16 -> S=187 encoder frames; ragged feat_lens exercise the attention mask."""
    model = build().train()
    feats, caps, fl, cl = batch(16, 3000, ragged=True)
    fl = np.array([3000, 2900, 2500, 2000, 1600, 1500, 1000, 999, 640, 512, 400, 333, 160, 100, 48, 17])
    ts = TrainStep(model, V)
    random.seed(0)
    loss, parts, out = ts.forward_loss(feats.cuda(), fl.copy(), caps, cl, 1.0, 0, 0.5)
    assert out["attn_weights"].shape == (16, 187, L - 1) and out["logits"].shape == (16, L - 1, V)
    lens = torch.as_tensor(fl // 16)
    w = out["attn_weights"].detach().cpu()
    for n in range(16):
        ln = int(lens[n])
        if 0 < ln < 187:
            assert float(w[n, ln:].abs().max()) == 0.0        # nothing attends past the clip
        assert torch.allclose(w[n].sum(0), torch.ones(L - 1), atol=1e-5)
    loss.backward()
    g = model.encoder.conv_block1.conv1.weight.grad
    assert torch.isfinite(loss) and g is not None and bool(torch.isfinite(g).all())


def test_inference_n5_samples_config5():
    """C5: greedy decode with N=5 z-samples per clip: distinct captions for one clip, bit-identical replay."""
    model = build().eval()
    feats, _, fl, _ = batch(4, 1000)
    f5 = feats.repeat(5, 1, 1).cuda()                         # runner :102-104 replication
    l5 = [int(x) for x in fl for _ in range(5)]
    eps = torch.randn(20, 20, E)
    outs = []
    for _ in range(2):
        model.noise = dict(eps_p=eps)
        with torch.no_grad():
            outs.append(model(f5, list(l5), method="greedy", beam_size=5)["seqs"].cpu())
    assert torch.equal(outs[0], outs[1]) and outs[0].shape == (20, 20) and outs[0].dtype == torch.long
    rows = outs[0][0::4]                                       # the 5 replicas of clip 0 (batch tiling order)
    assert len({tuple(r.tolist()) for r in rows}) > 1          # different z -> different captions
    for r in outs[0]:                                          # once <end> (2) is emitted the row stays <end>
        idx = (r == 2).nonzero()
        if len(idx):
            assert bool((r[int(idx[0]):] == 2).all())


C4_FEAT_LENS = np.array([3000, 2900, 2500, 2000, 1600, 1500, 1000, 999, 640, 512, 400, 333, 160, 100, 48, 17])


@pytest.mark.parametrize("B,T", [(32, 1000), (16, 3000), (5, 999), (9, 517), (3, 1601)])
def test_loss_vs_oracle_at_config2_full_size(B, T):
    """BASELINE configs[1] itself (B=32, T=1000, V=5000, E=512, 22-token captions), configs[3] itself (B=16, T=3000 ->
    S=187, the ragged feature lengths of test_long_audio_config4_t3000: Winograd row blocks at H=3000/1500/750/375), and
    the same model on batch sizes / frame counts that are no multiple of any tile (ragged caption and feature lengths):
    one forward + loss on the HIP path against the oracle on the same weights, batch, dropout masks and noise —
    north_star's bar, |loss diff| <= 1e-4, plus token ids exact; the gradient norm (through the whole backward) within
    2e-4 (5e-4 for the small odd batches, where one ReLU-boundary flip weighs more)."""
    import os, sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import acvae_oracle as O
    from acvae_amd.train_util import LabelSmoothingLoss, MSELoss, Normal_kl_loss
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    model = build(5).train()
    state = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    feats, caps, fl, cl = O.synthetic_batch(B, T, V, L, seed=4, ragged=True)
    if (B, T) == (16, 3000):
        fl = C4_FEAT_LENS.copy()
        for b in range(B):
            feats[b, int(fl[b]):] = 0.0
    rec = {}
    torch.manual_seed(9); random.seed(9)
    ores = O.OracleTrainer(state, V).step(feats, fl.copy(), caps, cl, 1.0, 0, record=rec, apply_update=False)
    model.encoder.dropout_masks = rec["dropout"]
    model.noise = dict(eps_q=rec["eps_q"], eps_p=rec["eps_p"])
    random.seed(9)
    out = model(feats.cuda(), fl.copy(), caps, cl, ss_ratio=1.0, dis_ratio=0)
    if (B, T) == (16, 3000):
        assert out["attn_weights"].shape == (16, 187, L - 1)
        w_got, w_want = out["attn_weights"].detach().cpu(), ores["out"]["attn_weights"].detach()
        # rtol 1e-4 / atol 1e-5 where the summation order changes
        viol = (w_got - w_want).abs() - (1e-5 + 1e-4 * w_want.abs())
        i = int(viol.argmax())
        assert float(viol.max()) <= 0, ("attn_weights", float(w_got.reshape(-1)[i]), float(w_want.reshape(-1)[i]),
                                        float((w_got - w_want).abs().max()), int((viol > 0).sum()))
    lens1 = np.asarray(cl) - 1
    ce = LabelSmoothingLoss(V, 0.1).masked(out["logits"], caps[:, 1:].to(torch.long), lens1)
    kl = Normal_kl_loss()(out["q_means"], out["q_logs"], out["p_means"], out["p_logs"])
    mse = MSELoss()(out["q_means_utt"], out["p_means_utt"])
    loss = ce + 0.5 * kl + 1.0 * mse
    for name, got, want in (("loss", loss, ores["loss"]), ("ce", ce, ores["ce"]), ("kl", kl, ores["kl"]), ("mse", mse, ores["mse"])):
        got, want = float(got.detach()), float(want.detach())
        assert abs(got - want) <= 1e-4 * max(1.0, abs(want)), (name, got, want)
    assert torch.equal(out["seqs"].cpu(), ores["out"]["seqs"])
    loss.backward()
    gn = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in model.parameters() if p.grad is not None))
    tol = 2e-4 if B >= 32 else 5e-4
    print(f"B={B} T={T}: grad-norm rel diff {abs(float(gn) - float(ores['grad_norm'])) / float(ores['grad_norm']):.2e} (bound {tol:.0e})")
    assert abs(float(gn) - float(ores["grad_norm"])) <= tol * float(ores["grad_norm"]), (float(gn), float(ores["grad_norm"]))


@pytest.mark.parametrize("B,T", [(5, 999), (32, 1000)])
def test_backward_is_bit_reproducible_from_the_first_run(B, T):
    """Forward + loss + backward of one batch, four times on fresh gradients (no dropout): every parameter gradient of every run
    equals the FIRST run's bit for bit.  The first run works on freshly allocated buffers, later ones on recycled memory that
    still holds the previous (identical) values - a kernel on the second stream that outlives its operands, or reads what it has
    not been handed yet, shows up exactly there (round 4: the trailing parameter-gradient products read the encoder memory in
    place after autograd had released it; only this comparison caught it)."""
    _assert_four_runs_bit_identical(B, T, dis_ratio=0)


@pytest.mark.parametrize("path", ["prior_feeds_decoder", "per_step_chains"])
def test_backward_is_bit_reproducible_on_the_two_chain_paths(path):
    """As above, on the forward paths whose two chains run on two streams step by step: dis_ratio > 0 (the prior's z feeds the
    decoder: the prior chain, then the decoder chain) and the per-step launches instead of the persistent one (both chains side
    by side).  Both read the zero h_{-1} on the prior chain's stream at step 0; it is zeroed in front of the fork (it used to be
    zeroed on the first stream behind the fork, with no edge to the reader).  The side stream stays on in both."""
    if path == "prior_feeds_decoder":
        _assert_four_runs_bit_identical(5, 999, dis_ratio=0.5)
    else:
        with _lib.override(persist=False):
            _assert_four_runs_bit_identical(5, 999, dis_ratio=0)


def _assert_four_runs_bit_identical(B, T, dis_ratio):
    import os, sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import acvae_oracle as O
    from acvae_amd.train_util import LabelSmoothingLoss, MSELoss, Normal_kl_loss
    model = build(5).train()
    assert model.use_side_stream
    model.encoder.p_block = model.encoder.p_fc = 0.0
    feats, caps, fl, cl = O.synthetic_batch(B, T, V, L, seed=4, ragged=True)
    g = torch.Generator().manual_seed(3)
    noise = dict(eps_q=torch.randn(B, L - 1, E, generator=g), eps_p=torch.randn(L - 1, B, E, generator=g))
    ref = None
    for run in range(4):
        for p in model.parameters():
            p.grad = None
        model.noise = noise
        random.seed(9)
        torch.manual_seed(9)             # the dis_ratio coins (and any dropout) are drawn on the CPU generator
        out = model(feats.cuda(), fl.copy(), caps, cl, ss_ratio=1.0, dis_ratio=dis_ratio)
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
            assert all(bool(torch.isfinite(v).all()) for v in cur.values())
            continue
        bad = [n for n in ref if not torch.equal(cur[n], ref[n])]
        assert not bad, (run, bad[:8])


def test_inference_n5_vs_oracle_config5_full_size():
    """configs[4] at full size against the oracle (not only properties): 4 clips x 5 z-samples, T=1000, V=5000, E=512,
    greedy decode with the prior's z every step (models/vae_model.py:880-894, runner :101-104 replication) on the same
    eps -> token ids bit-exact, first-step logits within fp32 rounding."""
    import os, sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import acvae_oracle as O
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    model = build(5).eval()
    state = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    feats, _, fl, _ = O.synthetic_batch(4, 1000, V, L, seed=6, ragged=True)
    f5 = feats.repeat(5, 1, 1)
    l5 = [int(x) for _ in range(5) for x in fl]                # feats.repeat tiles the batch: clip = row % 4
    eps = torch.randn(20, 20, E, generator=torch.Generator().manual_seed(12))
    with torch.no_grad():
        want = O.hybrid_forward(state, f5, np.asarray(l5), training=False, method="greedy", noise=dict(eps_p=eps))
        model.noise = dict(eps_p=eps)
        got = model(f5.cuda(), list(l5), method="greedy", beam_size=5)
    assert torch.equal(got["seqs"].cpu(), want["seqs"])
    d0 = (got["logits"][:, 0].cpu() - want["logits"][:, 0]).abs().max()
    assert float(d0) <= 2e-5 + 1e-4 * float(want["logits"][:, 0].abs().max()), float(d0)
    rows = got["seqs"].cpu()[0::4]
    assert len({tuple(r.tolist()) for r in rows}) > 1          # different z -> different captions of clip 0


def test_training_steps_do_not_leak_device_memory():
    """A tensor that an autograd Function both returns and keeps as a plain ctx attribute is never collected (tensor ->
    grad_fn -> ctx -> tensor); the Functions keep such tensors through save_for_backward.  Guard: the allocated bytes
    after step 4 and after step 14 are the same."""
    import gc
    model = build(2).train()
    ts = TrainStep(model, V)
    feats, caps, fl, cl = batch(4, 160, ragged=True)
    f = feats.cuda()
    marks = []
    for i in range(14):
        random.seed(i)
        ts.step(f, fl.copy(), caps, cl, 1.0, 0, 0.5)
        if i in (3, 13):
            torch.cuda.synchronize(); gc.collect()
            marks.append(torch.cuda.memory_allocated())
    assert marks[1] <= marks[0] + (1 << 20), marks
