"""GPU: one encoder pass shared by a clip's captions in the training step (``Hybrid_VAEModel.forward(..., clip_index=)``,
``TrainStep.step(..., clip_index=)``).

The kernels alone: acvae_rows_gather bit-equal to ``src[index]``, acvae_rows_fold bit-equal to a CPU fp32 loop that adds a
clip's rows in ascending order, twice the same bits, no scratch memory.

The model: B clips and N = B * k caption rows against the oracle's step on the batch in which every clip is repeated k times
(``feats[clip_index]``), which the shared pass equals exactly in real arithmetic: BatchNorm's batch mean and biased variance
over the clips are those over the repeated batch, the ReLU decisions are the same, every layer is linear in the upstream
gradient and the BatchNorm-backward means scale by exactly k.  The dropout masks are drawn per clip (the HIP encoder gets
them as they are, the oracle indexed by ``clip_index``), eps_q / eps_p are replayed on both sides.  Bounds are the project's
own for these shapes (tests/test_model_gpu.py): loss terms 1e-4 * max(1, |value|), words exact, tensors 1e-4 / 2e-5, every
parameter gradient through parity_util.grads_match_oracle under the HIP path's own ReLU decisions (indexed by
``clip_index`` for the oracle's repeated batch).  The encoder's outputs in front of the gather and every BatchNorm running
statistic are compared against the oracle's encoder on the B distinct clips alone (tolerances of tests/test_encoder_gpu.py):
``running_var`` carries the Bessel factor M / (M - 1) of the B clips, not kM / (kM - 1) of the repeated batch.

Seed of the Cnn14_16k case, chosen with the oracle alone on the CPU: at B = 2, T = 64 its last blocks normalise over 8 values
per channel, and for some batches the yardstick cannot resolve the 5e-4 gradient bound itself - the fp32 oracle's encoder
gradients on the repeated batch then lie further than that from the float64 oracle's under the same ReLU decisions (worst
tensor, seeds 9-16: 2.3e-3, 1.3e-4, 9.0e-5, 8.2e-5, 7.3e-5, 7.0e-4, 7.8e-5, 2.4e-5).  Criterion: the first seed at which the
fp32 oracle's own error is under a tenth of the bound (5e-5): seed 16.  The Cnn10 cases sit at 3e-6.
"""
import random
import types

import numpy as np
import pytest
import torch

import acvae_oracle as O
from acvae_amd import _lib
from parity_util import close, grads_match_oracle
from test_model_gpu import build_model, hip_loss
from test_sched_sampling_gpu import _caps, _patched

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ the kernels alone
def _csr(index, B):
    counts = np.bincount(index, minlength=B)
    offsets = np.zeros(B + 1, dtype=np.int32)
    np.cumsum(counts, out=offsets[1:])
    return offsets, np.argsort(index, kind="stable").astype(np.int32)


KERNEL_SHAPES = {                       # (B, N, R, index)
    "one_row": (1, 1, 64, [0]),
    "b3_k2_permuted": (3, 6, 4 * 64, [2, 0, 1, 1, 0, 2]),
    "b2_k5_config1_rows": (2, 10, 62 * 512, [1, 0, 0, 1, 1, 0, 1, 0, 0, 1]),
    "unequal_with_an_empty_clip": (5, 7, 1028, [4, 0, 2, 0, 3, 2, 0]),      # clip 1 has no rows; R is no multiple of the block
}


@pytest.mark.parametrize("shape", list(KERNEL_SHAPES))
def test_rows_gather_and_fold_are_exact(shape):
    B, N, R, index = KERNEL_SHAPES[shape]
    index = np.array(index, dtype=np.int64)
    assert len(index) == N and index.max() < B
    offsets, rows = _csr(index, B)
    g = torch.Generator().manual_seed(N * 1000 + B)
    src = torch.randn(B, R, generator=g)
    up = torch.randn(N, R, generator=g) * torch.logspace(-3, 3, N).unsqueeze(1)      # sums whose order shows in the last bit
    st = _lib.current_stream()
    dst = torch.full((N, R), float("nan"), device="cuda")
    _lib.call("acvae_rows_gather", src.cuda(), torch.from_numpy(index).cuda(), dst, B, N, R, st)
    assert torch.equal(dst.cpu(), src[torch.from_numpy(index)])
    want = torch.zeros(B, R)
    for c in range(B):
        for r in rows[offsets[c]:offsets[c + 1]]:            # ascending within the clip
            want[c] = want[c] + up[int(r)]
    assert list(rows[offsets[0]:offsets[1]]) == sorted(rows[offsets[0]:offsets[1]])
    up_d, off_d, rows_d = up.cuda(), torch.from_numpy(offsets).cuda(), torch.from_numpy(rows).cuda()
    folds = []
    for _ in range(2):
        out = torch.full((B, R), float("nan"), device="cuda")
        _lib.call("acvae_rows_fold", up_d, off_d, rows_d, out, B, N, R, st)
        folds.append(out.cpu())
    assert torch.equal(folds[0].view(torch.int32), want.view(torch.int32)), float((folds[0] - want).abs().max())
    assert torch.equal(folds[0].view(torch.int32), folds[1].view(torch.int32))
    if shape == "unequal_with_an_empty_clip":
        assert offsets[1] == offsets[2] and not folds[0][1].any()


def test_new_kernels_use_no_scratch():
    from acvae_amd.build import resource_usage
    u = resource_usage()
    mine = {k: v for k, v in u.items() if "rows_gather_kernel" in k or "rows_fold_kernel" in k}
    assert len(mine) == 2, sorted(mine)
    assert all(v.get("scratch", -1) == 0 for v in mine.values()), {k: v.get("scratch") for k, v in mine.items()}


# ------------------------------------------------------------------------------------------------ the model
V, E, TT, L = 44, 64, 64, 7


def make_case(B, k, seed, encoder="Cnn10", permute=True, dis=0):
    """B clips with ragged lengths, N = B * k ragged captions sorted by length, the rows' clips permuted; the oracle's
    encoder on the B clips alone (it draws the per-clip dropout masks); eps_q / eps_p."""
    g = torch.Generator().manual_seed(seed)
    div = 16 if encoder == "Cnn10" else 32
    state = O.closed_form_state(O.state_shapes(V, E, E, None, E, 512 if encoder == "Cnn10" else 2048, encoder=encoder))
    feats = torch.randn(B, TT, 64, generator=g)
    fl = np.array([TT] + [int(x) for x in torch.randint(div + 1, TT, (B - 1,), generator=g)])
    N = B * k
    cl = np.array(sorted([L] + [int(x) for x in torch.randint(2, L + 1, (N - 1,), generator=g)], reverse=True))
    caps = _caps(V, list(cl), L, g)
    ci = np.repeat(np.arange(B), k)
    if permute:
        ci = ci[torch.randperm(N, generator=g).numpy()]
    Tc = int(cl.max()) - 1
    st_b = {n: v.clone() for n, v in state.items()}
    masks = []
    torch.manual_seed(seed)
    with torch.no_grad():
        enc_b = O.cnn10_forward(st_b, feats, fl.copy(), True, None, masks)
    eps_q = torch.randn(N, Tc, E, generator=g)
    eps_p = torch.randn(Tc, N, E, generator=g)
    flags = [t % 2 == 1 for t in range(Tc)] if dis else None
    return types.SimpleNamespace(B=B, k=k, N=N, seed=seed, encoder=encoder, dis=dis, state=state, feats=feats, fl=fl, cl=cl,
                                 caps=caps, ci=ci, masks=masks, enc_b=enc_b, st_b=st_b, eps_q=eps_q, eps_p=eps_p, flags=flags)


def oracle_repeated(c, force=None, record=None):
    """The oracle's step on the batch with every clip repeated: feats[clip_index], the clips' masks indexed likewise."""
    idx = torch.from_numpy(c.ci)
    st = {n: v.clone() for n, v in c.state.items()}
    noise = dict(dropout=[m[idx].clone() for m in c.masks], eps_q=c.eps_q, eps_p=c.eps_p, relu_force=force)
    random.seed(c.seed)
    res = _patched(c.flags, lambda: O.OracleTrainer(st, V).step(c.feats[idx], c.fl[c.ci], c.caps, c.cl, 1.0, c.dis, noise=noise,
                                                               record=record, apply_update=False))
    return res, st


def hip_shared(c, model=None):
    """The HIP model on the B clips with clip_index -> (model, outputs, loss terms, the encoder's own outputs)."""
    if model is None:
        model = build_model(V, E, c.state, c.encoder).train()
    model.encoder.dropout_masks = [m.clone() for m in c.masks]
    model.encoder.keep_saved = True
    model.noise = dict(eps_q=c.eps_q, eps_p=c.eps_p)
    box = {}
    h = model.encoder.register_forward_hook(lambda m, i, o: box.update(
        audio_embeds=o["audio_embeds"].detach().clone(), pooled=o["audio_embeds_pooled"].detach().clone(),
        lens=torch.as_tensor(o["audio_embeds_lens"]).clone()))
    random.seed(c.seed)
    fl = c.fl.copy()
    out = _patched(c.flags, lambda: model(c.feats.cuda(), fl, c.caps, c.cl, ss_ratio=1.0, dis_ratio=c.dis, clip_index=c.ci))
    h.remove()
    assert np.array_equal(fl, c.fl // (16 if c.encoder == "Cnn10" else 32))       # divided in place, as without clip_index
    return model, out, hip_loss(out, c.caps, c.cl, V), box


CASES = {
    "b3_k2_permuted": dict(B=3, k=2, seed=5),                      # 6 rows: the persistent launches
    "b3_k1_permuted": dict(B=3, k=1, seed=6),
    "b2_k5": dict(B=2, k=5, seed=7),
    "b7_k5_per_step_launches": dict(B=7, k=5, seed=8),             # 35 rows > 32: the per-step launches
    "cnn14_ln_b2_k2": dict(B=2, k=2, seed=16, encoder="Cnn14_16k"),
    "b3_k2_dis": dict(B=3, k=2, seed=10, dis=0.5),                 # the prior's z feeds the decoder at the odd steps
}


@pytest.mark.parametrize("case", list(CASES))
def test_shared_encoder_step_vs_oracle_on_the_repeated_batch(case):
    c = make_case(**CASES[case])
    cnn14 = c.encoder != "Cnn10"
    rec = {}
    ores, ost = oracle_repeated(c, record=rec)
    model, out, (loss, ce, kl, mse), enc = hip_shared(c)
    assert out["logits"].shape[0] == c.N and enc["audio_embeds"].shape[0] == c.B
    for name, got, want in (("loss", loss, ores["loss"]), ("ce", ce, ores["ce"]), ("kl", kl, ores["kl"]), ("mse", mse, ores["mse"])):
        got, want = float(got.detach()), float(want)
        print(f"{case}: {name} hip {got:.6f} oracle {want:.6f} |d| = {abs(got - want):.2e}")
        assert abs(got - want) <= 1e-4 * max(1.0, abs(want)), (name, got, want)
    assert torch.equal(out["seqs"].cpu(), ores["out"]["seqs"])
    for key in ("logits", "attn_weights", "p_means", "q_means", "q_means_utt", "p_means_utt"):
        close(out[key], ores["out"][key], 1e-4, 2e-5, what=key)
    # every output has the captions' row count; the gathered lengths are the clips'
    for key in ("seqs", "logits", "p_means", "q_means", "q_z", "p_means_utt"):
        assert out[key].shape[0] == c.N, key
    loss.backward()
    named = dict(model.named_parameters())
    idx = torch.from_numpy(c.ci)
    shim = types.SimpleNamespace(encoder=types.SimpleNamespace(
        relu_masks=lambda: [m[idx.to(m.device)] for m in model.encoder.relu_masks()]))
    grads_match_oracle(shim, named, ores["grads"], rec, lambda force: oracle_repeated(c, force=force)[0]["grads"])
    model.check_persistent_launches()
    # in front of the gather: the oracle's encoder on the B distinct clips alone
    close(enc["audio_embeds"], c.enc_b["audio_embeds"], *((2e-4, 5e-5) if cnn14 else (1e-4, 1e-5)), what="audio_embeds of the clips")
    close(enc["pooled"], c.enc_b["audio_embeds_pooled"], 2e-4 if cnn14 else 1e-4, 1e-4, what="pooled of the clips")
    assert torch.equal(enc["lens"], torch.as_tensor(c.enc_b["audio_embeds_lens"]))
    sd = model.state_dict()
    stats = [n for n in sd if n.startswith("encoder.") and "running_" in n]
    assert len(stats) == (2 * 13 if cnn14 else 2 * 9)
    for n in stats:
        tol = (1e-4, 1e-4) if cnn14 and n.endswith("running_var") else (1e-4, 1e-5)
        close(sd[n], c.st_b[n], *tol, what=n)
    for n in sd:
        if n.endswith("num_batches_tracked"):
            assert int(sd[n]) == 1, n
    if c.k > 1:
        # The Bessel factor is the clips': in the deepest BatchNorm (the fewest values per channel: B * 8 * 8 for Cnn10 at
        # T = 64, i.e. M = 192 for B = 3) the running variances of the two batches differ by momentum * var / (2M), ~1e-4 of
        # the variance's share - far above fp32 rounding; the HIP value must lie nearer to the clips' than to the repeated
        # batch's.
        n = f"encoder.conv_block{6 if cnn14 else 4}.bn2.running_var"
        to_clips = float((sd[n].cpu().double() - c.st_b[n].double()).abs().max())
        gap = float((ost[n].double() - c.st_b[n].double()).abs().max())
        print(f"{case}: {n} |hip - clips| {to_clips:.2e}, |repeated - clips| {gap:.2e}")
        assert gap > 0 and to_clips < 0.5 * gap, (n, to_clips, gap)


def test_shared_encoder_backward_is_bit_reproducible():
    c = make_case(**CASES["b3_k2_permuted"])
    model = build_model(V, E, c.state).train()
    sd = {n: v.clone() for n, v in model.state_dict().items()}
    runs = []
    for _ in range(2):
        model.load_state_dict(sd)
        for p in model.parameters():
            p.grad = None
        _, _, (loss, *_), _ = hip_shared(c, model)
        loss.backward()
        torch.cuda.synchronize()
        runs.append({n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None})
    assert runs[0].keys() == runs[1].keys() and len(runs[0]) > 50
    bad = [n for n in runs[0] if not torch.equal(runs[0][n].view(torch.int32), runs[1][n].view(torch.int32))]
    assert not bad, bad


def test_train_step_with_clip_index_matches_torch_adam_twin():
    """TrainStep.step(..., clip_index=) three times at B = 3, k = 2 against a twin: the same model, forward_loss(...,
    clip_index=), clip_grad_norm_ and torch.optim.Adam (as tests/test_resnet38_gpu.py's twin)."""
    from acvae_amd.trainer import TrainStep
    from test_optim_gpu import close as oclose
    c = make_case(**CASES["b3_k2_permuted"])
    m1 = build_model(V, E, c.state).train()
    m3 = build_model(V, E, c.state).train()
    for m in (m1, m3):
        m.encoder.p_block = m.encoder.p_fc = 0.0
    t1, t3 = TrainStep(m1, V), TrainStep(m3, V)
    opt = torch.optim.Adam([p for p in m3.parameters() if p.requires_grad], lr=5e-4)
    for step in range(3):
        if step:
            with torch.no_grad():
                for a, b in zip(m1.parameters(), m3.parameters()):
                    b.copy_(a)
        torch.manual_seed(3 + step); random.seed(3 + step)
        parts = t1.step(c.feats.cuda(), c.fl.copy(), c.caps, c.cl, 1.0, 0, 0.5, clip_index=c.ci)
        torch.manual_seed(3 + step); random.seed(3 + step)
        for p in m3.parameters():
            p.grad = None
        loss, _, out = t3.forward_loss(c.feats.cuda(), c.fl.copy(), c.caps, c.cl, 1.0, 0, 0.5, clip_index=c.ci)
        assert out["logits"].shape[0] == c.N
        loss.backward()
        torch.nn.utils.clip_grad_norm_([p for p in m3.parameters() if p.grad is not None], 1.0)
        opt.step()
        assert abs(float(parts["loss"]) - float(loss.detach())) <= 1e-6 * abs(float(loss.detach()))
        n = 0
        for (name, a), (_, b) in zip(m1.named_parameters(), m3.named_parameters()):
            if b.grad is not None:
                oclose(b, a, 1e-5, 1e-6, what=f"step {step + 1} {name}")
                n += 1
        assert n == sum(1 for p in m1.parameters() if p.grad is not None) and n > 50
    t1.synchronize()
    m3.check_persistent_launches()
