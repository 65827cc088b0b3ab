"""GPU: the bf16-storage encoder (compute_dtype="bf16", BASELINE configs[2]) against the oracle in the same arithmetic
(acvae_oracle.cnn10_forward(..., enc_storage="bf16"): the same tensors and gradients rounded to bf16 at the same points),
tensor by tensor, under the HIP path's own ReLU decisions - the bf16 twin of test_encoder_gpu.py's encoder_grads_vs_oracle
(Cnn10, Cnn14_16k, training with explicit dropout masks, evaluation) and of test_fullsize_grads_gpu.py (configs[2]).

What separates two correct implementations here is not fp32 rounding but where an fp32 sum lands next to a bf16 rounding
midpoint: a different summation order rounds some stored values one bf16 step (2^-8) the other way, and BatchNorm, ReLU and
the next layers carry that on, more with every layer.  The yardstick is therefore measured, not assumed: the reference is
the oracle in float64, and the same oracle in fp32 (same rounding points, another summation order) shows how far a correct
implementation may be from it.  Every tensor of the HIP path must be within MARGIN x that distance (floor FLOOR), and its
ReLU decisions may differ from the float64 replay's z > 0 only within FLIP_REL x (|shift| + rms of z) of their channel:
near z = 0 the stored value sits at -shift / scale, so one bf16 step of it moves z by 2^-8 |shift|, and the fp32 oracle's
own decisions differ from the float64 ones by up to 0.23 of that scale in Cnn14_16k's last blocks."""
import os
import random

import pytest
import torch

import acvae_oracle as O
from test_bf16_gpu import build
from test_encoder_gpu import cnn14_state, make_cnn14, make_encoder
from test_fullsize_gpu import L, V
from test_model_gpu import hip_loss

pytestmark = pytest.mark.gpu

FLIP_REL = 0.5           # measured: the fp32 oracle 0.23, the HIP path 0.21 (Cnn14_16k blocks 5 and 6)
# every tensor within MARGIN x the fp32 oracle's distance from the float64 one (FLOOR: below it a distance counts as FLOOR).
# Measured worst ratio: 2.35 Cnn10 (bn0.weight, evaluation), 1.38 at full size; Cnn14_16k 5.3 (conv_block6.bn1.running_var,
# statistics of 32 values), which gets MARGIN_CNN14.
MARGIN, MARGIN_CNN14, FLOOR = 4.0, 8.0, 1e-4


def rel_l2(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).pow(2).sum().sqrt() / max(float(b.pow(2).sum().sqrt()), 1e-30))


def channel_rms(z):
    """rms over N, H, W of each channel of z [N,C,H,W], shaped [1,C,1,1]."""
    return z.double().pow(2).mean((0, 2, 3), keepdim=True).sqrt().clamp_min(1e-30)


def site_scales(st0, st1, zs, training, prefix="encoder"):
    """Per ReLU site, [1,C,1,1]: |shift| + rms(z) of each channel of the BatchNorm in front of it (shift = beta - mean * scale,
    scale = gamma / sqrt(var + eps)), from the oracle's state before (st0) and after (st1) its forward: in training the batch
    statistics are what the forward added to the running buffers."""
    out = []
    for i, z in enumerate(zs):
        p = f"{prefix}.conv_block{i // 2 + 1}.bn{i % 2 + 1}"
        f = lambda k, s: s[f"{p}.{k}"].detach().double()
        n = z.shape[0] * z.shape[2] * z.shape[3]
        if training:
            mean = (f("running_mean", st1) - 0.9 * f("running_mean", st0)) / 0.1
            var = (f("running_var", st1) - 0.9 * f("running_var", st0)) / 0.1 * (n - 1) / n
        else:
            mean, var = f("running_mean", st0), f("running_var", st0)
        scale = f("weight", st0) / torch.sqrt(var + 1e-5)
        shift = f("bias", st0) - mean * scale
        out.append(shift.abs().view(1, -1, 1, 1) + channel_rms(z))
    return out


def flip_report(masks, zs, scales):
    """(flips, largest |z| / scale among them, per-site 'site:flips@ratio' for the sites that have any)"""
    nflip, zmax, per = 0, 0.0, []
    for i, (m, z, sc) in enumerate(zip(masks, zs, scales)):
        d = m != (z > 0)
        if bool(d.any()):
            r = float((z.abs() / sc)[d].max())
            nflip += int(d.sum()); zmax = max(zmax, r)
            per.append(f"{i}:{int(d.sum())}@{r:.1e}/{float((z.abs() / channel_rms(z))[d].max()):.1e}")
    return nflip, zmax, " ".join(per)


def oracle_pair(state, feats, run):
    """run(state, feats) -> (output, grads) with the oracle in float64 and in fp32 on the same inputs: (ref, alt)"""
    s64 = {k: (v.detach().clone().double() if v.is_floating_point() else v.clone()) for k, v in state.items()}
    s32 = {k: v.detach().clone() for k, v in state.items()}
    return run(s64, feats.double()), run(s32, feats.float())


def within_margin(errs, alt, what, margin=MARGIN):
    """errs / alt: {name: relative L2 of the HIP path / of the fp32 oracle, both against the float64 oracle}"""
    ratio = {k: errs[k] / max(alt[k], FLOOR) for k in errs}
    worst = max(ratio, key=ratio.get)
    we = max(errs, key=errs.get)
    print(f"{what}: worst HIP/fp32-oracle ratio {worst} {ratio[worst]:.2f} ({errs[worst]:.2e} vs {alt[worst]:.2e}); "
          f"largest HIP distance {we} {errs[we]:.2e} (fp32 oracle {alt[we]:.2e})")
    assert ratio[worst] <= margin, f"{what}: {worst} is {errs[worst]:.2e} from the float64 bf16 oracle, " \
                                   f"{ratio[worst]:.1f} x the fp32 oracle's {alt[worst]:.2e}"


def bf16_encoder_vs_oracle(full, make, head, feats, R, lens, training=True):
    """The bf16 HIP encoder vs the bf16 oracle under the HIP path's ReLU decisions (encoder.relu_masks(), read back from the
    bf16 activations and replayed with relu_force), every parameter gradient, audio_embeds and in training the running
    statistics; explicit dropout masks in training."""
    enc_state = {k: v for k, v in full.items() if k.startswith("encoder.")}
    rec = []
    torch.manual_seed(5)
    with torch.no_grad():
        O.cnn10_forward({k: v.clone() for k, v in enc_state.items()}, feats, list(lens), training, None, rec,
                        enc_storage="bf16")
    enc = make(full)
    enc.compute_dtype = "bf16"
    enc.train(training)
    enc.keep_saved = True
    enc.dropout_masks = [m.clone() for m in rec] if training else None
    out = enc(feats.cuda(), list(lens))
    masks = [m.cpu() for m in enc.relu_masks()]
    (out["audio_embeds"] * R.cuda()).sum().backward()

    def run(st, f):
        for k in O.trainable_keys(st):
            st[k].requires_grad_(True)
        probe = []
        o = O.cnn10_forward(st, f, list(lens), training, [m.clone() for m in rec] if training else None, None,
                            relu_probe=probe, relu_force={i: m for i, m in enumerate(masks)}, enc_storage="bf16")
        (o["audio_embeds"] * R.to(f.dtype)).sum().backward()
        return st, probe, o["audio_embeds"].detach()
    (s64, z64, ae64), (s32, z32, ae32) = oracle_pair(enc_state, feats, run)
    scales = site_scales(full, s64, z64, training)
    nflip, zmax, per = flip_report(masks, z64, scales)
    _, zalt, _ = flip_report([z > 0 for z in z32], z64, scales)
    print(f"ReLU decisions that differ from the float64 replay, per site (count @ |z| / scale / |z| / rms): {per}; "
          f"the fp32 oracle's at most {zalt:.2e} x scale")
    assert zmax < FLIP_REL, f"{nflip} ReLU decisions differ from the bf16 oracle, one at |z| = {zmax:.2e} x its scale"
    named, sd = dict(enc.named_parameters()), enc.state_dict()
    errs = {"audio_embeds": rel_l2(out["audio_embeds"], ae64)}
    alt = {"audio_embeds": rel_l2(ae32, ae64)}
    for k in O.trainable_keys(s64):
        kk = k[len("encoder."):]
        if kk.startswith(head):
            assert named[kk].grad is None and s64[k].grad is None
            continue
        assert bool(torch.isfinite(named[kk].grad).all()), kk
        errs[kk] = rel_l2(named[kk].grad, s64[k].grad)
        alt[kk] = rel_l2(s32[k].grad, s64[k].grad)
    if training:
        # running statistics: the batch's part (running = 0.9 old + 0.1 batch), so that the old value does not hide it
        for k in s64:
            kk = k[len("encoder."):]
            if k.endswith(("running_mean", "running_var")):
                old = 0.9 * full[k].double()
                errs[kk] = rel_l2(sd[kk].cpu().double() - old, s64[k] - old)
                alt[kk] = rel_l2(s32[k].double() - old, s64[k] - old)
            elif k.endswith("num_batches_tracked"):
                assert int(sd[kk]) == int(s64[k]) == 1, k
    return nflip, zmax, errs, alt


@pytest.mark.parametrize("B,Tt,seed,training", [(2, 64, 1, True), (3, 999, 2, True), (2, 250, 3, False)],
                         ids=["B2_T64", "B3_T999", "B2_T250_eval"])
def test_cnn10_bf16_vs_bf16_oracle(B, Tt, seed, training):
    """T = 999: odd heights 999 / 499 / 249 in front of the pools.  Evaluation mode: running statistics in the forward and
    the backward, whose data-gradient filters are repacked into scratch (the forward built none)."""
    full = O.closed_form_state(O.state_shapes(10))
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(B, Tt, 64, generator=g) * 1.5 + 0.3
    R = torch.randn(B, Tt // 16, 512, generator=g)
    nflip, zmax, errs, alt = bf16_encoder_vs_oracle(full, make_encoder, "embed_pooled", feats, R, [Tt] * B, training)
    within_margin(errs, alt, f"Cnn10 bf16 B={B} T={Tt} training={training} ({nflip} decisions differ, max {zmax:.1e})")


def test_cnn14_bf16_vs_bf16_oracle():
    full = cnn14_state()
    g = torch.Generator().manual_seed(6)
    feats = torch.randn(4, 128, 64, generator=g) * 1.5 + 0.3
    R = torch.randn(4, 128 // 32, 2048, generator=g)
    nflip, zmax, errs, alt = bf16_encoder_vs_oracle(full, make_cnn14, "fc1", feats, R, [128] * 4)
    within_margin(errs, alt, f"Cnn14_16k bf16 B=4 T=128 ({nflip} decisions differ, max {zmax:.1e})", MARGIN_CNN14)


# ------------------------------------------------------------------------------------------------ full size
SEED = 9
FULL = {"B32_T1000": dict(B=32, T=1000), "B3_T1601": dict(B=3, T=1601)}


@pytest.mark.parametrize("case", list(FULL))
def test_every_parameter_gradient_bf16_vs_bf16_oracle_at_full_size(case):
    """configs[2] (B=32, T=1000, V=5000, E=512) and B=3, T=1601 through the whole model: the bf16 HIP model against
    OracleTrainer(..., enc_storage="bf16") on the same weights, batch and noise, replayed under the HIP path's ReLU decisions
    in float64 and in fp32 - the loss terms, the teacher-forced tokens (where the decision margin is clear) and every
    parameter gradient, encoder and text side, within MARGIN x the fp32 oracle's distance."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    B, T = FULL[case]["B"], FULL[case]["T"]
    model = build(5, dtype="bf16").train()
    state = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    feats, caps, fl, cl = O.synthetic_batch(B, T, V, L, seed=4, ragged=True)
    rec = {}
    with torch.no_grad():                        # the oracle's draws: dropout masks, eps
        torch.manual_seed(SEED); random.seed(SEED)
        O.hybrid_forward({k: v.clone() for k, v in state.items()}, feats, fl.copy(), caps, cl, ss_ratio=1.0, dis_ratio=0,
                         record=rec, enc_storage="bf16")
    model.encoder.dropout_masks = rec["dropout"]
    model.encoder.keep_saved = True
    model.noise = dict(eps_q=rec["eps_q"], eps_p=rec["eps_p"])
    torch.manual_seed(SEED); random.seed(SEED)
    out = model(feats.cuda(), fl.copy(), caps, cl, ss_ratio=1.0, dis_ratio=0)
    hl = hip_loss(out, caps, cl, V)
    hl[0].backward()
    torch.cuda.synchronize()
    masks = [m.cpu() for m in model.encoder.relu_masks()]
    del rec["relu_z"]

    def run(st, f):
        noise = dict(dropout=[m.clone() for m in rec["dropout"]], eps_q=rec["eps_q"].to(f.dtype),
                     eps_p=rec["eps_p"].to(f.dtype), relu_force={i: m for i, m in enumerate(masks)})
        torch.manual_seed(SEED); random.seed(SEED)
        r = O.OracleTrainer(st, V, enc_storage="bf16").step(f, fl.copy(), caps, cl, 1.0, 0, noise=noise, apply_update=False)
        return {k: r[k] for k in ("loss", "ce", "kl", "mse", "grads")} | {"logits": r["out"]["logits"].detach(),
                                                                          "seqs": r["out"]["seqs"]}
    r64, r32 = oracle_pair(state, feats, run)
    terms = {}
    for i, name in enumerate(("loss", "ce", "kl", "mse")):
        want, alt = float(r64[name]), float(r32[name])
        terms[name] = abs(float(hl[i].detach()) - want) / max(1.0, abs(want))
        assert terms[name] <= max(MARGIN * abs(alt - want) / max(1.0, abs(want)), 1e-5), (name, float(hl[i]), want, alt)
    # teacher-forced greedy tokens: equal wherever the float64 oracle's decision margin exceeds 20x the largest logit difference
    lg_h, lg_o = out["logits"].detach().cpu().double(), r64["logits"].double()
    dlog = float((lg_h - lg_o).abs().max())
    margin = O.decision_margin(lg_o.reshape(-1, lg_o.shape[-1]), "greedy").reshape(lg_o.shape[:2])
    valid = torch.arange(lg_o.shape[1]).unsqueeze(0) < (torch.as_tensor(cl) - 1).unsqueeze(1)
    differ = (out["seqs"].cpu() != r64["seqs"]) & valid
    assert not bool((differ & (margin > 20 * dlog)).any()), f"{int(differ.sum())} tokens differ, largest logit diff {dlog:.2e}"
    named = dict(model.named_parameters())
    assert set(k for k, p in named.items() if p.grad is not None) == set(r64["grads"])
    errs = {k: rel_l2(named[k].grad, g) for k, g in r64["grads"].items()}
    alt = {k: rel_l2(r32["grads"][k], g) for k, g in r64["grads"].items()}
    print(f"bf16 full size {case}: loss terms {', '.join(f'{k} {v:.1e}' for k, v in terms.items())}; "
          f"{int(differ.sum())} tokens differ (logits {dlog:.1e})")
    within_margin(errs, alt, f"bf16 full size {case}")
