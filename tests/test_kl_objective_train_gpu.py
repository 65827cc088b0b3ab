"""GPU: TrainStep with the KL objective (kl_reduction=, free_bits=, free_bits_over=) on the golden-size model (E = 64,
B <= 4) against the oracle.

The oracle's step is the reference's loss line; here its variational term is replaced (O.train_loss is patched for the
test) by the objective's definition written in torch - torch.where for the cell set, torch.clamp for the free bits - on the
oracle's own outputs, so that autograd carries it to every parameter.  lam is placed by the oracle's first run, at the
midpoint of the widest gap in the middle half of its own sorted m_e / s_c, and every later run (the HIP step, the oracle fed
the HIP words, the oracle under the HIP path's ReLU decisions) uses that value.  Before any gradient is compared the test
asserts that the HIP outputs and the oracle's open the same gates and that no m_e / s_c lies within 100 x their largest
difference of lam.  Gradients: parity_util.grads_match_oracle with its own bounds; loss terms 1e-4 * max(1, |value|)."""
import random

import numpy as np
import pytest
import torch

import acvae_oracle as O
import kl_objective_util as K
import test_shared_encoder_gpu as SE
from acvae_amd.train_util import KLObjective, Normal_kl_loss
from acvae_amd.trainer import TrainStep
from parity_util import close, grads_match_oracle
from test_model_gpu import build_model
from test_sched_sampling_gpu import exercised, oracle_and_hip, words_match_by_margin

pytestmark = pytest.mark.gpu

GAUSS = ("q_means", "q_logs", "p_means", "p_logs")
DIAG = {"kl_raw", "kl_dims", "kl_steps", "gates_open"}


def _values(out, cap_lens, red):
    """-> (k [R,T,E], mask, D) of a forward's outputs, differentiable."""
    q_m, q_l, p_m, p_l = (out[k] for k in GAUSS)
    R, T, _ = q_m.shape
    k = p_l / 2. - q_l / 2. + (torch.exp(q_l) + (q_m - p_m) ** 2.) / (2. * torch.exp(p_l)) - .5
    mask = K.cell_mask(torch.as_tensor(np.asarray(cap_lens) - 1), R, T, red)
    return torch.where(mask[:, :, None], k, torch.zeros_like(k)), mask, int(mask.sum())


def patch_oracle_loss(monkeypatch, cfg, box):
    """O.train_loss with the KL objective in place of normal_kl_loss; the first call places box["lam"]."""
    def train_loss(out, caps, cap_lens, vocab, smoothing=0.1, kl_weight=0.5, alpha=1.0):
        lens1 = np.asarray(cap_lens) - 1
        ce = O.label_smoothing_loss(O.pack_rows(out["logits"], lens1), O.pack_rows(caps[:, 1:], lens1), vocab, smoothing)
        kS, mask, Dv = _values(out, cap_lens, cfg["red"])
        m_e, s_c = kS.sum((0, 1)) / Dv, kS.sum(-1)
        if cfg["fb"] and "lam" not in box:
            box["lam"], box["half"] = K.place_lam((m_e if cfg["over"] == "dim" else s_c[mask]).detach())
        lam = box.get("lam")
        if lam is None:
            kl = kS.sum() / Dv
        elif cfg["over"] == "dim":
            kl = torch.clamp(m_e, min=lam).sum()
        else:
            kl = torch.where(mask, torch.clamp(s_c, min=lam), torch.zeros_like(s_c)).sum() / Dv
        box["oracle"] = {"m_e": m_e.detach(), "s_c": s_c.detach(), "raw": m_e.sum().detach(), "mask": mask, "D": Dv}
        mse = torch.nn.functional.mse_loss(out["q_means_utt"], out["p_means_utt"])
        return ce + kl_weight * kl + alpha * mse, ce, kl, mse
    monkeypatch.setattr(O, "train_loss", train_loss)


def trainstep(model, V, cfg, box):
    return TrainStep(model, V, lr=5e-4, max_grad_norm=1.0, smoothing=0.1, alpha=1.0, kl_reduction=cfg["red"],
                     free_bits=box.get("lam"), free_bits_over=cfg["over"])


def check_forward(tag, cfg, box, parts, out, cl, ores):
    """Loss terms and diagnostics against the oracle's; the same gates on both sides, none near lam."""
    ora = box["oracle"]
    for name in ("ce", "kl", "mse"):
        got, want = float(parts[name]), float(ores[name])
        print(f"{tag}: {name} hip {got:.6f} oracle {want:.6f}")
        assert abs(got - want) <= 1e-4 * max(1.0, abs(want)), (name, got, want)
    assert DIAG <= set(parts)
    close(parts["kl_dims"], ora["m_e"], 1e-4, 2e-5, what="kl_dims")
    assert abs(float(parts["kl_raw"]) - float(ora["raw"])) <= 1e-4 * max(1.0, float(ora["raw"]))
    hip = K.objective(*[out[k].detach().cpu() for k in GAUSS], torch.as_tensor(np.asarray(cl) - 1), cfg["red"], box.get("lam"),
                      cfg["over"])
    assert hip["D"] == ora["D"]
    n_t = ora["mask"].sum(0).clamp_min(1)
    close(parts["kl_steps"], (ora["s_c"].sum(0) / n_t), 1e-4, 2e-5, what="kl_steps")
    if box.get("lam") is None:
        assert int(parts["gates_open"]) == out["q_means"].shape[2]
        return
    lam = box["lam"]
    if cfg["over"] == "dim":
        a, b = hip["dims"], ora["m_e"].double()
    else:
        a, b = hip["s_c"][hip["mask"]], ora["s_c"][ora["mask"]].double()
    diff, near = float((a - b).abs().max()), float((b - lam).abs().min())
    print(f"{tag}: lam {lam:.4g} (half-gap at placement {box['half']:.3g}), nearest value {near:.3g} away, largest |hip - oracle| "
          f"{diff:.2e}, {int((b > lam).sum())}/{b.numel()} gates open")
    assert near > 100 * diff, (near, diff)
    assert torch.equal(a > lam, b > lam) and 0 < int((b > lam).sum()) < b.numel()
    assert int(parts["gates_open"]) == int((b > lam).sum())


CONFIGS = {
    "valid": dict(red="valid", fb=False, over="dim"),
    "valid_dim": dict(red="valid", fb=True, over="dim"),
    "valid_cell": dict(red="valid", fb=True, over="cell"),
    "all_dim": dict(red="all", fb=True, over="dim"),
}
PLAIN = dict(V=40, E=64, B=4, Tt=96, L=7, seed=19, ss=1.0, cap_lens=[7, 5, 4, 2])
SS = dict(V=40, E=64, B=3, Tt=96, L=6, seed=11, ss=0.6)


def _run_case(tag, p, cfg, monkeypatch):
    box, got = {}, {}
    patch_oracle_loss(monkeypatch, cfg, box)

    def hip_step(model, run, batch, kw):
        feats, caps, fl, cl = batch
        ts = trainstep(model, p["V"], cfg, box)
        loss, parts, out = run(lambda: ts.forward_loss(feats.cuda(), fl.copy(), caps, cl, ss_ratio=p["ss"], dis_ratio=0,
                                                       kl_weight=0.5))
        loss.backward()
        got.update(loss=float(loss.detach()), parts=parts, out=out)
        return out["seqs"], out["logits"]

    c = oracle_and_hip(p, hip_step)
    feats, caps, fl, cl = c["batch"]
    ores = c["ores"]                                    # (the run the HIP step is to match set box["oracle"] last)
    if p["ss"] < 1:
        exercised(tag, c["rec"], caps)
        words_match_by_margin(tag, c["hip_seqs"], c["hip_logits"], ores["out"], c["rec"]["margins"])
    else:
        assert torch.equal(c["hip_seqs"], ores["out"]["seqs"])
    if cfg["red"] == "valid":
        assert int((np.asarray(cl) - 1).sum()) < len(cl) * (int(max(cl)) - 1)           # there are padded cells
    ora = dict(box["oracle"])
    want = float(ores["loss"])
    assert abs(got["loss"] - want) <= 1e-4 * max(1.0, abs(want)), (got["loss"], want)
    box["oracle"] = ora
    check_forward(tag, cfg, box, got["parts"], got["out"], cl, ores)
    grads_match_oracle(c["model"], dict(c["model"].named_parameters()), ores["grads"], c["rec"], c["under"])
    c["model"].check_persistent_launches()


@pytest.mark.parametrize("config", list(CONFIGS))
def test_forward_loss_and_every_gradient_against_the_oracle(config, monkeypatch):
    _run_case(config, PLAIN, CONFIGS[config], monkeypatch)


@pytest.mark.parametrize("config", ["valid_dim", "valid_cell"])
def test_under_scheduled_sampling_fed_the_hip_words(config, monkeypatch):
    _run_case("ss06_" + config, SS, CONFIGS[config], monkeypatch)


@pytest.mark.parametrize("config", ["valid_dim", "valid_cell"])
def test_with_clip_index_three_clips_of_two_captions(config, monkeypatch):
    cfg, box = CONFIGS[config], {}
    patch_oracle_loss(monkeypatch, cfg, box)
    c = SE.make_case(B=3, k=2, seed=5)
    rec = {}
    ores, _ = SE.oracle_repeated(c, record=rec)
    ora = dict(box["oracle"])
    model = build_model(SE.V, SE.E, c.state).train()
    model.encoder.dropout_masks = [m.clone() for m in c.masks]
    model.encoder.keep_saved = True
    model.noise = dict(eps_q=c.eps_q, eps_p=c.eps_p)
    ts = trainstep(model, SE.V, cfg, box)
    random.seed(c.seed)
    loss, parts, out = ts.forward_loss(c.feats.cuda(), c.fl.copy(), c.caps, c.cl, 1.0, 0, 0.5, clip_index=c.ci)
    assert out["q_means"].shape[0] == c.N == 6
    loss.backward()
    assert abs(float(loss.detach()) - float(ores["loss"])) <= 1e-4 * max(1.0, abs(float(ores["loss"])))
    box["oracle"] = ora
    check_forward("clip_index_" + config, cfg, box, parts, out, c.cl, ores)
    idx = torch.from_numpy(c.ci)
    import types
    shim = types.SimpleNamespace(encoder=types.SimpleNamespace(
        relu_masks=lambda: [m[idx.to(m.device)] for m in model.encoder.relu_masks()]))
    grads_match_oracle(shim, dict(model.named_parameters()), ores["grads"], rec,
                       lambda force: SE.oracle_repeated(c, force=force)[0]["grads"])
    model.check_persistent_launches()


def test_three_steps_against_a_torch_adam_twin():
    """TrainStep.step three times with kl_reduction="valid" and free bits against a twin: the same model, forward_loss,
    clip_grad_norm_ and torch.optim.Adam (as tests/test_shared_encoder_gpu.py's twin)."""
    from test_optim_gpu import close as oclose
    c = SE.make_case(B=4, k=1, seed=6, permute=False)
    m1, m3 = build_model(SE.V, SE.E, c.state).train(), build_model(SE.V, SE.E, c.state).train()
    for m in (m1, m3):
        m.encoder.p_block = m.encoder.p_fc = 0.0
    kw = dict(kl_reduction="valid", free_bits=0.05, free_bits_over="dim")
    t1, t3 = TrainStep(m1, SE.V, **kw), TrainStep(m3, SE.V, **kw)
    assert isinstance(t1.kl_loss, KLObjective)
    opt = torch.optim.Adam([p for p in m3.parameters() if p.requires_grad], lr=5e-4)
    for step in range(3):
        if step:
            with torch.no_grad():
                for a, b in zip(m1.parameters(), m3.parameters()):
                    b.copy_(a)
        torch.manual_seed(3 + step); random.seed(3 + step)
        parts = t1.step(c.feats.cuda(), c.fl.copy(), c.caps, c.cl, 1.0, 0, 0.5)
        torch.manual_seed(3 + step); random.seed(3 + step)
        for p in m3.parameters():
            p.grad = None
        loss, twin_parts, _ = t3.forward_loss(c.feats.cuda(), c.fl.copy(), c.caps, c.cl, 1.0, 0, 0.5)
        loss.backward()
        torch.nn.utils.clip_grad_norm_([p for p in m3.parameters() if p.grad is not None], 1.0)
        opt.step()
        assert abs(float(parts["loss"]) - float(loss.detach())) <= 1e-6 * abs(float(loss.detach()))
        assert DIAG <= set(parts) and 0 < int(parts["gates_open"]) <= SE.E
        assert torch.equal(parts["kl_dims"], twin_parts["kl_dims"]) and float(parts["kl"]) >= float(parts["kl_raw"]) - 1e-6
        n = 0
        for (name, a), (_, b) in zip(m1.named_parameters(), m3.named_parameters()):
            if b.grad is not None:
                oclose(b, a, 1e-5, 1e-6, what=f"step {step + 1} {name}")
                n += 1
        assert n == sum(1 for p in m1.parameters() if p.grad is not None) and n > 50
    t1.synchronize()
    m3.check_persistent_launches()


def test_the_defaults_are_normal_kl_loss_bit_for_bit():
    """TrainStep() with the defaults against a TrainStep as it was before the keywords existed - its kl_loss a Normal_kl_loss and
    nothing else on the path: the loss and every parameter after one step carry the same bits, and the diagnostics are absent."""
    c = SE.make_case(B=4, k=1, seed=6, permute=False)
    runs = []
    for explicit in (False, True):
        m = build_model(SE.V, SE.E, c.state).train()
        ts = TrainStep(m, SE.V)
        assert type(ts.kl_loss) is Normal_kl_loss and ts.kl_objective is None
        if explicit:
            ts.kl_loss, ts.kl_objective = Normal_kl_loss(), None
        torch.manual_seed(5); random.seed(5)
        parts = ts.step(c.feats.cuda(), c.fl.copy(), c.caps, c.cl, 1.0, 0, 0.5)
        ts.synchronize()
        assert not (DIAG & set(parts)) and set(parts) == {"ce", "kl", "mse", "loss", "grad_norm"}
        runs.append((parts, {n: p.detach().clone() for n, p in m.named_parameters()}))
    (pa, a), (pb, b) = runs
    for key in ("loss", "ce", "kl", "mse"):
        assert torch.equal(pa[key].view(-1).view(torch.int32), pb[key].view(-1).view(torch.int32)), key
    bad = [n for n in a if not torch.equal(a[n].view(torch.int32), b[n].view(torch.int32))]
    assert not bad, bad
