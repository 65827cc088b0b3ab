"""CPU: the oracle's bf16-storage encoder (cnn10_forward(..., enc_storage="bf16"), the reference the bf16 HIP encoder is held
to in test_bf16_oracle_gpu.py).  The default arithmetic is untouched; in the bf16 mode every tensor the bf16 kernels store,
and the gradient of each, is a bf16 value, the weights with Cin >= 64 are multiplied as bf16 while their gradients stay fp32,
and the first convolution keeps fp32 weights."""
import numpy as np
import pytest
import torch

import acvae_oracle as O


def enc_state(encoder="Cnn10", dtype=torch.float32):
    width = 512 if encoder == "Cnn10" else 2048
    shapes = {k: v for k, v in O.state_shapes(10, enc_embed=width, encoder=encoder).items() if k.startswith("encoder.")}
    st = O.closed_form_state(shapes)
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in st.items()}


def is_bf16(t):
    t = t.detach()
    return bool(torch.equal(t.float().bfloat16().to(t.dtype), t))


def run(st, feats, storage, masks=None, force=None, rec=None, probe=None, training=True):
    keys = O.trainable_keys(st)
    for k in keys:
        st[k].requires_grad_(True)
        st[k].grad = None
    torch.manual_seed(5)
    o = O.cnn10_forward(st, feats, [feats.shape[1]] * feats.shape[0], training, masks, rec, relu_probe=probe,
                        relu_force=force, enc_storage=storage)
    R = torch.randn(o["audio_embeds"].shape, generator=torch.Generator().manual_seed(9), dtype=feats.dtype)
    (o["audio_embeds"] * R).sum().backward()
    return o, {k: st[k].grad.clone() for k in keys if st[k].grad is not None}


def test_default_storage_is_the_fp32_arithmetic_bit_for_bit():
    feats = torch.randn(2, 48, 64, generator=torch.Generator().manual_seed(1)) * 1.5 + 0.3
    outs = []
    for kw in ({}, {"enc_storage": "f32"}):
        st = enc_state()
        keys = O.trainable_keys(st)
        for k in keys:
            st[k].requires_grad_(True)
        torch.manual_seed(5)
        o = O.cnn10_forward(st, feats, [48, 48], True, None, None, **kw)
        o["audio_embeds"].sum().backward()
        outs.append((o["audio_embeds"].detach(), {k: st[k].grad for k in keys if st[k].grad is not None},
                     {k: v.detach() for k, v in st.items()}))
    (a0, g0, s0), (a1, g1, s1) = outs
    assert torch.equal(a0, a1)
    assert set(g0) == set(g1) and all(torch.equal(g0[k], g1[k]) for k in g0)
    assert all(torch.equal(s0[k], s1[k]) for k in s0)
    with pytest.raises(ValueError):
        O.cnn10_forward(enc_state(), feats, [48, 48], True, enc_storage="fp16")


@pytest.mark.parametrize("encoder,T,dtype", [("Cnn10", 40, torch.float32), ("Cnn10", 35, torch.float64),
                                             ("Cnn14_16k", 64, torch.float32)])
def test_bf16_storage_rounds_where_the_kernels_round(monkeypatch, encoder, T, dtype):
    """Spies on the two rounding ops: what `store` returns and the gradient it hands back are bf16 values, there are
    four stored tensors per block (Y1, relu(bn1(Y1)), Y2, P), and every 3x3 weight but conv_block1.conv1 goes
    through `wround`; the weight gradients themselves are not rounded."""
    st = enc_state(encoder, dtype)
    nb = len(O.ENCODERS[encoder]["channels"])
    stored, sgrads, wrounded = [], [], []
    orig_store, orig_wround = O._store, O._wround

    def spy_store(x):
        y = orig_store(x)
        stored.append(y.detach())
        if x.requires_grad:
            x.register_hook(lambda g: sgrads.append(g.detach()))
        return y

    def spy_wround(w):
        wrounded.append(w)
        return orig_wround(w)
    monkeypatch.setattr(O, "_store", spy_store)
    monkeypatch.setattr(O, "_wround", spy_wround)
    feats = (torch.randn(2, T, 64, generator=torch.Generator().manual_seed(3)) * 1.5 + 0.3).to(dtype)
    o, grads = run(st, feats, "bf16")
    assert len(stored) == 4 * nb and len(sgrads) == 4 * nb
    assert all(t.dtype == dtype and is_bf16(t) for t in stored)
    assert all(g.dtype == dtype and is_bf16(g) for g in sgrads)
    assert all(float(g.abs().max()) > 0 for g in sgrads)
    conv_w = [f"encoder.conv_block{b}.conv{i}.weight" for b in range(1, nb + 1) for i in (1, 2)]
    assert [id(w) for w in wrounded] == [id(st[k]) for k in conv_w[1:]]
    # conv_block1.conv1 multiplies the fp32 weights: its weights have more than 8 significant bits and are used as they are
    assert not is_bf16(st["encoder.conv_block1.conv1.weight"])
    # the weight gradients stay fp32 (the kernels return them in fp32)
    for k in conv_w:
        assert grads[k].dtype == dtype and not is_bf16(grads[k]), k
    assert o["audio_embeds"].dtype == dtype and not is_bf16(o["audio_embeds"])


@pytest.mark.parametrize("encoder", ["Cnn10", "Cnn14_16k"])
def test_bf16_storage_is_not_a_no_op(encoder):
    """Against the fp32 oracle on the same weights, batch and dropout masks, under the same ReLU decisions (the fp32 run's
    z > 0 forced on the bf16 one, so that the difference is the rounding alone): the output and every gradient tensor move
    by far more than fp32 rounding (measured: output 2.1e-2 / 8.1e-2, gradients from 1.6e-3; BatchNorm over a few values
    in Cnn14's last blocks amplifies some bias gradients to 0.6)."""
    feats = torch.randn(2, 64, 64, generator=torch.Generator().manual_seed(4)) * 1.5 + 0.3
    rec, probe = [], []
    o32, g32 = run(enc_state(encoder), feats, "f32", rec=rec, probe=probe)
    force = {i: z > 0 for i, z in enumerate(probe)}
    o16, g16 = run(enc_state(encoder), feats, "bf16", masks=[m.clone() for m in rec], force=force)
    assert set(g32) == set(g16)

    def rel(a, b):
        return float((a.double() - b.double()).norm() / b.double().norm())
    e_out = rel(o16["audio_embeds"].detach(), o32["audio_embeds"].detach())
    e_grad = {k: rel(g16[k], g32[k]) for k in g32}
    worst = max(e_grad, key=e_grad.get)
    print(f"{encoder}: bf16 vs fp32 oracle under the same ReLU decisions: output {e_out:.2e}, gradients "
          f"{min(e_grad.values()):.2e} .. {e_grad[worst]:.2e} ({worst})")
    assert 1e-3 < e_out < 0.2
    assert all(v > 1e-4 for v in e_grad.values()), min(e_grad.items(), key=lambda kv: kv[1])
    assert all(bool(torch.isfinite(g).all()) for g in g16.values())


def test_trainer_threads_the_storage_mode():
    """OracleTrainer(..., enc_storage=) reaches the encoder: the loss of a whole training step moves, the text side's
    arithmetic is the same."""
    V, E = 40, 32
    losses = {}
    for mode in ("f32", "bf16"):
        st = O.closed_form_state(O.state_shapes(V, E, E, None, E, 512))
        feats, caps, fl, cl = O.synthetic_batch(2, 64, V, 6, seed=4)
        torch.manual_seed(4)
        import random
        random.seed(4)
        r = O.OracleTrainer(st, V, enc_storage=mode).step(feats, fl.copy(), caps, cl, 1.0, 0, apply_update=False)
        losses[mode] = float(r["loss"])
    assert losses["f32"] != losses["bf16"]
    assert abs(losses["f32"] - losses["bf16"]) < 1e-2 * abs(losses["f32"])
    assert np.isfinite(losses["bf16"])
