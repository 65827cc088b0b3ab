"""Write tests/golden/g17_resnet38_encoder.npz from the reference's ResNet38 (models/encoder.py:1169-1234), on the CPU.

The reference is imported at run time through oracle/ref_shim.py; only arrays are stored: the reference's state-dict key
list and shapes, inputs, train-mode outputs with the 21 dropout keep-masks (bit-packed, NCHW / [N,2048]), eval-mode
outputs, selected running statistics and num_batches_tracked after the train forward, and the mutated lens.  Parameters
are acvae_oracle.closed_form_state over the reference's shapes (not stored: the model is 291 MB).

Masks are recorded by wrapping torch.nn.functional.dropout with the draw ATen's CPU dropout makes
(empty_like(x).bernoulli_(1 - p), then / (1 - p)); the tool checks that the wrapped run reproduces the unwrapped output
bit for bit under the same seed.  Run: python tools/make_resnet38_golden.py  (deterministic: regenerates identical bytes)."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import acvae_oracle as O  # noqa: E402
import ref_shim  # noqa: E402

CASES = [(2, 64), (3, 96), (2, 200)]
STATS = ["bn0.running_mean", "conv_block1.bn2.running_var", "resnet.layer2.0.downsample.2.running_mean",
         "resnet.layer3.4.bn1.running_var", "resnet.layer4.2.bn2.running_mean", "conv_block_after1.bn2.running_var"]


def recorded_dropout(masks):
    def dropout(x, p=0.5, training=True, inplace=False):
        if not training or p == 0.0:
            return x
        noise = torch.empty_like(x).bernoulli_(1 - p)
        masks.append(noise.bool().clone())
        noise.div_(1 - p)
        return x.mul_(noise) if inplace else x * noise
    return dropout


def run(model, feats, lens, seed, masks=None):
    torch.manual_seed(seed)
    orig = F.dropout
    if masks is not None:
        F.dropout = recorded_dropout(masks)
    try:
        out = model(feats.clone(), lens)
    finally:
        F.dropout = orig
    return out


def main():
    ref_shim.load()
    import models.encoder as E
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    probe = E.ResNet38(64, 2048)
    shapes = {k: tuple(v.shape) for k, v in probe.state_dict().items()}
    keys = list(shapes)
    out = {"keys": np.array(keys), "ndims": np.array([len(s) for s in shapes.values()], dtype=np.int64),
           "shapes": np.array([list(s) + [0] * (4 - len(s)) for s in shapes.values()], dtype=np.int64)}
    state = O.closed_form_state(shapes)
    for ci, (B, T) in enumerate(CASES):
        g = torch.Generator().manual_seed(100 + ci)
        feats = torch.randn(B, T, 64, generator=g)
        lens = np.array([T - 5 * i for i in range(B)], dtype=np.int64)
        p = f"c{ci}_"
        out[p + "feats"] = feats.numpy()
        out[p + "lens"] = lens.copy()
        seed = 7 + ci
        m0 = E.ResNet38(64, 2048)
        m0.load_state_dict(state)
        m0.train()
        plain = run(m0, feats, torch.as_tensor(lens.copy()), seed)
        m = E.ResNet38(64, 2048)
        m.load_state_dict(state)
        m.train()
        masks = []
        lt = torch.as_tensor(lens.copy())
        o = run(m, feats, lt, seed, masks)
        assert len(masks) == 21, len(masks)
        for k in ("audio_embeds", "audio_embeds_pooled"):
            assert torch.equal(o[k], plain[k]), f"the recorded dropout does not reproduce the reference ({k})"
        out[p + "train_audio_embeds"] = o["audio_embeds"].detach().numpy()
        out[p + "train_pooled"] = o["audio_embeds_pooled"].detach().numpy()
        out[p + "lens_after"] = lt.numpy().copy()
        for i, mk in enumerate(masks):
            out[p + f"noise_drop{i}_bits"] = np.packbits(mk.numpy().astype(np.uint8).reshape(-1))
            out[p + f"noise_drop{i}_shape"] = np.array(mk.shape)
        sd = m.state_dict()
        for k in STATS:
            out[p + "stat_" + k] = sd[k].numpy().copy()
        out[p + "nbt"] = np.array(int(sd["resnet.layer3.0.bn2.num_batches_tracked"]))
        me = E.ResNet38(64, 2048)
        me.load_state_dict(state)
        me.eval()
        with torch.no_grad():
            oe = me(feats.clone(), torch.as_tensor(lens.copy()))
        out[p + "eval_audio_embeds"] = oe["audio_embeds"].numpy()
        out[p + "eval_pooled"] = oe["audio_embeds_pooled"].numpy()
    dst = os.path.join(ROOT, "tests", "golden", "g17_resnet38_encoder.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
