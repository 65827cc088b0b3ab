"""ResNet38 encoder without a GPU: the reference's state-dict layout and initialisation, the PANNs checkpoint loader,
and the host arithmetic of the C ABI for ACVAE_ARCH_RESNET38."""
import ctypes
import os

import numpy as np
import pytest
import torch

from acvae_amd import _lib
from acvae_amd.encoder import ResNet38
from acvae_amd.train_util import load_pretrained_model
from conftest import load_golden

ARCH = 2


def golden_keys():
    g = load_golden("g17_resnet38_encoder")
    keys = [str(k) for k in g["keys"]]
    shapes = [tuple(int(x) for x in g["shapes"][i][:int(g["ndims"][i])]) for i in range(len(keys))]
    return keys, shapes


def test_state_dict_matches_reference_layout():
    keys, shapes = golden_keys()
    sd = ResNet38(64, 2048).state_dict()
    assert list(sd.keys()) == keys
    assert [tuple(v.shape) for v in sd.values()] == shapes
    assert len(keys) == 241
    assert sum(v.numel() for k, v in sd.items() if "running" not in k and "num_batches" not in k) == 72_703_424
    # a state dict in the reference's layout loads strictly
    ref = {k: torch.randn(s) if "num_batches" not in k else torch.tensor(3) for k, s in zip(keys, shapes)}
    m = ResNet38(64, 2048)
    m.load_state_dict(ref, strict=True)
    assert torch.equal(m.resnet.layer3[0].downsample[1].weight,
                       ref["resnet.layer3.0.downsample.1.weight"])


def test_param_table_is_state_dict_order():
    m = ResNet38(64, 2048)
    t = m._param_table()
    sd = m.state_dict(keep_vars=True)
    assert len(t) == 241 == _lib.lib().acvae_encoder_nparams(ARCH)
    assert all(a is b for a, b in zip(t, sd.values()))


def test_initialisation_rules():
    torch.manual_seed(0)
    m = ResNet38(64, 2048)
    blocks = m.resnet.blocks()
    assert len(blocks) == 16
    for b in blocks:
        assert bool((b.bn2.weight == 0).all())
        assert bool((b.bn1.weight == 1).all())
    for name, mod in m.named_modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            assert bool((mod.bias == 0).all()), name
            if not name.endswith("bn2") or not name.startswith("resnet"):
                assert bool((mod.weight == 1).all()), name
        if isinstance(mod, torch.nn.Conv2d):
            w = mod.weight
            fan_in, fan_out = w.shape[1] * w[0, 0].numel(), w.shape[0] * w[0, 0].numel()
            bound = (6.0 / (fan_in + fan_out)) ** 0.5
            assert float(w.abs().max()) <= bound * (1 + 1e-6), name      # (fp32 rounding of the bound)
            assert float(w.abs().max()) > 0.5 * bound, name          # Xavier-uniform, not PyTorch's default
    assert bool((m.fc1.bias == 0).all())
    assert sum(1 for mm in m.modules() if isinstance(mm, torch.nn.Conv2d)) == 39


def test_bf16_is_refused():
    m = ResNet38(64, 2048, compute_dtype="bf16")
    with pytest.raises(ValueError):
        m._arch()


def test_load_pretrained_model(tmp_path):
    src = ResNet38(64, 2048)
    with torch.no_grad():
        for p in src.parameters():
            p.add_(1.0)
    ck = dict(src.state_dict())
    ck["spectrogram_extractor.stft.conv_real.weight"] = torch.randn(513, 1, 1024)
    ck["logmel_extractor.melW"] = torch.randn(513, 64)
    ck["fc_audioset.weight"] = torch.randn(527, 2048)
    ck["fc_audioset.bias"] = torch.randn(527)
    ck["fc1.weight"] = torch.randn(10, 2048)                      # shape mismatch: left alone
    path = str(tmp_path / "panns.pth")
    torch.save({"model": ck}, path)
    dst = ResNet38(64, 2048)
    before = dst.fc1.weight.detach().clone()
    log = []
    load_pretrained_model(dst, path, log.append)
    assert not log
    sd = dst.state_dict()
    for k, v in src.state_dict().items():
        if k != "fc1.weight":
            assert torch.equal(sd[k], v), k
    assert torch.equal(dst.fc1.weight, before)
    assert "fc_audioset.weight" not in sd
    # a bare state dict (no "model" wrapper) loads the same
    path2 = str(tmp_path / "bare.pth")
    torch.save(src.state_dict(), path2)
    dst2 = ResNet38(64, 2048)
    load_pretrained_model(dst2, path2, log.append)
    assert torch.equal(dst2.fc1.weight, src.fc1.weight)
    # a missing file only logs
    dst3 = ResNet38(64, 2048)
    keep = {k: v.clone() for k, v in dst3.state_dict().items()}
    load_pretrained_model(dst3, str(tmp_path / "missing.pth"), log.append)
    assert len(log) == 1 and "missing.pth" in log[0]
    assert all(torch.equal(keep[k], v) for k, v in dst3.state_dict().items())


def test_abi_host_arithmetic():
    L = _lib.lib()
    S, C = ctypes.c_int(), ctypes.c_int()
    assert L.acvae_encoder_out_dims(ARCH, 1000, ctypes.byref(S), ctypes.byref(C)) == 0 and (S.value, C.value) == (31, 2048)
    assert L.acvae_encoder_out_dims(ARCH, 72, ctypes.byref(S), ctypes.byref(C)) == 0 and S.value == 2
    assert L.acvae_encoder_out_dims(ARCH, 31, ctypes.byref(S), ctypes.byref(C)) == -1
    assert L.acvae_encoder_out_dims(ARCH | _lib.ENC_BF16, 64, ctypes.byref(S), ctypes.byref(C)) == -1
    assert L.acvae_encoder_nparams(ARCH) == 241 and L.acvae_encoder_nparams(ARCH | _lib.ENC_BF16) == -1
    assert L.acvae_encoder_nparams(0) == 55 and L.acvae_encoder_nparams(1) == 79
    for f in ("acvae_encoder_saved_bytes", "acvae_encoder_scratch_bytes"):
        a = _lib.call(f, ARCH, 2, 64, 64)
        b = _lib.call(f, ARCH, 4, 64, 64)
        assert a > 0 and b > a and a % 16 == 0
        assert _lib.call(f, ARCH, 2, 31, 64) == -1                 # T < 32
        assert _lib.call(f, ARCH, 2, 64, 63) == -1                 # F != 64
        assert _lib.call(f, ARCH | _lib.ENC_BF16, 2, 64, 64) == -1
        assert _lib.call(f, ARCH, 0, 64, 64) == -1
    # saved holds at least every activation the backward reads: per block y1, h1, y2, out (+ pooled input, downsample)
    assert _lib.call("acvae_encoder_saved_bytes", ARCH, 32, 1000, 64) > 4 * 32 * 500 * 32 * 64 * 4 * 3
    # refusals before any launch: null pointers / bad shapes come back as ACVAE_EINVAL without touching a device
    null = ctypes.c_void_p(0)
    assert L.acvae_encoder_fwd(null, null, null, null, null, ctypes.c_int64(0), null, ctypes.c_int64(0), ARCH, 2, 31, 64, 1,
                               ctypes.c_float(0.2), ctypes.c_float(0.5), ctypes.c_uint64(0), null, null) == -1
    assert L.acvae_encoder_fwd(null, null, null, null, null, ctypes.c_int64(0), null, ctypes.c_int64(0), ARCH | _lib.ENC_BF16,
                               2, 64, 64, 1, ctypes.c_float(0.2), ctypes.c_float(0.5), ctypes.c_uint64(0), null, null) == -1
    assert L.acvae_encoder_bwd(null, null, null, null, null, ctypes.c_int64(0), null, ctypes.c_int64(0), ARCH, 2, 64, 63, 1,
                               ctypes.c_float(0.2), ctypes.c_uint64(0), null, null) == -1
    assert L.acvae_encoder_relu_mask(null, ctypes.c_int64(0), ARCH, 2, 64, 64, 36, null, null) == -1


def test_site_shapes():
    relu, drop = ResNet38(64, 2048).site_shapes(2, 200)
    assert len(relu) == 36 and len(drop) == 21
    assert drop[0] == (2, 64, 100, 32) and drop[4] == (2, 128, 50, 16) and drop[16] == (2, 512, 12, 4)
    assert drop[17] == (2, 512, 6, 2) and drop[19] == (2, 2048)
    assert relu[0] == (2, 64, 200, 64) and relu[35] == (2, 2048, 6, 2)
