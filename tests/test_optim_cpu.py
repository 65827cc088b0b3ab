"""CPU: the fused AdamW / SGD entry points are exported and refuse bad arguments without a device; TrainStep's
optimizer name and option resolution (acvae_amd.optim.resolve) follows torch.optim and rejects what the fused update
does not implement."""
import ctypes

import pytest
import torch

import __graft_entry__ as ge
from acvae_amd import _lib
from acvae_amd.optim import resolve


def test_new_optimizer_symbols_are_exported_and_parsed():
    ge.build()
    protos, _ = _lib.parse_header()
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("acvae_adamw_step", 18), ("acvae_sgd_step", 14)):
        assert name in protos, f"{name} not declared in include/acvae_hip.h"
        assert len(protos[name][1]) == nargs, (name, protos[name][1])
        assert hasattr(so, name), f"{name} not exported"
    assert _lib.lib().acvae_abi_version() == 3


def test_optimizer_bad_arguments_are_reported_not_thrown():
    lib = _lib.lib()
    fake = 1 << 20                                  # 16-B aligned, never dereferenced: every check precedes any launch
    # adamw: params, grads, m, v, vmax, n, lr, b1, b2, eps, wd, decoupled, amsgrad, step, gscale, max_norm, norm, stream
    assert lib.acvae_adamw_step(None, None, None, None, None, 0, 1e-3, .9, .999, 1e-8, 0, 1, 0, 1, 1, 1, None, None) == -1
    assert lib.acvae_adamw_step(fake, fake, fake, fake, None, 0, 1e-3, .9, .999, 1e-8, 0, 1, 0, 1, 1, 1, None, None) == -1
    assert lib.acvae_adamw_step(fake, fake, fake, fake, None, 8, 1e-3, .9, .999, 1e-8, 0, 1, 0, 0, 1, 1, None, None) == -1
    assert lib.acvae_adamw_step(fake, fake, fake, fake, None, 8, 1e-3, .9, .999, 1e-8, 0, 1, 1, 1, 1, 1, None, None) == -1
    assert lib.acvae_adamw_step(fake + 4, fake, fake, fake, None, 8, 1e-3, .9, .999, 1e-8, 0, 1, 0, 1, 1, 1, None, None) == -2
    assert lib.acvae_adamw_step(fake, fake, fake, fake, fake + 8, 8, 1e-3, .9, .999, 1e-8, 0, 1, 1, 1, 1, 1, None, None) == -2
    # sgd: params, grads, buf, n, lr, momentum, dampening, wd, nesterov, first, gscale, max_norm, norm, stream
    assert lib.acvae_sgd_step(None, None, None, 0, 1e-3, 0, 0, 0, 0, 0, 1, 1, None, None) == -1
    assert lib.acvae_sgd_step(fake, fake, None, 0, 1e-3, 0, 0, 0, 0, 0, 1, 1, None, None) == -1
    assert lib.acvae_sgd_step(fake, fake, None, 8, 1e-3, 0.9, 0, 0, 0, 0, 1, 1, None, None) == -1   # momentum, no buffer
    assert lib.acvae_sgd_step(fake, fake, fake, 8, 1e-3, 0.0, 0, 0, 1, 0, 1, 1, None, None) == -1   # nesterov, momentum 0
    assert lib.acvae_sgd_step(fake, fake, fake, 8, 1e-3, 0.9, 0.1, 0, 1, 0, 1, 1, None, None) == -1  # nesterov, dampening
    assert lib.acvae_sgd_step(fake, fake + 4, fake, 8, 1e-3, 0.9, 0, 0, 0, 0, 1, 1, None, None) == -2


def test_resolve_reads_torch_defaults_and_applies_options_in_order():
    dummy = [torch.zeros(1, requires_grad=True)]
    for name in ("Adam", "AdamW", "SGD"):
        g = resolve(name)
        ref = dict(getattr(torch.optim, name)(dummy).defaults)
        assert set(g) == set(ref), name
        for k in ref:
            if k != "betas":
                assert g[k] == ref[k], (name, k)
    assert resolve("AdamW")["weight_decay"] == 1e-2
    assert resolve("AdamW", weight_decay=None)["weight_decay"] == 1e-2
    assert resolve("Adam", lr=5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)["lr"] == 5e-4
    g = resolve("AdamW", {"lr": 1e-3, "amsgrad": True}, lr=5e-4, weight_decay=0.1)
    assert g["lr"] == 1e-3 and g["weight_decay"] == 0.1 and g["amsgrad"] and g["decoupled_weight_decay"]
    g = resolve("SGD", {"momentum": 0.9, "nesterov": True}, lr=5e-4)
    assert g["momentum"] == 0.9 and g["nesterov"] and g["dampening"] == 0 and g["lr"] == 5e-4


@pytest.mark.parametrize("name, args, kw, what", [
    ("Nesterov", None, {}, "Nesterov"),
    ("RMSprop", None, {}, "RMSprop"),
    ("SGD", {"nesterov": True, "momentum": 0}, {}, "nesterov"),
    ("SGD", {"nesterov": True, "momentum": 0.9, "dampening": 0.1}, {}, "nesterov"),
    ("Adam", {"maximize": True}, {}, "maximize"),
    ("AdamW", {"differentiable": True}, {}, "differentiable"),
    ("SGD", {"maximize": True, "momentum": 0.9}, {}, "maximize"),
    ("Adam", {"momentum": 0.9}, {}, "momentum"),
    ("SGD", None, {"betas": (0.9, 0.99)}, "betas"),
    ("Adam", {"params": []}, {}, "param group"),
    ("Adam", {"lr": -1.0}, {}, "learning rate"),
])
def test_resolve_refuses_what_the_fused_update_does_not_implement(name, args, kw, what):
    with pytest.raises(ValueError, match=what):
        resolve(name, args, **kw)
