"""No GPU: what TrainStep(accum_steps=, ema_decay=, ema_warmup=) refuses, before anything is built and before any library
call; ema_warmup's decay schedule; the two new entry points in the header and in the built library."""
import ctypes
import re

import numpy as np
import pytest

from acvae_amd import _lib, trainer


@pytest.fixture
def no_library(monkeypatch):
    """Any use of the library (or of the model, which is None) is a failure of the test, not a ValueError."""
    def used(*a, **k):
        raise AssertionError("the library was reached before the arguments were refused")
    monkeypatch.setattr(_lib, "lib", used)
    monkeypatch.setattr(_lib, "call", used)
    monkeypatch.setattr(_lib, "require_cuda", used)


@pytest.mark.parametrize("kw, match", [
    (dict(accum_steps=0), "accum_steps"),
    (dict(accum_steps=-2), "accum_steps"),
    (dict(accum_steps=2.0), "accum_steps"),
    (dict(accum_steps=1.5), "accum_steps"),
    (dict(accum_steps="2"), "accum_steps"),
    (dict(accum_steps=True), "accum_steps"),
    (dict(accum_steps=None), "accum_steps"),
    (dict(ema_decay=1.0), "ema_decay"),
    (dict(ema_decay=1.5), "ema_decay"),
    (dict(ema_decay=-0.1), "ema_decay"),
    (dict(ema_decay=float("nan")), "ema_decay"),
    (dict(ema_warmup=True), "ema_warmup"),
    (dict(accum_steps=4, ema_warmup=True), "ema_warmup"),
])
def test_constructor_refuses_before_anything_is_built(no_library, kw, match):
    with pytest.raises(ValueError, match=match):
        trainer.TrainStep(None, 40, **kw)


def test_accepted_values_pass_the_check():
    for kw in (dict(accum_steps=1, ema_decay=None, ema_warmup=False), dict(accum_steps=np.int64(3), ema_decay=0.0, ema_warmup=True),
               dict(accum_steps=128, ema_decay=0.9999, ema_warmup=False)):
        trainer.check_accumulation(**kw)


def test_ema_warmup_decay_follows_the_formula():
    d = 0.999
    for t in (0, 1, 9, 10_000):
        want = min(d, (1 + t) / (10 + t))
        assert trainer.ema_decay_at(d, t, warmup=True) == want
        assert trainer.ema_decay_at(d, t, warmup=False) == d
    assert trainer.ema_decay_at(d, 0, True) == 0.1 and trainer.ema_decay_at(d, 1, True) == 2 / 11
    assert trainer.ema_decay_at(d, 9, True) == 10 / 19
    assert trainer.ema_decay_at(d, 10_000, True) == d            # 10001 / 10010 = 0.99910...: the cap holds
    assert trainer.ema_decay_at(0.5, 9, True) == 0.5             # 10 / 19 > 0.5


def test_header_declares_and_library_exports_both_symbols():
    P = ctypes.c_void_p
    want = {"acvae_grad_accumulate": [("acc", P), ("grads", P), ("n", ctypes.c_int64), ("first", ctypes.c_int), ("stream", P)],
            "acvae_ema_step": [("ema", P), ("params", P), ("n", ctypes.c_int64), ("decay", ctypes.c_double), ("stream", P)]}
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name, args in want.items():
        assert name in _lib.PROTOS, name
        ret, got = _lib.PROTOS[name]
        assert ret is ctypes.c_int and got == args, (name, got)
        assert hasattr(so, name), f"{name} is declared but not exported"
    src = open(_lib.HEADER).read()
    assert int(re.search(r"#define\s+ACVAE_ABI_VERSION\s+(\d+)", src).group(1)) == 3
    assert int(re.search(r"#define\s+ACVAE_FLAT_BLOCKS_CAP\s+(\d+)", src).group(1)) >= 1
