"""GPU: acvae_spec_augment (acvae_amd/csrc/augment.hip) through acvae_amd.augment.apply - against the reference's own
outputs (tests/golden/augment_ref.npz) on a padded batch, against the fp64 numpy restatement on random tables at the
edges (8 + 8 overlapping masks, full-width frequency masks, extreme shifts, one-frame clips, N up to 64, T up to 3000),
identity and determinism, host validation and the C entry point's argument checks, and TrainStep.step(augment=...)
against the same step on the host-augmented batch."""
import ctypes
import random

import numpy as np
import pytest
import torch

import acvae_oracle as O
from acvae_amd import _lib
from acvae_amd import augment as A
from acvae_amd import batch as B
from test_augment_cpu import (check_against_reference, draw_golden, golden_clips, golden_configs, golden_output,
                              restate)
from test_model_gpu import build_model
from conftest import load_golden

pytestmark = pytest.mark.gpu
EPS32 = float(np.finfo(np.float32).eps)


def pad(feats, T):
    x = np.zeros((len(feats), T, feats[0].shape[1]), np.float32)
    for n, f in enumerate(feats):
        x[n, :len(f)] = f
    return x


def run(x, lens, params):
    xd = torch.from_numpy(x).cuda()
    out = A.apply(xd, lens, params)
    torch.cuda.synchronize()
    return xd, out


def test_reference_outputs_on_a_padded_batch():
    g = load_golden("augment_ref")
    cl = golden_clips(g)
    for k, spec in golden_configs(g):
        drawn, _, _ = draw_golden(g, k, spec, cl)
        feats = [f for f, _ in drawn]
        params = [r for _, r in drawn]
        lens = np.array([len(f) for f in feats])
        T = int(lens.max()) + 3
        x = pad(feats, T)
        _, out = run(x, lens, params)
        out = out.cpu().numpy()
        for n, (f, rec) in enumerate(drawn):
            L = len(f)
            _, masked = restate(f, rec)
            check_against_reference(out[n, :L], golden_output(g, k, n, cl[n]), masked, f"config {k} {spec} clip {n}")
            assert np.array_equal(out[n, L:], x[n, L:]), f"config {k} clip {n}: padding rows changed"


def random_records(rng, lens, F, max_masks=A.MAX_MASKS):
    recs = []
    for n, L in enumerate(lens):
        L = int(L)
        shift = [0, L - 1, int(rng.integers(0, L))][n % 3]
        tm, fm = [], []
        for _ in range(int(rng.integers(0, max_masks + 1))):
            a = int(rng.integers(0, L))
            tm.append((a, int(rng.integers(a + 1, min(L, a + 1 + max(1, L // 3)) + 1))))
        for j in range(int(rng.integers(0, max_masks + 1))):
            if j == 0 and n % 4 == 1:
                fm.append((0, F))                                        # a full-width frequency mask
            else:
                a = int(rng.integers(0, F))
                fm.append((a, int(rng.integers(a + 1, F + 1))))
        recs.append(A.AugmentParams(L, shift, tm, fm))
    return recs


@pytest.mark.parametrize("N, T, F", [(64, 300, 64), (5, 3000, 64), (9, 40, 4), (7, 130, 12)])
def test_random_tables_against_the_fp64_restatement(N, T, F):
    rng = np.random.default_rng(N * 7919 + T * 31 + F)
    lens = rng.integers(1, T + 1, size=N)
    lens[0], lens[-1] = T, 1                                             # a full clip and a one-frame clip
    if N > 2:
        lens[1] = 2
    recs = random_records(rng, lens, F)
    i = N - 1 if N % 2 else 0                                            # 8 + 8 masks on top of each other
    recs[i] = A.AugmentParams(int(lens[i]), 0, [(0, int(lens[i]))] * A.MAX_MASKS, [(0, F)] * A.MAX_MASKS)
    x = (rng.standard_normal((N, T, F)) * 3 - 2).astype(np.float32)
    for n, L in enumerate(lens):
        x[n, L:] = 0
    x[N // 2, int(lens[N // 2]):] = 7.0                                  # non-zero padding is copied as it is
    _, out = run(x, lens, recs)
    out = out.cpu().numpy()
    for n, (L, rec) in enumerate(zip(lens, recs)):
        want, masked = restate(x[n, :L], rec)
        got = out[n, :L]
        assert np.array_equal(got[~masked], want[~masked]), f"clip {n}: cells outside the masks differ"
        rms = float(np.sqrt((x[n, :L].astype(np.float64) ** 2).mean()))
        err = np.abs(got[masked].astype(np.float64) - want[masked])
        tol = 4 * EPS32 * (np.abs(want[masked]) + rms)
        assert bool((err <= tol).all()), f"clip {n}: fill error {float(err.max()):.3e}"
        assert np.array_equal(out[n, L:], x[n, L:]), f"clip {n}: padding rows changed"


def test_identity_is_a_bitwise_copy_and_runs_are_reproducible():
    rng = np.random.default_rng(3)
    N, T, F = 32, 1000, 64
    lens = rng.integers(400, T + 1, size=N)
    x = rng.standard_normal((N, T, F)).astype(np.float32)
    x[0, 5, 7] = np.float32(-0.0)
    x[1, 2, 3] = np.float32(np.nan)
    xd, out = run(x, lens, [A.AugmentParams(int(L)) for L in lens])
    assert out.data_ptr() != xd.data_ptr()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), x.view(np.uint32))

    recs = random_records(rng, lens, F, max_masks=2)
    xd = torch.from_numpy(x).cuda()
    xd[1, 2, 3] = 0.0
    keep = xd.clone()
    a = A.apply(xd, lens, recs)
    b = A.apply(xd, lens, recs)
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "two runs differ"
    assert torch.equal(xd.view(torch.int32), keep.view(torch.int32)), "apply wrote into its input"


def test_malformed_tables_raise_before_any_launch():
    x = torch.zeros(2, 10, 64, device="cuda")
    good = [A.AugmentParams(10), A.AugmentParams(8)]
    A.apply(x, [10, 8], good)
    for params, lens in [
        (good, [10, 9]),                                                     # record / length mismatch
        (good[:1], [10, 8]),
        ([A.AugmentParams(10, shift=-1), good[1]], [10, 8]),
        ([A.AugmentParams(10, time_masks=[(3, 11)]), good[1]], [10, 8]),
        ([A.AugmentParams(10, freq_masks=[(0, 65)]), good[1]], [10, 8]),
        ([A.AugmentParams(10, freq_masks=[(1, 2)] * 9), good[1]], [10, 8]),
        ([A.AugmentParams(11), A.AugmentParams(8)], [11, 8]),                  # longer than T
    ]:
        with pytest.raises(ValueError):
            A.apply(x, lens, params)
    with pytest.raises(ValueError):
        A.apply(torch.zeros(2, 10, 6, device="cuda"), [10, 8], good)         # F % 4
    with pytest.raises(ValueError):
        A.apply(torch.zeros(2, 10, A.MAX_F + 4, device="cuda"), [10, 8], good)
    with pytest.raises(ValueError):
        A.apply(torch.zeros(2, 10, 64, device="cuda", dtype=torch.float64), [10, 8], good)


def test_entry_point_rejects_bad_scalars():
    lib = _lib.lib()
    x = torch.zeros(4, 8, 64, device="cuda")
    y = torch.empty_like(x)
    lens = torch.full((4,), 8, dtype=torch.int32, device="cuda")
    tab = torch.zeros(4, A.TABLE_WIDTH, dtype=torch.int32, device="cuda")
    st = _lib.current_stream()
    p = [t.data_ptr() for t in (x, y, lens, tab)]
    fn = lib.acvae_spec_augment
    assert fn(*p, 4, 8, 64, A.TABLE_WIDTH, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(x, y)
    bad = [(0, 8, 64, A.TABLE_WIDTH), (-1, 8, 64, A.TABLE_WIDTH), (4, 0, 64, A.TABLE_WIDTH), (4, 8, 62, A.TABLE_WIDTH),
           (4, 8, 0, A.TABLE_WIDTH), (4, 8, 64, A.TABLE_WIDTH - 1), (4, 8, 64, A.TABLE_WIDTH + 1),
           (4, 8, A.MAX_F + 4, A.TABLE_WIDTH)]
    for args in bad:
        assert fn(*p, *args, st) == -1, args
    for k in range(4):
        q = list(p)
        q[k] = None
        assert fn(*q, 4, 8, 64, A.TABLE_WIDTH, st) == -1
    assert fn(ctypes.c_void_p(p[0] + 4).value, *p[1:], 4, 8, 64, A.TABLE_WIDTH, st) == -2       # misaligned


V, E = 40, 64


def _model(state):
    from acvae_amd.trainer import TrainStep
    m = build_model(V, E, state).train()
    m.encoder.p_block = m.encoder.p_fc = 0.0
    return m, TrainStep(m, V)


def test_train_step_with_device_augment_matches_the_host_augmented_batch():
    state = O.closed_form_state(O.state_shapes(V, E, E, None, E, 512))
    feats, caps, fl, cl = O.synthetic_batch(3, 64, V, 7, seed=1, ragged=True)
    aug = A.Augment([A.Augment.roll(0, 10)], p=1.0, T=12, F=15)
    random.seed(11); np.random.seed(11)
    params = [aug.draw(feats[n, :int(L)].numpy())[1] for n, L in enumerate(fl)]
    assert any(r.time_masks for r in params) and any(r.freq_masks for r in params) and any(r.shift for r in params)
    host = feats.clone()
    for n, (L, rec) in enumerate(zip(fl, params)):
        host[n, :int(L)] = torch.from_numpy(restate(feats[n, :int(L)].numpy(), rec)[0])
    assert not torch.equal(host, feats)

    m1, t1 = _model(state)
    m2, t2 = _model(state)
    fd = feats.cuda()
    torch.manual_seed(3); random.seed(3)
    p1 = t1.step(fd, fl.copy(), caps, cl, 1.0, 0, 0.5, augment=params)
    torch.manual_seed(3); random.seed(3)
    p2 = t2.step(host.cuda(), fl.copy(), caps, cl, 1.0, 0, 0.5)
    t1.synchronize(); t2.synchronize()
    assert torch.equal(fd.cpu(), feats), "step(augment=...) wrote into the caller's batch"
    for key in ("loss", "grad_norm"):
        a, b = float(p1[key]), float(p2[key])
        assert abs(a - b) <= 1e-6 * abs(b), f"{key}: {a} vs {b}"

    # forward_batch: the batch's own AugmentParams column (CaptionDataset(..., augment=...)) is applied the same way
    keys = [f"a{n}" for n in range(3)]
    outs = []
    for batch, kw in (([feats, caps, keys, tuple(params), fl.copy(), cl], {}), ([host, caps, keys, fl.copy(), cl], {}),
                      ([feats, caps, keys, fl.copy(), cl], {"augment": params})):
        torch.manual_seed(5); random.seed(5)
        outs.append(B.forward_batch(m1, batch, "train", ss_ratio=1.0, dis_ratio=0, **kw)["packed_logits"].detach().cpu())
    torch.testing.assert_close(outs[0], outs[1], rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(outs[2], outs[1], rtol=1e-6, atol=1e-6)
