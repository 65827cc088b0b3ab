"""GPU: acvae_augment_window (acvae_amd/csrc/augment.hip) through acvae_amd.augment.apply_plans - against the reference's own
outputs (tests/golden/augment_ref.npz) from the uncropped clips, bit for bit against the existing path (host crop, upload,
acvae_spec_augment) on random plans at the edges, determinism, the C entry point's argument checks - and the Augmented front
end in TrainStep.step and forward_batch against the same calls on features augmented by the existing path."""
import ctypes
import random

import numpy as np
import pytest
import torch

import acvae_oracle as O
import frontend_util as U
from acvae_amd import _lib
from acvae_amd import augment as A
from acvae_amd import batch as B
from acvae_amd import frontend as FE
from test_augment_cpu import check_against_reference, golden_augment, golden_clips, golden_configs, golden_output, restate
from test_augment_gpu import pad, random_records
from test_model_gpu import build_model
from conftest import load_golden

pytestmark = pytest.mark.gpu


def cropped(clip, plan):
    """The host crop: the gather by source_rows() with the final roll undone."""
    return np.roll(clip[plan.source_rows()], -plan.params.shift, axis=0)


def run_plans(x, lens, plans):
    xd = torch.from_numpy(x).cuda()
    out, out_lens = A.apply_plans(xd, lens, plans)
    torch.cuda.synchronize()
    return xd, out, out_lens


def existing_path(x, plans):
    """numpy gather, upload, A.apply with the plans' records -> [N, To, F] (numpy) and the lengths."""
    feats = [cropped(x[n], p) for n, p in enumerate(plans)]
    lens = np.array([len(f) for f in feats])
    out = A.apply(torch.from_numpy(pad(feats, int(lens.max()))).cuda(), lens, [p.params for p in plans])
    torch.cuda.synchronize()
    return out.cpu().numpy(), lens


def test_reference_outputs_from_the_uncropped_clips():
    g = load_golden("augment_ref")
    cl = golden_clips(g)
    F = int(g["F"])
    lens = np.array([len(c) for c in cl])
    x = pad(cl, int(lens.max()) + 3)
    fired = 0
    for k, spec in golden_configs(g):
        seed = int(g[f"c{k}_seed"])
        random.seed(seed); np.random.seed(seed)
        aug = golden_augment(spec)
        plans = [aug.draw_shape(len(c), F) for c in cl]
        _, out, out_lens = run_plans(x, lens, plans)
        out = out.cpu().numpy()
        assert out.shape == (len(cl), int(out_lens.max()), F)
        for n, plan in enumerate(plans):
            L = int(out_lens[n])
            fired += len(plan.windows)
            assert L == plan.params.length
            _, masked = restate(cropped(cl[n], plan), plan.params)
            check_against_reference(out[n, :L], golden_output(g, k, n, cl[n]), masked, f"config {k} {spec} clip {n}")
            assert not out[n, L:].any(), f"config {k} clip {n}: rows behind the clip are not zeros"
    assert fired


def random_plan(rng, L, F, n_windows, sizes, kinds, wrap=False):
    """A plan of ``n_windows`` crops down to ``sizes`` with the shift of each window 0, length - 1 or random by ``kinds``;
    ``wrap``: the first window starts on the clip's last row, so it runs round the clip's end."""
    windows, cur = [], int(L)
    for w in range(n_windows):
        size = int(sizes[w])
        assert 1 <= size <= cur
        shift = [0, cur - 1, int(rng.integers(0, cur))][kinds[w % len(kinds)]]
        if wrap and w == 0 and cur > 1:
            shift, start = max(shift, 1), cur - 1
        elif shift == 0:
            start = int(rng.integers(0, cur - size + 1))
        else:
            start = int(rng.integers(0, cur))
        windows.append((start, shift, cur))
        cur = size
    return A.AugmentPlan(int(L), windows, random_records(rng, [cur], F)[0])


@pytest.mark.parametrize("N, T, F, size", [(9, 40, 4, 7), (7, 130, 12, 50), (64, 300, 64, 100), (5, 3000, 64, 1000)])
def test_random_plans_are_bit_equal_to_the_existing_path_on_the_host_cropped_clip(N, T, F, size):
    rng = np.random.default_rng(N * 7919 + T * 31 + F)
    lens = rng.integers(size + 8, T + 1, size=N)
    lens[0] = T
    plans = []
    for n, L in enumerate(lens):
        nw = [0, 1, A.MAX_WINDOWS][n % 3]
        sizes = [size] if nw == 1 else [size + 6, size + 4, size + 1, size][:nw]
        plans.append(random_plan(rng, L, F, nw, sizes, [[0], [1], [2], [0, 2, 1]][n % 4], wrap=n % 5 == 1))
    plans[0] = A.AugmentPlan(T, [], random_records(rng, [T], F)[0])                           # out_len == T
    plans[1] = random_plan(rng, lens[1], F, 1, [size], [2], wrap=True)                        # round the clip's end
    plans[2] = random_plan(rng, lens[2], F, A.MAX_WINDOWS, [size + 6, size + 4, size + 1, 1], [1, 2, 0])   # one frame out
    L3 = min(size, int(lens[3]))                                                              # 8 + 8 stacked masks
    plans[3] = A.AugmentPlan(int(lens[3]), [(int(lens[3]) - 2, 5, int(lens[3]))],
                             A.AugmentParams(L3, L3 - 1, [(0, L3)] * A.MAX_MASKS, [(0, F)] * A.MAX_MASKS))
    assert {len(p.windows) for p in plans} == {0, 1, A.MAX_WINDOWS}
    assert any(w[0] + s > w[2] for p in plans for w, s in zip(p.windows, [q[2] for q in p.windows[1:]] + [p.params.length]))
    x = (rng.standard_normal((N, T, F)) * 3 - 2).astype(np.float32)
    for n, L in enumerate(lens):
        x[n, L:] = 0
    x[N // 2, int(lens[N // 2]):] = 7.0                                                        # non-zero input padding
    xd, out, out_lens = run_plans(x, lens, plans)
    assert np.array_equal(xd.cpu().numpy().view(np.uint32), x.view(np.uint32)), "apply_plans wrote into its input"
    out = out.cpu().numpy()
    want, want_lens = existing_path(x, plans)
    assert np.array_equal(out_lens, want_lens) and out.shape == want.shape and out.shape[1] == T
    for n, L in enumerate(out_lens):
        assert np.array_equal(out[n, :L].view(np.uint32), want[n, :L].view(np.uint32)), f"clip {n} ({plans[n].windows})"
        assert not out[n, L:].view(np.uint32).any(), f"clip {n}: rows behind the clip are not zeros"


def test_no_windows_equals_spec_augment_and_runs_are_reproducible():
    rng = np.random.default_rng(3)
    N, T, F = 16, 400, 64
    lens = rng.integers(100, T + 1, size=N)
    lens[5] = T
    x = rng.standard_normal((N, T, F)).astype(np.float32)                # the input's padding rows are not zeros
    x[0, 5, 7] = np.float32(-0.0)
    recs = random_records(rng, lens, F, max_masks=3)
    recs[0] = A.AugmentParams(int(lens[0]))
    plans = [A.AugmentPlan(int(L), [], r) for L, r in zip(lens, recs)]
    xd, out, out_lens = run_plans(x, lens, plans)
    assert out.shape == xd.shape and np.array_equal(out_lens, lens)
    want = A.apply(xd, lens, recs)
    keep = xd.clone()
    again, _ = A.apply_plans(xd, lens, plans)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), again.view(torch.int32)), "two runs differ"
    assert torch.equal(xd.view(torch.int32), keep.view(torch.int32)), "apply_plans wrote into its input"
    for n, L in enumerate(lens):
        assert torch.equal(out[n, :L].view(torch.int32), want[n, :L].view(torch.int32)), f"clip {n}"
        assert not bool(out[n, L:].view(torch.int32).any()), f"clip {n}: rows behind the clip are not zeros"

    plans = [random_plan(rng, L, F, 2, [90, 60], [2]) for L in lens]     # and with crops firing
    a, _ = A.apply_plans(xd, lens, plans)
    b, _ = A.apply_plans(xd, lens, plans)
    torch.cuda.synchronize()
    assert a.shape == (N, 60, F) and torch.equal(a.view(torch.int32), b.view(torch.int32)), "two runs differ"
    assert torch.equal(xd.view(torch.int32), keep.view(torch.int32)), "apply_plans wrote into its input"


def test_entry_point_rejects_bad_arguments():
    lib = _lib.lib()
    K = A.WINDOW_TABLE_WIDTH
    x = torch.randn(4, 8, 64, device="cuda")
    y = torch.full((4, 6, 64), 3.0, device="cuda")
    lens = torch.full((4,), 8, dtype=torch.int32, device="cuda")
    tab = torch.zeros(4, K, dtype=torch.int32, device="cuda")
    tab[:2, A.TABLE_WIDTH] = 6
    st = _lib.current_stream()
    p = [t.data_ptr() for t in (x, y, lens, tab)]
    fn = lib.acvae_augment_window
    assert fn(*p, 4, 8, 6, 64, K, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(y[:2], x[:2, :6]) and not bool(y[2:].any())
    bad = [(0, 8, 6, 64, K), (-1, 8, 6, 64, K), (4, 0, 6, 64, K), (4, 8, 0, 64, K), (4, 8, -1, 64, K), (4, 8, 9, 64, K),
           (4, 8, 6, 62, K), (4, 8, 6, 0, K), (4, 8, 6, A.MAX_F + 4, K), (4, 8, 6, 64, K - 1), (4, 8, 6, 64, K + 1),
           (4, 8, 6, 64, A.TABLE_WIDTH), (4, (1 << 31) // 64, 6, 64, K)]
    for args in bad:
        assert fn(*p, *args, st) == -1, args
    for k in range(4):
        q = list(p)
        q[k] = None
        assert fn(*q, 4, 8, 6, 64, K, st) == -1
    assert fn(ctypes.c_void_p(p[0] + 4).value, *p[1:], 4, 8, 6, 64, K, st) == -2             # misaligned
    assert fn(p[0], ctypes.c_void_p(p[1] + 8).value, *p[2:], 4, 8, 6, 64, K, st) == -2
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------- end to end on a tiny model
V, E = 40, 64
SEED = 11


def _model(state):
    from acvae_amd.trainer import TrainStep
    m = build_model(V, E, state).train()
    m.encoder.p_block = m.encoder.p_fc = 0.0
    return m, TrainStep(m, V)


def seed_draws():
    random.seed(SEED); np.random.seed(SEED)


def twin_features(fe, aug, pcm, lens):
    """The existing path on the front end's features: downloaded, Augment.draw clip by clip in batch order, uploaded, apply."""
    feats, fl = fe(pcm, lens)
    host = feats.cpu().numpy()
    drawn = [aug.draw(host[n, :int(L)]) for n, L in enumerate(fl)]
    tl = np.array([len(f) for f, _ in drawn])
    x = torch.from_numpy(pad([f for f, _ in drawn], int(tl.max()))).cuda()
    return A.apply(x, tl, [r for _, r in drawn]), tl, fl


@pytest.mark.parametrize("rate", [32000, 44100])
def test_train_step_and_forward_batch_with_an_augmented_front_end(rate):
    fe = FE.LogMel.panns_32k().at_input_rate(rate)
    aug = A.Augment([A.Augment.roll(0, 10), A.Augment.crop(20, 1.0)], p=1.0, T=12, F=15)
    afe = fe.augmented(aug)
    lens = np.array([int(0.6 * rate), int(0.45 * rate) + 7, int(0.3 * rate) + 1])
    waves = torch.zeros(3, int(lens.max()))
    for n, L in enumerate(lens):
        waves[n, :L] = torch.from_numpy(U.clip(int(L), rate, 70 + n))
    pcm = torch.from_numpy(np.rint(waves.numpy() * 32768.0).clip(-32768, 32767).astype(np.int16))
    state = O.closed_form_state(O.state_shapes(V, E, E, None, E, 512))
    _, caps, _, cl = O.synthetic_batch(3, 64, V, 7, seed=1, ragged=True)

    seed_draws()
    got, gl = afe(pcm, lens)
    plans = afe.last_plans
    assert len(plans) == 3 and all(len(p.windows) == 1 for p in plans), "every crop fires"
    assert any(p.windows[0][1] for p in plans) and any(p.params.time_masks for p in plans) \
        and any(p.params.freq_masks for p in plans)
    seed_draws()
    twin, tl, fl = twin_features(fe, aug, pcm, lens)
    assert [p.src_length for p in plans] == list(fl) and list(gl) == list(tl) == [20, 20, 20]
    assert torch.equal(got.view(torch.int32), twin.view(torch.int32)), "the features out of the augmented front end differ"

    (m1, t1), (m2, t2) = _model(state), _model(state)
    seed_draws(); torch.manual_seed(3)
    p1 = t1.step(pcm.clone(), lens.copy(), caps, cl, 1.0, 0, 0.5, frontend=afe)
    assert afe.last_plans == plans
    seed_draws(); torch.manual_seed(3)
    twin, tl, _ = twin_features(fe, aug, pcm, lens)
    p2 = t2.step(twin, tl.copy(), caps, cl, 1.0, 0, 0.5)
    t1.synchronize(); t2.synchronize()
    for key in ("loss", "grad_norm"):
        a, b = float(p1[key]), float(p2[key])
        print(f"rate {rate} {key}: {a!r} vs {b!r}")
        assert abs(a - b) <= 1e-6 * abs(b), f"{key}: {a} vs {b}"

    keys = [f"a{n}" for n in range(3)]
    seed_draws(); torch.manual_seed(5)
    batch = [pcm.clone(), caps, keys, lens.copy(), cl]
    a = B.forward_batch(m1, batch, "train", frontend=afe, ss_ratio=1.0, dis_ratio=0)["packed_logits"].detach().cpu()
    assert tuple(batch[0].shape) == (3, 20, 64) and len(batch[-2]) == 3, "batch slots not replaced"
    seed_draws(); torch.manual_seed(5)
    twin, tl, _ = twin_features(fe, aug, pcm, lens)
    b = B.forward_batch(m1, [twin, caps, keys, tl.copy(), cl], "train", ss_ratio=1.0, dis_ratio=0)["packed_logits"].detach().cpu()
    torch.testing.assert_close(a, b, rtol=1e-6, atol=1e-6)
