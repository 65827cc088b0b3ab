"""GPU: CIDEr-D on the device (acvae_ciderd_scores / acvae_ciderd_reward, acvae_amd/cider.py) and the SCST step that uses it.

The kernel alone against the dictionary yardstick of tests/cider_util.py on the words read back, bound
1e-12 * max(1, |score|) (derived, cider_util.bound: the two differ only in the order of sums of at most 64 non-negative
float64 terms and a handful of correctly rounded operations per order); planted rows; V = 50 / 5000, max_length 20 / 30,
N = 1 / 2 / 7 / 32, sample_n 2 / 5; two launches bit-identical.  Worst difference observed on an MI355X over every case
of this file: 1.78e-15 absolute on a score of 5.1, 3.5e-4 of the bound (most scores come out bit-identical: the kernel adds
a row's terms in the order in which the dictionary scorer walks its n-grams; the references' norms are summed in another
order on the host).

End to end: TrainStep.scst_step(..., scorer=CiderD(vocab)) against a twin built from the same seed that takes the host
route with the yardstick as its scorer - same words, float64 scores within the bound, f32 rewards within one unit in the
last place (exactly 0 where the sampled and the greedy words coincide), and the loss and the updated parameters bit-equal
where every f32 reward is (compare_params of tests/test_optim_gpu.py otherwise).  During the device step
train_util._seqs_to_host and the tensor read-backs (.cpu(), .item(), .tolist()) of device tensors raise."""
import random

import numpy as np
import pytest
import torch

import acvae_oracle as O
import cider_util as CU
from acvae_amd import train_util
from cider_util import SPECIALS, DictCiderD, Vocabulary
from scst_util import text_side
from test_cider_cpu import random_rows, random_text

pytestmark = pytest.mark.gpu
START, END = 1, 2


def device_tables(vocab, keys, key2refs, mode):
    from acvae_amd.cider import CiderD
    return CiderD(vocab).prepare(keys, key2refs, mode, device="cuda")


def check_scores(tag, vocab, keys, key2refs, mode, *sets):
    """Device scores of the token-row sets against the yardstick on the same words; a second launch bit-identical."""
    tab = device_tables(vocab, keys, key2refs, mode)
    dev = [torch.as_tensor(s).cuda() for s in sets]
    got = tab.scores(*dev)
    again = tab.scores(*dev)
    torch.cuda.synchronize()
    assert torch.equal(got, again), tag
    got = got.cpu().numpy()
    want = np.concatenate([CU.row_scores(s, keys, key2refs, vocab, mode) for s in sets])
    err = np.abs(got - want)
    print(f"{tag}: {len(want)} scores {want.min():.4f} .. {want.max():.4f} ({int((want > 0).sum())} non-zero), worst |d| "
          f"{float(err.max()):.3g} = {float((err / CU.bound(want)).max()):.3g} of the bound; upload {tab.nbytes} B")
    assert np.all(err <= CU.bound(want)), (tag, got, want)
    return tab, dev, got, want


def ulp32(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)


# ---------------------------------------------------------------- the kernel alone
@pytest.mark.parametrize("N", [1, 2, 7, 32])
@pytest.mark.parametrize("T", [20, 30])
@pytest.mark.parametrize("V", [50, 5000])
def test_scores_and_rewards_against_the_yardstick(V, T, N):
    vocab, keys, key2refs = random_text(V, N, seed=N + T, oov=True)
    # "batch": sampled and greedy rows in one launch; the last key twice when there is room (scored by its first row)
    bkeys = keys + keys[-1:] if N > 1 else keys
    sampled = random_rows(V, len(bkeys), T, N, key2refs, bkeys, vocab)
    greedy = random_rows(V, len(bkeys), T, N + 7)
    greedy[::3] = sampled[::3]                                   # some rows whose sampled and greedy words coincide
    tab, dev, got, want = check_scores(f"batch V{V} T{T} N{N}", vocab, bkeys, key2refs, "batch", sampled, greedy)
    n = len(bkeys)
    rs = tab.reward(dev[0], dev[1], 1)
    torch.cuda.synchronize()
    reward, score = rs["reward"].cpu().numpy(), rs["score"].cpu().numpy()
    assert reward.dtype == np.float32 and np.array_equal(score, got[:n])
    assert np.array_equal(reward, (got[:n] - got[n:]).astype(np.float32))          # from the device's own scores: exact
    assert np.all(ulp32(reward, (want[:n] - want[n:]).astype(np.float32))) and not reward[::3].any()
    assert float(rs["reward_mean"].cpu()) == pytest.approx(float((got[:n] - got[n:]).mean()), abs=1e-12)
    for sample_n in (2, 5):
        rkeys = [k for k in keys for _ in range(sample_n)]
        rows = random_rows(V, len(rkeys), T, N + sample_n, key2refs, rkeys, vocab)
        tab, dev, got, want = check_scores(f"rows V{V} T{T} N{N} x{sample_n}", vocab, rkeys, key2refs, "rows", rows)
        rs = tab.reward(dev[0], None, sample_n)
        torch.cuda.synchronize()
        reward = rs["reward"].cpu().numpy()
        assert np.array_equal(reward, train_util.leave_one_out_reward(got, sample_n).astype(np.float32))
        assert np.all(ulp32(reward, train_util.leave_one_out_reward(want, sample_n).astype(np.float32)))
        assert float(rs["reward_mean"].cpu()) == pytest.approx(0.0, abs=1e-12)   # leave-one-out rewards of a clip sum to 0


def test_planted_rows():
    words = SPECIALS + ("a dog barks at the cat in rain falls on tin roof while birds sing loudly far away wind blows "
                        "through tall trees near river").split()
    words += [f"w{i}" for i in range(len(words), 50)]
    vocab = Vocabulary(words)
    w = {x: i for i, x in enumerate(words)}
    T = 20

    def row(text, end=True, fill=0):
        ids = [w[x] for x in text.split()] + ([END] if end else [])
        return ids + [fill] * (T - len(ids))
    key2refs = {"only": ["a dog barks at the cat"],
                "several": ["rain falls on the tin roof", "birds sing loudly far away", "wind blows through tall trees"],
                "short": ["a dog barks", "the cat", "rain falls"],
                "long": ["wind blows through tall trees near the river while birds sing loudly far away in the rain",
                         "a dog barks at the cat on the tin roof while rain falls on tall trees near the river far away"],
                "misc": ["the <unk> barks at <pad> cat", "a dog zebra at the okapi"]}
    plan = [("only", row("a dog barks at the cat")),                      # identical to the document's only reference: 10
            ("several", row("birds sing loudly far away")),              # identical to one of several
            ("short", row("a dog barks at the cat in the rain on the tin roof")),        # longer than every reference
            ("long", row("wind blows")),                                  # shorter than every reference
            ("misc", [END] + [w["dog"]] * (T - 1)),                       # <end> at step 0: the empty hypothesis
            ("misc", row("dog")),                                         # a single word
            ("misc", row("a dog barks at the cat in rain falls on tin roof while birds sing loudly far away wind", end=False)),
            ("misc", [w["a"], START, w["dog"], START, START, w["barks"], END] + [w["cat"]] * (T - 7)),   # <start> in mid-row
            ("misc", [w["the"]] * T),                                     # one repeated word, no <end>
            ("misc", row("the <unk> barks at <pad> cat")),                # <unk> and <pad> ids are words
            ("misc", [0, 3, 3, 0, END] + [0] * (T - 5))]
    keys = [k for k, _ in plan]
    seqs = np.array([r for _, r in plan])
    assert seqs.shape == (len(plan), T)
    tab, dev, got, want = check_scores("planted rows", vocab, keys, key2refs, "rows", seqs)
    print("planted rows:", np.round(got, 4).tolist())
    assert abs(got[0] - 10.0) <= CU.bound(10.0) and 0 < got[1] < 10 and got[4] == 0.0
    assert 0 < got[2] < want.max() and 0 < got[3] and got[9] > got[10] > 0
    # "batch" over the same rows: the documents are the 5 distinct keys, a row is scored by the first row with its key
    tab, dev, got, want = check_scores("planted batch", vocab, keys, key2refs, "batch", seqs, seqs[::-1].copy())
    n = len(keys)
    assert np.array_equal(got[5:n], np.full(n - 5, got[4])) and abs(got[0] - 10.0) <= CU.bound(10.0)
    assert np.array_equal(got[n + 5:], np.full(n - 5, got[n + 4]))
    # one document: ln D = 0, every score 0
    tab, dev, got, want = check_scores("one document", vocab, ["only"], key2refs, "batch", seqs[:1])
    assert got.tolist() == [0.0]


def test_wrong_shapes_and_host_only_tables_are_refused():
    from acvae_amd.cider import CiderD
    vocab, keys, key2refs = random_text(50, 3, seed=1)
    cd = CiderD(vocab)
    tab = cd.prepare(keys, key2refs, "batch", device="cuda")
    seqs = torch.zeros(3, 20, dtype=torch.long, device="cuda")
    with pytest.raises(ValueError, match="prepared for 3 rows"):
        tab.scores(seqs[:2])
    with pytest.raises(ValueError, match="at most 64"):
        tab.scores(torch.zeros(3, 65, dtype=torch.long, device="cuda"))
    with pytest.raises(ValueError, match="baseline"):
        tab.reward(seqs, None, 1)
    with pytest.raises(RuntimeError, match="host only"):
        cd.prepare(keys, key2refs, "batch").scores(seqs)
    with pytest.raises(RuntimeError, match="no CPU fallback|MI355X"):
        tab.scores(seqs.cpu())
    assert tab.scores(seqs.to(torch.int32)[:, ::1]).shape == (3,)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- end to end: the device route against the host route
class _NoReadBack:
    """While active, reading a device tensor back (.cpu(), .item(), .tolist()) and train_util._seqs_to_host raise."""

    def __init__(self, monkeypatch):
        self.mp = monkeypatch

    def __enter__(self):
        def refuse(*a, **k):
            raise AssertionError("the device route read the words back (_seqs_to_host)")
        self.mp.setattr(train_util, "_seqs_to_host", refuse)
        for name in ("cpu", "item", "tolist"):
            orig = getattr(torch.Tensor, name)

            def guard(self, *a, _orig=orig, _name=name, **k):
                if self.is_cuda:
                    raise AssertionError(f"the device route called .{_name}() on a device tensor")
                return _orig(self, *a, **k)
            self.mp.setattr(torch.Tensor, name, guard)
        return self

    def __exit__(self, *exc):
        self.mp.undo()
        return False


def twin_steps(tag, monkeypatch, make, feats, fl, keys, key2refs, vocab, sample_n, max_length, steps, **kw):
    from acvae_amd.cider import CiderD
    from test_optim_gpu import compare_params, sync_params
    (m1, t1), (m2, t2) = make(), make()
    cd, host = CiderD(vocab), DictCiderD()
    f = feats.cuda()
    exact_steps = 0
    for k in range(steps):
        if k:
            sync_params(m1, m2)
        torch.manual_seed(11 + k); random.seed(11 + k)
        with _NoReadBack(monkeypatch):
            p1 = t1.scst_step(f, np.asarray(fl).copy(), keys, key2refs, vocab, cd, sample_n=sample_n, max_length=max_length, **kw)
        torch.manual_seed(11 + k); random.seed(11 + k)
        p2 = t2.scst_step(f, np.asarray(fl).copy(), keys, key2refs, vocab, host, sample_n=sample_n, max_length=max_length, **kw)
        t1.synchronize(); t2.synchronize()
        assert p1["reward"].is_cuda and p1["score"].is_cuda and p1["reward"].dtype == torch.float32
        assert p1["score"].dtype == torch.float64 and not p2["reward"].is_cuda
        assert torch.equal(p1["sampled_seqs"], p2["sampled_seqs"]), tag
        if sample_n == 1:
            assert torch.equal(p1["greedy_seqs"], p2["greedy_seqs"]), tag
        s1, s2 = p1["score"].cpu().numpy(), p2["score"].numpy()
        r1, r2 = p1["reward"].cpu().numpy(), p2["reward"].numpy().astype(np.float32)
        err = np.abs(s1 - s2)
        same = int((r1 == r2).sum())
        print(f"{tag} step {k + 1}: scores {s2.min():.4f} .. {s2.max():.4f} ({int((s2 > 0).sum())}/{len(s2)} non-zero), worst |d| "
              f"{float(err.max()):.3g} = {float((err / CU.bound(s2)).max()):.3g} of the bound; rewards {r2.min():.4f} .. "
              f"{r2.max():.4f}, {same}/{len(r2)} bit-equal in f32; loss device route {float(p1['loss']):.8f} host route "
              f"{float(p2['loss']):.8f}")
        assert s1.shape == s2.shape and np.all(err <= CU.bound(s2)), tag
        assert r1.shape == r2.shape and np.all(ulp32(r1, r2)), (tag, r1, r2)
        assert float(np.abs(r2).max()) > 0, "a step without reward checks nothing"
        if sample_n == 1:
            coincide = (p1["sampled_seqs"] == p1["greedy_seqs"]).all(1).cpu().numpy()
            assert not r1[coincide].any() and not r2[coincide].any()
        if same == len(r2):
            exact_steps += 1
            assert torch.equal(p1["loss"], p2["loss"]), tag
            for (name, a), (_, b) in zip(m1.named_parameters(), m2.named_parameters()):
                assert torch.equal(a, b), (tag, name)
        else:
            compare_params(m1, m2, f"{tag} step {k + 1}")
    print(f"{tag}: {exact_steps}/{steps} steps with every f32 reward, the loss and every parameter bit-equal")


def _bias_towards(state_or_model, ids, bump, end_bump):
    """Raise the classifier's bias for a small pool of words (and <end>): the rollouts of an untrained model then share
    n-grams with references drawn from that pool, and some rows finish early."""
    b = state_or_model["decoder.classifier.bias"] if isinstance(state_or_model, dict) else state_or_model.decoder.classifier.bias
    with torch.no_grad():
        b[ids] += bump
        b[END] += end_bump


def _pool_text(V, B, seed, pool, nrefs=5):
    """text_side's vocabulary and keys, with references of 8-16 words drawn from the word ids `pool`."""
    vocab, keys, _ = text_side(V, B, seed)
    rng = np.random.default_rng(seed)
    key2refs = {k: [" ".join(vocab.idx2word[int(i)] for i in rng.choice(pool, rng.integers(8, 17))) for _ in range(nrefs)]
                for k in keys}
    return vocab, keys, key2refs


@pytest.mark.parametrize("sample_n", [1, 5])
def test_scst_step_device_route_against_host_route_small(monkeypatch, sample_n):
    from test_optim_gpu import E, V, _state, fresh
    pool = np.arange(4, 12)

    def make():
        state = _state()
        _bias_towards(state, pool, 2.0, 1.0)
        return fresh(state=state)
    feats, _, fl, _ = O.synthetic_batch(3, 64, V, 7, seed=1, ragged=True)
    vocab, keys, key2refs = _pool_text(V, 3, 1, pool, nrefs=3)
    twin_steps(f"small n{sample_n}", monkeypatch, make, feats, fl, keys, key2refs, vocab, sample_n, 10, steps=3)


@pytest.mark.parametrize("B,sample_n", [(32, 1), (8, 5)])
def test_scst_step_device_route_against_host_route_full_size(monkeypatch, B, sample_n):
    """configs[1]: B = 32, T = 1000, V = 5000, E = 512, max_length 20; and B = 8 with sample_n = 5."""
    from acvae_amd.trainer import TrainStep
    from test_fullsize_gpu import V, batch, build
    pool = np.arange(4, 44)

    def make():
        m = build(5).train()
        _bias_towards(m, torch.as_tensor(pool, device="cuda"), 8.0, 8.5)
        return m, TrainStep(m, V)
    feats, _, fl, _ = batch(B, 1000, ragged=True)
    vocab, keys, key2refs = _pool_text(V, B, 9, pool)
    twin_steps(f"full size B{B} n{sample_n}", monkeypatch, make, feats, fl, keys, key2refs, vocab, sample_n, 20, steps=2,
               rng="device")
