"""GPU: consensus reranking on the device (acvae_consensus_scores, acvae_amd/consensus.py) and the ``rerank=`` keyword.

The kernel through the C ABI against the dictionary yardstick of tests/consensus_util.py on the same words, every score
within cider_util.bound (1e-12 * max(1, |score|)); sample_n 2 / 3 / 5 / 16, B 1 / 3, T 1 / 2 / 4 / 20 / 64; planted rows;
an empty table, a table of one entry, one of about 5000 entries that holds part of the rows' n-grams, and the table of a
one-document corpus (log_d = 0: every score 0).  Per launch: ``best`` is the first maximum of the device's own scores,
the yardstick's score of the picked candidate is within 2 bounds of the yardstick's maximum, ``picked`` is the row at
``best``, and a second launch is bit-equal.

Then the model: N = 5 rollouts per clip of a small model, "sample" on the device generator and "greedy", with and without
top_p / no_repeat_ngram_size; the output dict, the evaluate() payload and the refusals."""
import numpy as np
import pytest
import torch

import acvae_oracle as O
import cider_util as CU
import consensus_util as MU
from acvae_amd import _lib
from acvae_amd import evaluate as EV
from cider_util import SPECIALS, Vocabulary
from test_consensus_cpu import einval_cases, pack
from test_model_gpu import build_model

pytestmark = pytest.mark.gpu
START, END = 1, 2
V = 50
VOCAB = Vocabulary(SPECIALS + [f"w{i}" for i in range(4, V)])
LEN_FACTOR = np.exp(-(np.arange(64, dtype=np.float64) ** 2) / 72.0)


def launch(seqs, sample_n, keys, vals, log_d, pick=True):
    """acvae_consensus_scores on token rows [B * sample_n, T] -> (scores [B, sample_n], best [B], picked [B, T]) as tensors."""
    seqs = torch.as_tensor(np.ascontiguousarray(seqs), dtype=torch.long).cuda()
    n, T = seqs.shape
    B = n // sample_n
    dk = torch.from_numpy(np.ascontiguousarray(keys, dtype=np.uint64).view(np.int64)).cuda() if len(keys) else None
    dv = torch.from_numpy(np.ascontiguousarray(vals, dtype=np.float64)).cuda() if len(keys) else None
    lf = torch.from_numpy(LEN_FACTOR).cuda()
    score = torch.full((B, sample_n), -7.0, dtype=torch.float64, device="cuda")
    best = torch.full((B,), -7, dtype=torch.long, device="cuda")
    picked = torch.full((B, T), -7, dtype=torch.long, device="cuda") if pick else None
    _lib.call("acvae_consensus_scores", seqs, T, n, sample_n, T, START, END, dk, dv, len(keys), float(log_d), lf, 64, score,
              best, picked, _lib.current_stream())
    return score, best, picked


def ngrams_of(seqs):
    """The distinct n-grams (tuples of ids) of the cleaned rows, in a fixed order."""
    out = {}
    for row in np.asarray(seqs):
        ids = []
        for w in row:
            if w == START:
                continue
            if w == END:
                break
            ids.append(int(w))
        for k in range(1, 5):
            for p in range(len(ids) - k + 1):
                out[tuple(ids[p:p + k])] = True
    return list(out)


def make_tables(seqs, seed):
    """[(name, keys, vals, log_d, idf by word tuples)]: the four kinds of table."""
    from acvae_amd.consensus import Consensus
    rng = np.random.default_rng(seed)
    grams = ngrams_of(seqs)
    word = VOCAB.idx2word
    out = [("empty", [], [], 1.0, {})]
    g = grams[0] if grams else (5,)
    out.append(("one", [pack(g)], [0.37], 1.3, {tuple(word[i] for i in g): 0.37}))
    inside = [grams[i] for i in range(0, len(grams), 2)]                      # every other n-gram of the rows inside
    chosen = {pack(g): g for g in inside}
    theirs = set(grams)
    while len(chosen) < 5000:
        g = tuple(int(x) for x in rng.integers(0, V, rng.integers(1, 5)))
        if g not in theirs:
            chosen.setdefault(pack(g), g)
    keys = sorted(chosen)
    vals = rng.uniform(0.0, 2.0, len(keys))
    out.append(("5000", keys, vals, 2.2, {tuple(word[i] for i in chosen[k]): float(v) for k, v in zip(keys, vals)}))
    corpus = {"only": [CU.sentence_of(r, VOCAB) for r in np.asarray(seqs)[:3]]}
    c = Consensus(VOCAB, corpus)
    idf, log_d = MU.corpus_idf(corpus)
    assert c.log_d == 0.0 == log_d
    out.append(("one-document", c.idf_keys, c.idf_vals, c.log_d, idf))
    return out


def check(tag, seqs, sample_n, seed=0):
    """Every table on the rows `seqs`: scores within the bound, best / picked, two launches bit-equal."""
    seqs = np.asarray(seqs)
    B = len(seqs) // sample_n
    grams = set(ngrams_of(seqs))
    worst = 0.0
    for name, keys, vals, log_d, idf in make_tables(seqs, seed):
        if name == "5000":
            held = len({pack(g) for g in grams} & set(keys))
            assert len(keys) == 5000 and (not grams or 0 < held) and (len(grams) < 2 or held < len(grams))
        score, best, picked = launch(seqs, sample_n, keys, vals, log_d)
        again = launch(seqs, sample_n, keys, vals, log_d)
        only = launch(seqs, sample_n, keys, vals, log_d, pick=False)          # picked is optional
        torch.cuda.synchronize()
        for a, b, c in zip((score, best, picked), again, only):
            assert torch.equal(a, b), (tag, name)
            assert c is None or torch.equal(a, c), (tag, name)
        got, best, picked = score.cpu().numpy(), best.cpu().numpy(), picked.cpu().numpy()
        want = MU.clip_scores(seqs, sample_n, VOCAB, CU.sentence_of, idf, log_d)
        err = np.abs(got - want)
        worst = max(worst, float((err / CU.bound(want)).max()))
        assert np.all(err <= CU.bound(want)), (tag, name, got, want)
        assert np.array_equal(best, got.argmax(axis=1)), (tag, name, best, got)      # the first maximum of the device's scores
        top = want.max(axis=1)
        assert np.all(want[np.arange(B), best] >= top - 2.0 * CU.bound(top)), (tag, name, best, want)
        assert np.array_equal(picked, seqs[np.arange(B) * sample_n + best]), (tag, name)
        if name == "one-document":
            assert not got.any() and not best.any()
    print(f"{tag}: worst difference {worst:.3g} of the bound")
    return worst


def random_clips(B, sample_n, T, seed):
    """Rows over a few words, so that a clip's candidates share n-grams; some cut short, one empty where there is room."""
    rng = np.random.default_rng(seed)
    seqs = rng.integers(3, 12, (B * sample_n, T))
    seqs[rng.random(seqs.shape) < 0.04] = START
    for i in range(len(seqs)):
        if T > 2 and rng.random() < 0.6:
            seqs[i, rng.integers(1, T)] = END
    if B * sample_n > 3 and T > 1:
        seqs[3, 0] = END
    for b in range(B):                                   # a candidate that repeats another's beginning
        if T >= 4:
            seqs[b * sample_n + 1, :T // 2] = seqs[b * sample_n, :T // 2]
    return seqs


@pytest.mark.parametrize("T", [1, 2, 4, 20, 64])
@pytest.mark.parametrize("sample_n", [2, 3, 5, 16])
def test_kernel_against_the_yardstick(sample_n, T):
    for B in (1, 3):
        check(f"N{sample_n} B{B} T{T}", random_clips(B, sample_n, T, 7 * sample_n + T + B), sample_n, seed=T + B)


@pytest.mark.parametrize("T", [4, 20, 64])
def test_planted_rows(T):
    w = [4 + i for i in range(40)]
    fill = w[30]

    def row(ids, end=True, pad=fill):
        ids = list(ids)[:T - 1 if end else T] + ([END] if end else [])
        return ids + [pad] * (T - len(ids))
    # one clip of five: empty, one word, <start> in mid-row, no <end> at full length, one word repeated to the end
    mixed = [[END] + [w[0]] * (T - 1), row([w[0]]), [w[0], START, w[1], END][:T] + [w[2]] * max(0, T - 4),
             row([w[i % 3] for i in range(T)], end=False), [w[0]] * T]
    # all candidates identical; no two candidates sharing a word (every score 0: best == 0)
    same = [row([w[0], w[1], w[2], w[1], w[0]]) for _ in range(5)]
    apart = [row([w[5 * j + i] for i in range(3)]) for j in range(5)]
    # counts above 1 on both sides: clipping at the smaller weight
    clipped = [row([w[0]] * 2 + [w[1]]), row([w[0]] * 3), row([w[0]]), row([w[1], w[0], w[0], w[0]][:T - 1]), row([w[1]] * 3)]
    seqs = np.array(mixed + same + apart + clipped)
    check(f"planted T{T}", seqs, 5, seed=T)
    score, best, _ = launch(seqs, 5, [], [], 1.0)
    score, best = score.cpu().numpy(), best.cpu().numpy()
    assert score[0, 0] == 0.0                                        # the empty candidate
    full = 10.0 * min(4, 5, T - 1) / 4.0                             # identical candidates agree fully in every order they
    assert np.all(np.abs(score[1] - full) <= 1e-11) and best[1] == 0  # have n-grams of; the lowest index wins
    assert not score[2].any() and best[2] == 0
    # sixteen candidates, the last two identical and unlike the rest: they are each other's only agreement
    rows16 = [row([w[2 * j], w[2 * j + 1]]) for j in range(14)] + [row([w[35], w[36], w[37]])] * 2
    check(f"planted16 T{T}", np.array(rows16), 16, seed=T + 1)
    assert int(launch(np.array(rows16), 16, [], [], 1.0)[1].cpu()) == 14


def test_einval_returns_without_a_launch():
    out = torch.full((4096,), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    for kw, rc in einval_cases(_lib.lib(), out.data_ptr()):
        assert rc == -1, kw
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())                                 # nothing ran: every output word is as it was
    with pytest.raises(RuntimeError, match="EINVAL"):
        launch(np.zeros((10, 20), dtype=np.int64), 1, [], [], 1.0)


# ---------------------------------------------------------------------------------------------- the model and evaluate()
MV, ME, ML, MB, MN = 40, 64, 12, 3, 5
MVOCAB = Vocabulary(SPECIALS + [f"w{i}" for i in range(4, MV)])
MCORPUS = {f"k{d}": [" ".join(f"w{4 + (3 * d + 5 * c + i) % 30}" for i in range(4 + c)) for c in range(3)] for d in range(6)}
_model = {}


def small():
    """A small model (closed-form weights, V = 40, E = 64) on the GPU, the bias of <end> lowered so that captions differ
    in length, and its features."""
    if not _model:
        state = O.closed_form_state(O.state_shapes(MV, ME, ME, None, ME, 512))
        state["decoder.classifier.bias"] = state["decoder.classifier.bias"].clone()
        state["decoder.classifier.bias"][O.END_IDX] -= 2.0
        feats, _, feat_lens, _ = O.synthetic_batch(MB, 64, MV, 6, seed=5, ragged=False)
        _model["m"] = (build_model(MV, ME, state).eval(), feats.cuda(), feat_lens)
    return _model["m"]


CASES = [dict(method="sample", rng="device"), dict(method="sample", rng="device", top_p=0.8, no_repeat_ngram_size=2),
         dict(method="greedy"), dict(method="greedy", no_repeat_ngram_size=2)]


@pytest.mark.parametrize("corpus", [None, MCORPUS], ids=["no-table", "corpus"])
@pytest.mark.parametrize("kw", CASES, ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_rollouts_reranked(kw, corpus):
    from acvae_amd.consensus import Consensus
    model, feats, lens = small()
    rr = Consensus(MVOCAB, corpus)
    idf, log_d = MU.corpus_idf(corpus) if corpus else ({}, 1.0)
    torch.manual_seed(11)
    with torch.no_grad():
        plain = model.rollout_shared_encoder(feats, np.asarray(lens).copy(), MN, max_length=ML, **kw)
    torch.manual_seed(11)
    with torch.no_grad():
        out = model.rollout_shared_encoder(feats, np.asarray(lens).copy(), MN, max_length=ML, rerank=rr, **kw)
    torch.cuda.synchronize()
    cand, seqs = out["candidates"].cpu().numpy(), out["seqs"].cpu().numpy()
    got, best = out["consensus_scores"].cpu().numpy(), out["consensus_best"].cpu().numpy()
    assert "candidates" not in plain and np.array_equal(plain["seqs"].cpu().numpy(), cand)      # the same rollouts
    assert cand.shape == (MB * MN, ML) and seqs.shape == (MB, ML) and got.shape == (MB, MN) and best.shape == (MB,)
    assert got.dtype == np.float64 and best.dtype == np.int64
    assert np.array_equal(seqs, cand[np.arange(MB) * MN + best])
    want = MU.clip_scores(cand, MN, MVOCAB, CU.sentence_of, idf, log_d)
    assert np.all(np.abs(got - want) <= CU.bound(want)), (got, want)
    assert np.array_equal(best, got.argmax(axis=1))
    if kw["method"] == "sample":
        assert len({tuple(r) for r in cand.tolist()}) > MB           # the clips' rollouts are not all alike: there is a choice
    print(f"scores {got.min():.3f} .. {got.max():.3f}, best {best.tolist()}")


def test_evaluate_writes_the_picked_caption(tmp_path):
    from acvae_amd.batch import collate_fn, forward_batch_shared_encoder
    from acvae_amd.consensus import Consensus
    model, _, _ = small()
    voc = EV.Vocabulary()
    for word in MVOCAB.idx2word.values():
        voc.add_word(word)
    rr = Consensus(voc, MCORPUS)
    g = torch.Generator().manual_seed(5)
    items = [(f"clip{i}", torch.randn(64, 64, generator=g)) for i in range(3)]
    kw = dict(method="sample", rng="device", beam_size=MN, max_length=ML, top_p=0.9)
    torch.manual_seed(21)
    path = tmp_path / "pred.json"
    payload = EV.evaluate(model, items, voc, caption_output=path, batch_size=3, rerank=rr, **kw)
    torch.manual_seed(21)
    batch = collate_fn([1])(list(items))
    with torch.no_grad():
        out = forward_batch_shared_encoder(model, batch, rerank=rr, **kw)
    assert list(batch[0]) == ["clip0", "clip1", "clip2"]                   # one row per clip: the keys are the clips'
    seqs = out["seqs"].cpu().numpy()
    preds = payload["predictions"]
    assert [p["filename"] for p in preds] == list(batch[0]) and all("captions" not in p for p in preds)
    assert [p["caption"] for p in preds] == [EV.convert_idx2sentence(r, voc) for r in seqs]
    assert path.exists()
    torch.manual_seed(21)
    many = EV.evaluate(model, items, voc, batch_size=3, rerank=None, **kw)          # None: the N-captions form of before
    assert all(len(p["captions"]) == MN for p in many["predictions"])
    cand = out["candidates"].cpu().numpy()
    assert [c["caption"] for p in many["predictions"] for c in p["captions"]] == [EV.convert_idx2sentence(r, voc) for r in cand]


def test_refusals_on_the_device_model():
    from acvae_amd.consensus import Consensus
    model, feats, lens = small()
    rr = Consensus(MVOCAB)
    items = [("clip0", torch.zeros(64, 64))]
    calls = []
    real = _lib.call
    _lib.call = lambda *a: (calls.append(a[0]), real(*a))[1]
    try:
        for method in ("beam", "dbs"):
            with pytest.raises(ValueError, match="rerank with method"):
                EV.evaluate(model, items, MVOCAB, method=method, beam_size=5, rerank=rr)
            with pytest.raises(ValueError, match="rerank with method"):
                model.rollout_shared_encoder(feats, np.asarray(lens).copy(), 5, method=method, rerank=rr)
        for n in (1, 17):
            with pytest.raises(ValueError, match="2 <= N <= 16"):
                EV.evaluate(model, items, MVOCAB, method="sample", beam_size=n, rerank=rr)
            with pytest.raises(ValueError, match="2 <= N <= 16"):
                model.rollout_shared_encoder(feats, np.asarray(lens).copy(), n, method="sample", rerank=rr)
        with pytest.raises(ValueError, match="training forward"):
            model(feats, np.asarray(lens).copy(), torch.ones(MB, 5, dtype=torch.long), np.array([5] * MB), ss_ratio=1.0,
                  dis_ratio=0, rerank=rr)
        with pytest.raises(ValueError, match="know N"):
            model(feats, np.asarray(lens).copy(), method="sample", rerank=rr)
        model.train()
        try:
            with pytest.raises(ValueError, match="differentiable rollout"):
                model.rollout_shared_encoder(feats, np.asarray(lens).copy(), 5, method="sample", rerank=rr)
        finally:
            model.eval()
    finally:
        _lib.call = real
        model.eval()
    assert calls == []                                               # every refusal came in front of the first launch
