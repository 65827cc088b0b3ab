"""CPU: the yardstick of the caption-likelihood kernels against brute force, the mutants its bounds must flag, the Python
refusals (each in front of any library call) and ``Likelihood.result()``'s formulas on hand-made records."""
import math
import types

import numpy as np
import pytest
import torch

import likelihood_util as LU
import text_ref as R
from acvae_amd import _lib, likelihood as lk
from acvae_amd.evaluate import Vocabulary, evaluate_likelihood
from text_ref import D


# ------------------------------------------------------------------------------------------------ the yardstick
def test_rank_is_the_position_in_a_stable_descending_sort():
    g = torch.Generator().manual_seed(3)
    x = torch.randint(-2, 3, (4, 6, 11), generator=g).float()           # many ties
    tg = torch.randint(0, 11, (4, 6), generator=g)
    _, rank, _ = LU.terms(x, tg, None)
    order = torch.sort(x, dim=-1, descending=True, stable=True).indices
    want = (order == tg.unsqueeze(-1)).float().argmax(-1)
    assert torch.equal(rank, want)
    # rank 0 is exactly "the greedy decode emits the target": torch.max's first maximum
    assert torch.equal(rank == 0, x.max(-1).indices == tg)


def test_logprob_and_kl_against_brute_force():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 3, 7, generator=g)
    tg = torch.randint(0, 7, (2, 3), generator=g)
    lens1 = torch.tensor([3, 1])
    gauss = [torch.randn(2, 3, 5, generator=g) for _ in range(4)]
    lp, rank, kl = LU.terms(x, tg, lens1, gauss)
    for r in range(2):
        for t in range(3):
            if t >= int(lens1[r]):
                assert lp[r, t] == 0 and rank[r, t] == 0 and kl[r, t] == 0
                continue
            p = [math.exp(float(v)) for v in x[r, t]]
            assert abs(float(lp[r, t]) - math.log(p[int(tg[r, t])] / sum(p))) < 1e-12
            mu1, lv1, mu2, lv2 = (gq[r, t].double() for gq in gauss)
            want = sum(float(lv2[e] / 2 - lv1[e] / 2 + (math.exp(lv1[e]) + (mu1[e] - mu2[e]) ** 2) / (2 * math.exp(lv2[e])) - .5)
                       for e in range(5))
            assert abs(float(kl[r, t]) - want) < 1e-12
    nll, ks, tokens, h1, h5 = LU.sums(lp, rank, kl, lens1)
    assert list(tokens) == [3, 1]
    assert abs(nll[0] + float(lp[0].sum())) < 1e-12 and abs(ks[1] - float(kl[1, 0])) < 1e-15
    assert h1[0] == int((rank[0] < 1).sum()) and h5[0] == int((rank[0] < 5).sum())


def test_logmeanexp_against_the_plain_mean_of_exp():
    x = np.array([[-1.5, -2.0, -0.25], [0.5, 0.5, 0.5]])
    want = np.log(np.exp(x).mean(axis=-1))
    assert LU.lme_ok(LU.logmeanexp(x), want)
    assert LU.lme_ok(lk.logmeanexp(x), want)                            # the product's own
    big = np.array([[-800.0, -803.0, -801.0]])                          # exp underflows without the shift
    assert LU.lme_ok(lk.logmeanexp(big), LU.logmeanexp(big)) and np.isfinite(LU.logmeanexp(big)).all()


# ------------------------------------------------------------------------------------------------ mutants
def _case():
    buf, tgb, lens1 = R.ce_case(63, "zero")
    N, T = buf.shape[:2]
    x, tg = buf[..., :63], tgb[:, :T]
    px, ptg = LU.planted(63)
    g = torch.Generator().manual_seed(9)
    gauss = [torch.randn(N, T, 8, generator=g) for _ in range(4)]
    return x, tg, lens1, gauss, px, ptg


def test_term_mutants_are_flagged():
    x, tg, lens1, gauss, px, ptg = _case()
    lp, rank, kl = LU.terms(x, tg, lens1, gauss)
    tlp, tkl = LU.logprob_tol(x, tg, lens1), LU.kl_tol(gauss, lens1)
    # the fp32 restatement passes its own bounds (they are not so tight that a correct kernel could not meet them)
    lp32 = torch.where(LU.mask(lens1, *x.shape[:2]), x.gather(-1, tg.unsqueeze(-1)).squeeze(-1) - torch.logsumexp(x, -1),
                       torch.zeros(()))
    assert not R.flagged(lp32, lp, tlp)
    kl32 = torch.where(LU.mask(lens1, *x.shape[:2]), R.kl_terms(*gauss, dtype=torch.float32).view(*x.shape[:2], -1).sum(-1),
                       torch.zeros(()))
    assert not R.flagged(kl32, kl, tkl)
    m_lp, m_rank, _ = LU.terms(x, tg, lens1, gauss, mutant="mask_at_len+1")
    assert R.flagged(m_lp, lp, tlp) and not torch.equal(m_rank, rank)
    _, _, m_kl = LU.terms(x, tg, lens1, gauss, mutant="kl_unmasked")
    assert R.flagged(m_kl, kl, tkl)
    _, prank, _ = LU.terms(px, ptg, None)
    _, m_prank, _ = LU.terms(px, ptg, None, mutant="tie_rule_reversed")
    assert not torch.equal(m_prank, prank)
    assert int(prank[0, 3]) == int(ptg[0, 3]) and int(prank[0, 4]) == 0 and int(prank[0, 5]) >= 1


def test_logmeanexp_mutants_are_flagged():
    x = -np.array([[801.0, 795.5, 810.25], [30.0, 31.0, 29.5]])         # -nll of three draws
    ref = LU.logmeanexp(x)
    for mutant in LU.LME_MUTANTS:
        assert not LU.lme_ok(LU.logmeanexp(x, mutant), ref), mutant
    # the estimate lies between the mean and the max of the draws
    assert (ref > x.mean(axis=-1)).all() and (ref <= x.max(axis=-1)).all()


# ------------------------------------------------------------------------------------------------ refusals
def _fake_model(hidden=64, embed=64):
    dec = types.SimpleNamespace(model=types.SimpleNamespace(hidden_size=hidden), embed_size=embed)

    def boom(*a, **k):
        raise AssertionError("the model was touched")
    return types.SimpleNamespace(decoder=dec, parameters=boom, modules=boom, eval=boom, encoder=boom)


@pytest.fixture
def no_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a library call in front of the refusal")
    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(_lib, "call", boom)
    monkeypatch.setattr(_lib, "h2d", boom)
    monkeypatch.setattr(torch, "randn", boom)
    monkeypatch.setattr(torch, "rand", boom)


CAPS = torch.tensor([[1, 5, 6, 2], [1, 7, 2, 0], [1, 2, 0, 0]])
GOOD = dict(feats=torch.zeros(3, 64, 64), feat_lens=np.array([64, 64, 64]), caps=CAPS, cap_lens=np.array([4, 3, 2]))


@pytest.mark.parametrize("what, change, match", [
    ("samples 0", dict(samples=0), "samples"),
    ("samples 17", dict(samples=17), "samples"),
    ("samples True", dict(samples=True), "samples"),
    ("z", dict(z="both"), "z must be one of"),
    ("short caption", dict(cap_lens=np.array([4, 3, 1])), "<start> <end>"),
    ("unequal captions per clip", dict(clip_index=np.array([0, 0, 1])), "same number of captions.*pad"),
    ("clip out of range", dict(clip_index=np.array([0, 1, 3])), "clip_index"),
    ("captions without clip_index", dict(cap_lens=np.array([4, 3]), caps=CAPS[:2]), "clip_index"),
])
def test_score_captions_refuses_before_any_library_call(no_library, what, change, match):
    with pytest.raises(ValueError, match=match):
        lk.score_captions(_fake_model(), **dict(GOOD, **change))


def test_score_captions_refuses_unequal_widths_and_augmented_front_ends(no_library):
    with pytest.raises(ValueError, match="hidden_size"):
        lk.score_captions(_fake_model(hidden=128), **GOOD)
    from acvae_amd.frontend import Augmented
    aug = Augmented.__new__(Augmented)
    with pytest.raises(ValueError, match="never augments"):
        lk.score_captions(_fake_model(), frontend=aug, **GOOD)


def _vocab():
    v = Vocabulary()
    for w in ("<pad>", "<start>", "<end>", "<unk>", "a", "dog", "barks"):
        v.add_word(w)
    return v


def test_evaluate_likelihood_refuses_before_any_library_call(no_library):
    items = [("c0", torch.zeros(64, 64)), ("c1", torch.zeros(64, 64))]
    good = {"c0": ["a dog", "a dog barks"], "c1": ["a", "dog barks"]}
    m = _fake_model()
    with pytest.raises(ValueError, match="samples"):
        evaluate_likelihood(m, items, good, _vocab(), batch_size=2, samples=0)
    with pytest.raises(ValueError, match="z must be one of"):
        evaluate_likelihood(m, items, good, _vocab(), batch_size=2, z=("posterior", "iwae"))
    with pytest.raises(ValueError, match="same number of captions"):
        evaluate_likelihood(m, items, dict(good, c1=["a"]), _vocab(), batch_size=2)
    with pytest.raises(ValueError, match="no captions"):
        evaluate_likelihood(m, items, dict(good, c1=[]), _vocab(), batch_size=2)
    # unequal sets are fine one clip per batch; an item that key2caps lacks is known only when it arrives, still in front
    # of any library call (the items are not materialised: the generator is read no further than that item)
    seen = []

    def stream():
        for item in items:
            seen.append(item[0])
            yield item
    quiet = types.SimpleNamespace(decoder=m.decoder, parameters=lambda: iter([torch.zeros(1)]), modules=lambda: [],
                                  eval=lambda: None)
    with pytest.raises(ValueError, match="no captions in key2caps"):
        evaluate_likelihood(quiet, stream(), {"c1": ["a"], "zz": ["a", "dog"]}, _vocab(), batch_size=1)
    assert seen == ["c0"]
    with pytest.raises(ValueError, match="without words"):
        evaluate_likelihood(m, items, dict(good, c1=["a", "  "]), _vocab(), batch_size=2)
    with pytest.raises(ValueError, match="hidden_size"):
        evaluate_likelihood(_fake_model(embed=32), items, good, _vocab(), batch_size=2)


def test_rows_order_pairs_by_length_with_adjacent_draws():
    rows = lk.Rows(np.array([3, 5, 3, 4]), np.array([1, 0, 0, 1]), 2, 2)
    assert list(rows.pair) == [1, 1, 3, 3, 0, 0, 2, 2]                  # descending, stable; the K draws adjacent
    assert list(rows.clip) == [0, 0, 1, 1, 1, 1, 0, 0]
    assert list(rows.lens) == [5, 5, 4, 4, 3, 3, 3, 3]
    assert list(rows.place) == [2, 0, 3, 1]
    assert list(rows.pair[rows.place * 2]) == [0, 1, 2, 3]


# ------------------------------------------------------------------------------------------------ the formulas
def _record(z, nll, kl, tokens, hit1, hit5, kl_steps):
    return {"z": z, "samples": len(nll[0]), "nll": torch.tensor(nll, dtype=D), "kl": torch.tensor(kl, dtype=D),
            "tokens": torch.tensor(tokens, dtype=torch.int32), "hit1": torch.tensor(hit1, dtype=torch.int32),
            "hit5": torch.tensor(hit5, dtype=torch.int32), "kl_steps": torch.tensor(kl_steps, dtype=torch.float32)}


def test_result_formulas_on_hand_made_records():
    # two updates of different widths; K = 2
    a = _record("prior", [[4.0, 6.0], [1.0, 1.0]], [[2.0, 4.0], [0.5, 1.5]], [3, 1], [[1, 2], [1, 0]], [[3, 3], [1, 1]],
                [[[1.0, 0.5, 0.5], [2.0, 1.0, 1.0]], [[0.5, 0.0, 0.0], [1.5, 0.0, 0.0]]])
    b = _record("prior", [[2.0, 3.0]], [[1.0, 1.0]], [2], [[0, 1]], [[2, 2]], [[[0.25, 0.75], [0.5, 0.5]]])
    meter = lk.Likelihood("prior", 2)
    meter.update(["p0", "p1"], a)
    meter.update(["p2"], b)
    res = meter.result()
    marg = [math.log((math.exp(-4) + math.exp(-6)) / 2), -1.0, math.log((math.exp(-2) + math.exp(-3)) / 2)]
    assert [p["key"] for p in res["pairs"]] == ["p0", "p1", "p2"]
    for p, m, n, k, t in zip(res["pairs"], marg, (5.0, 1.0, 2.5), (3.0, 1.0, 1.0), (3, 1, 2)):
        assert abs(p["log_marginal"] - m) < 1e-12 and p["nll"] == n and p["kl"] == k and p["tokens"] == t
    assert res["tokens"] == 6 and res["captions"] == 3 and res["samples"] == 2
    assert abs(res["nll_per_token"] - (-sum(marg) / 6)) < 1e-12
    assert abs(res["perplexity"] - math.exp(-sum(marg) / 6)) < 1e-12
    assert abs(res["kl_per_token"] - 5.0 / 6) < 1e-12
    assert abs(res["top1"] - 5 / 12) < 1e-12 and abs(res["top5"] - 1.0) < 1e-12
    # step 0: all three captions, both draws; step 1: p0 and p2; step 2: p0 alone
    want = [(1.0 + 2.0 + 0.5 + 1.5 + 0.25 + 0.5) / 6, (0.5 + 1.0 + 0.75 + 0.5) / 4, (0.5 + 1.0) / 2]
    assert np.allclose(res["kl_by_step"], want, rtol=0, atol=1e-12)
    # the posterior's score is the mean reconstruction term, and it claims no marginal
    post = lk.Likelihood("posterior", 2)
    a["z"] = "posterior"
    post.update(["p0", "p1"], a)
    res = post.result()
    assert res["pairs"][0]["log_marginal"] is None
    assert abs(res["nll_per_token"] - 6.0 / 4) < 1e-12 and abs(res["perplexity"] - math.exp(1.5)) < 1e-12
    with pytest.raises(ValueError, match="record of z"):
        post.update(["p2"], b)
    with pytest.raises(ValueError, match="without an update"):
        lk.Likelihood().result()
