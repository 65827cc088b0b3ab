"""CPU: the yardstick of consensus reranking (tests/consensus_util.py) tied to the CIDEr-D yardstick (tests/cider_util.py),
and the host side of acvae_amd/consensus.py: the corpus's (key, idf) table, the constructor's refusals, the argument
checks of the entry point (no launch without a GPU) and the refusals of ``rerank=`` that need no device."""
import math

import numpy as np
import pytest

import cider_util as CU
import consensus_util as MU
from cider_util import SPECIALS, Vocabulary

START, END = 1, 2


def vocab_of(V):
    return Vocabulary(SPECIALS + [f"w{i}" for i in range(4, V)])


def pack(ids):
    return sum((int(w) + 1) << (16 * j) for j, w in enumerate(ids))


CORPUS = {"a": ["the dog barks at the cat", "a dog barks", "the the the cat"],
          "b": ["rain falls on a tin roof", "rain falls"],
          "c": ["the dog sleeps on a tin roof while rain falls", "birds sing"],
          "d": ["wind"]}


def test_yardstick_is_ciderd_with_the_other_candidates_as_references():
    """consensus(0) of [h] + gts[d] under the corpus's idf is CIDEr-D of h against document d's references."""
    idf, log_d = MU.corpus_idf(CORPUS)
    assert log_d == math.log(4.0) and idf[("the",)] == math.log(4.0) - math.log(2.0) and idf[("wind",)] == log_d
    hyps = ["the dog barks at the cat", "", "the the the the cat the the", "rain falls on the dog", "okapi", "a tin roof",
            "wind", "the dog barks at the cat on a tin roof while rain falls and birds sing"]
    worst = 0.0
    for h in hyps:
        want = CU.ciderd(CORPUS, {d: [h] for d in CORPUS})[1]
        for at, d in enumerate(CORPUS):
            got = MU.consensus([h] + CORPUS[d], idf, log_d)[0]
            worst = max(worst, abs(got - want[at]) / CU.bound(want[at]))
            assert abs(got - want[at]) <= CU.bound(want[at]), (h, d, got, want[at])
    assert MU.consensus([""] + CORPUS["a"], idf, log_d)[0] == 0.0
    print(f"worst difference {worst:.3g} of the bound")


def test_yardstick_anchors():
    # no table, log_d = 1: every n-gram weighs 1; identical candidates agree fully, disjoint ones not at all
    assert np.all(np.abs(MU.consensus(["a b c d e"] * 3) - 10.0) <= 1e-12 * 10)
    assert MU.consensus(["a b c", "d e f", "g h"]).tolist() == [0.0, 0.0, 0.0]
    # two one-word candidates "a" vs "a a a": unigram vectors (1) and (3), clipped: min(1, 3) * 3 / (1 * 3) = 1 and
    # min(3, 1) * 1 / (3 * 1) = 1/3; lengths 0 and 2 bigrams; only the first order is non-zero for the first candidate
    pen = math.exp(-4.0 / 72.0)
    got = MU.consensus(["a", "a a a"])
    assert abs(got[0] - 10.0 * pen / 4.0) <= 1e-12 and abs(got[1] - 10.0 * pen / 3.0 / 4.0) <= 1e-12
    # a corpus of one document: ln 1 = 0, every weight 0, every score 0
    idf, log_d = MU.corpus_idf({"only": ["a b c"]})
    assert log_d == 0.0 and MU.consensus(["a b c", "a b c"], idf, log_d).tolist() == [0.0, 0.0]


def test_host_table():
    from acvae_amd.consensus import Consensus
    words = SPECIALS + "the dog barks at cat a rain falls on tin roof".split()
    vocab = Vocabulary(words)
    w2i = {w: i for i, w in enumerate(words)}
    c = Consensus(vocab, CORPUS)
    assert c.n_docs == 4 and c.log_d == math.log(4.0)              # keys "c" and "d" hold out-of-vocabulary words: they count in D
    assert c.idf_keys.dtype == np.uint64 and c.idf_vals.dtype == np.float64
    assert np.all(c.idf_keys[1:] > c.idf_keys[:-1])                # strictly ascending: the kernel bisects
    idf, log_d = MU.corpus_idf(CORPUS)
    inside = {g: v for g, v in idf.items() if all(w in w2i for w in g)}
    assert len(inside) == c.idf_keys.size and len(inside) < len(idf)
    table = dict(zip((int(k) for k in c.idf_keys), c.idf_vals))
    for g, v in inside.items():
        assert table[pack([w2i[w] for w in g])] == v, g            # the same two logarithms: bit-equal
    # out-of-vocabulary words: "sleeps", "while", "birds", "sing", "wind" get no entry, alone or inside an n-gram
    assert pack([w2i["dog"]]) in table and ("dog", "sleeps") in idf
    assert table[pack([w2i["rain"], w2i["falls"]])] == math.log(4.0) - math.log(2.0)     # keys "b" and "c"
    assert table[pack([w2i["the"]])] == math.log(4.0) - math.log(2.0)                   # df counts keys, not captions
    # no corpus: the empty table, every n-gram weighs 1
    e = Consensus(vocab)
    assert e.idf_keys.size == 0 and e.idf_vals.size == 0 and e.log_d == 1.0
    assert e.len_factor.size == 64 and e.len_factor[0] == 1.0 and abs(e.len_factor[3] - math.exp(-9.0 / 72.0)) <= 4e-16
    assert abs(Consensus(vocab, sigma=2.0).len_factor[3] - math.exp(-9.0 / 8.0)) <= 4e-16    # (numpy's exp: an ulp or two)
    one = Consensus(vocab, {"only": ["the dog barks"]})
    assert one.log_d == 0.0 and not one.idf_vals.any() and one.idf_keys.size == 6


def test_constructor_refusals():
    from acvae_amd.consensus import MAX_VOCAB, Consensus
    with pytest.raises(ValueError, match="share the word"):
        Consensus(Vocabulary(SPECIALS + ["cat", "dog", "cat"]))
    for bad in ("two words", "", "tab\there", " lead"):
        with pytest.raises(ValueError, match="whitespace"):
            Consensus(Vocabulary(SPECIALS + [bad]))
    with pytest.raises(ValueError, match="16 bits"):
        Consensus(Vocabulary([f"w{i}" for i in range(MAX_VOCAB + 1)]))
    Consensus(Vocabulary([f"w{i}" for i in range(MAX_VOCAB)]))
    with pytest.raises(ValueError, match="no keys"):
        Consensus(vocab_of(10), {})

    class ListVocabulary:
        idx2word = SPECIALS + ["cat"]
    assert Consensus(ListVocabulary()).word2id["cat"] == 4


def einval_cases(lib, p):
    """Every refusal of acvae_consensus_scores, with `p` a valid pointer for every array -> [(case, return code)]."""
    def call(**kw):
        a = dict(seqs=p, ld=20, n=10, sample_n=5, max_length=20, start_idx=1, end_idx=2, idf_keys=p, idf_vals=p, n_idf=3,
                 log_d=1.0, len_factor=p, n_len=64, score=p, best=p, picked=p, stream=None)
        a.update(kw)
        return lib.acvae_consensus_scores(*a.values())
    cases = (dict(seqs=None), dict(len_factor=None), dict(score=None), dict(best=None), dict(idf_keys=None), dict(idf_vals=None),
             dict(sample_n=1), dict(sample_n=0), dict(sample_n=17, n=34), dict(sample_n=-5), dict(n=0), dict(n=-5), dict(n=11),
             dict(n=4), dict(max_length=0), dict(max_length=65, ld=65), dict(ld=19), dict(n_len=0), dict(n_len=-1),
             dict(n_idf=-1))
    return [(kw, call(**kw)) for kw in cases]


def test_entry_point_refuses_bad_arguments_before_any_launch():
    import torch
    from acvae_amd import _lib
    from acvae_amd.consensus import MAX_LENGTH, MAX_SAMPLES
    assert MAX_LENGTH == 64 and MAX_SAMPLES == 16
    p = torch.zeros(64, dtype=torch.float64).data_ptr()            # host memory: every refusal comes before any launch
    for kw, rc in einval_cases(_lib.lib(), p):
        assert rc == -1, kw


def test_rerank_refusals_that_need_no_device():
    import torch
    from acvae_amd.consensus import Consensus, check_sample_n
    from acvae_amd.decoder import VAERNNBahdanauAttnDecoder
    from acvae_amd.encoder import Cnn10
    from acvae_amd.vae_model import Hybrid_VAEModel
    V, E = 52, 64
    dec = VAERNNBahdanauAttnDecoder(vocab_size=V, enc_mem_size=E, embed_size=E, hidden_size=E, attn_size=E)
    model = Hybrid_VAEModel(Cnn10(64, 512), dec, posterior_model="PosteriorRNN_hybrid", posterior_args={"hidden_size": E},
                            prior_model="PriorRNN", prior_args={"hidden_size": E}).eval()
    rr = Consensus(vocab_of(V))
    feats, lens = torch.zeros(2, 64, 64), [64, 64]
    for method in ("beam", "dbs"):
        with pytest.raises(ValueError, match="rerank with method"):
            model.rollout_shared_encoder(feats, lens, 5, method=method, rerank=rr)
    for n in (1, 0, 17, True, 2.0):
        with pytest.raises(ValueError, match="2 <= N <= 16"):
            model.rollout_shared_encoder(feats, lens, n, method="sample", rerank=rr)
    assert check_sample_n(2) == 2 and check_sample_n(np.int64(16)) == 16
    with pytest.raises(ValueError, match="max_length=65"):
        model.rollout_shared_encoder(feats, lens, 5, method="sample", max_length=65, rerank=rr)
    with pytest.raises(ValueError, match="Consensus"):
        model.rollout_shared_encoder(feats, lens, 5, method="sample", rerank="cider")
    with pytest.raises(ValueError, match="training forward"):
        model(feats, lens, torch.zeros(2, 5, dtype=torch.long), [5, 5], ss_ratio=1.0, dis_ratio=0, rerank=rr)
    with pytest.raises(ValueError, match="know N"):
        model(feats, lens, method="sample", rerank=rr)
    with pytest.raises(ValueError, match="know N"):
        model.inference_forward({}, method="sample", rerank=rr)
    model.train()
    with pytest.raises(ValueError, match="differentiable rollout"):
        model.rollout_shared_encoder(feats, lens, 5, method="sample", rerank=rr)
    model.eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):     # a host tensor is no candidate set: nothing is scored on the host
        rr.select(torch.zeros(10, 20, dtype=torch.long), 5)
    with pytest.raises(ValueError, match="clip-major"):
        rr.select(torch.zeros(11, 20, dtype=torch.long), 5)
