"""CPU: the yardstick of the diversity metrics (tests/diversity_util.py) on hand-checked clips and on planted clips whose
answer changes under each plausible mistake, and the host side of acvae_amd/diversity.py: the formulas of ``summarize`` on
the yardstick's integers, the constructor's and ``update_payload``'s refusals, the argument checks of the entry point (no
launch without a GPU) and the refusals of ``evaluate(diversity=)`` that need no device."""
import math

import numpy as np
import pytest

import diversity_util as DU
from cider_util import SPECIALS, Vocabulary


def vocab_of(V):
    return Vocabulary(SPECIALS + [f"w{i}" for i in range(4, V)])


def test_hand_checked_clip():
    s = DU.clip_stats(["a a a b", "a a c"])
    assert s["words"] == 7 and s["distinct"][:2] == [3, 3]               # a b c;  (a a) (a b) (a c)
    assert s["distinct"] == [3, 3, 3, 1]                                 # (a a a) (a a b) (a a c);  (a a a b)
    c0, c1 = s["cands"]
    assert (c0["testlen"], c0["reflen"], c0["guess"], c0["correct"]) == (4, 3, [4, 3, 2, 1], [2, 1, 0, 0])
    assert (c1["testlen"], c1["reflen"], c1["guess"], c1["correct"]) == (3, 4, [3, 2, 1, 0], [2, 1, 0, 0])
    assert c0["clipped"] and c1["clipped"]                               # a: 3 against 2; c: 1 against 0
    assert DU.record_of(s) == [7, 3, 3, 3, 1, 4, 3, 2, 1, 0, 0, 3, 4, 2, 1, 0, 0]
    d = DU.diversity([["a a a b", "a a c"]])
    assert d["Div1"] == 3 / (1e-6 + 7.0) == d["Div2"] and d["gDiv1"] == 3.0 and d["clips"] == 1 and d["sample_n"] == 2
    # candidate 0: p1 = 2/4, ratio 4/3 >= 1: no penalty; candidate 1: p1 = 2/3, ratio 3/4: exp(1 - 4/3)
    want = 0.5 * (2.0 / 4.0 + 2.0 / 3.0 * math.exp(1.0 - 4.0 / 3.0))
    assert abs(d["mBLeu_1"] - want) <= 1e-9                              # (the 1e-9 of the denominators)


def test_identical_candidates_score_one():
    """(C + 1e-15) / (G + 1e-9) and the length ratio (TL + 1e-15) / (RL + 1e-9) fall short of 1 by 1e-9 / G: within 1e-12
    of 1 takes some thousand n-grams per candidate index, here 1000 clips of ten words (G_4 = 7000)."""
    d = DU.diversity([["a b c d e f g h i j"] * 3] * 1000)
    for k in range(1, 5):
        assert abs(d[f"mBLeu_{k}"] - 1.0) <= 1e-12, (k, d[f"mBLeu_{k}"] - 1.0)
    assert d["gDiv1"] == 10.0 and abs(d["Div1"] - 10 / 30) <= 1e-7 and abs(d["Div2"] - 9 / 30) <= 1e-7


def test_disjoint_candidates_share_nothing():
    s = DU.clip_stats(["a b c d", "e f g", "h i j k l"])
    assert all(c["correct"] == [0, 0, 0, 0] for c in s["cands"])
    assert s["distinct"] == [12, 9, 6, 3] and s["words"] == 12 and s["repeated"] == [False] * 4
    d = DU.diversity([["a b c d", "e f g", "h i j k l"]])
    assert d["Div1"] == 12 / (1e-6 + 12.0) and d["mBLeu_4"] < 1e-9


# ---- planted clips: each answer changes under one plausible mistake
def test_clipping_takes_the_maximum_over_references_not_their_sum():
    c = DU.clip_stats(["a a a", "a", "a"])["cands"][0]
    by_sum = min(3, 1 + 1)
    assert c["correct"][0] == 1 != by_sum


def test_reference_length_is_the_closest_and_ties_go_to_the_shorter():
    c = DU.clip_stats(["a b c d e", "a b", "a b c d e f"])["cands"][0]
    assert c["reflen"] == 6 != min(2, 6)                                 # not the shortest
    c = DU.clip_stats(["a b c d", "a b c", "a b c d e"])["cands"][0]
    assert c["reflen"] == 3 != 5                                         # |3 - 4| == |5 - 4|: the shorter
    c = DU.clip_stats(["a b c d", "a b c d e", "a b c"])["cands"][0]
    assert c["reflen"] == 3                                              # whatever their order
    # and the penalty sees it: with reflen 5 candidate 0 would be penalised (4 < 5), with 3 it is not
    d = DU.diversity([["a b c d", "a b c", "a b c d e"]])
    cand = [dict(c, reflen=5) for c in [d["stats"][0]["cands"][0]]]
    assert DU.corpus_bleu(cand)[0] < DU.corpus_bleu([d["stats"][0]["cands"][0]])[0]


def test_div2_divides_by_words_not_by_bigrams():
    d = DU.diversity([["a b c", "a b d"]])
    bigrams = 2 + 2
    assert d["Div2"] == 3 / (1e-6 + 6.0) and abs(d["Div2"] - 3 / bigrams) > 0.2


def test_distinct_counts_an_ngram_once():
    s = DU.clip_stats(["a a", "a"])
    occurrences = 3
    assert s["distinct"] == [1, 1, 0, 0] and s["distinct"][0] != occurrences and s["repeated"] == [True, False, False, False]


def test_corpus_bleu_per_index_is_not_the_mean_of_sentence_bleu():
    clips = [["a b c d e f", "a b c d e f"], ["a b", "c d"]]
    d = DU.diversity(clips)
    per_clip = [DU.diversity([c])["mBLeu_1"] for c in clips]             # 1 and 0: their mean is 1/2
    assert abs(sum(per_clip) / 2 - 0.5) <= 1e-9
    assert abs(d["mBLeu_1"] - 6 / 8) <= 1e-9                             # C_1 = 6 + 0 over G_1 = 6 + 2


# ---- the host side of acvae_amd/diversity.py
CLIPS = [["a a a b", "a a c", ""], ["x y z w v", "x y z w v", "x y z w"], ["", "", ""], ["q", "q q q q q q", "r s t u"],
         ["a b c d e f g", "a b c d x f g", "g f e d c b a"]]


def test_summarize_evaluates_the_formulas_on_the_integers():
    from acvae_amd.diversity import HEAD, PER, record_ints, summarize
    assert (HEAD, PER) == (5, 6) and record_ints(3) == 23
    want = DU.diversity(CLIPS)
    record = np.array([DU.record_of(s) for s in want["stats"]], dtype=np.int32)
    got = summarize(record, 3, int(want["gDiv1"]))
    worst = 0.0
    for key in ("Div1", "Div2", "gDiv1", "mBLeu_1", "mBLeu_2", "mBLeu_3", "mBLeu_4"):
        worst = max(worst, abs(got[key] - want[key]) / DU.bound(want[key]))
        assert abs(got[key] - want[key]) <= DU.bound(want[key]), (key, got[key], want[key])
    for key in ("div1", "div2"):
        assert np.all(np.abs(got["per_clip"][key] - np.array(want["per_clip"][key])) <= 1e-12)
    assert got["clips"] == 5 and got["sample_n"] == 3
    assert set(got) == {"Div1", "Div2", "gDiv1", "mBLeu_1", "mBLeu_2", "mBLeu_3", "mBLeu_4", "clips", "sample_n", "per_clip"}
    print(f"worst difference {worst:.3g} of the bound")


def test_constructor_refusals():
    from acvae_amd.diversity import MAX_VOCAB, Diversity
    with pytest.raises(ValueError, match="share the word"):
        Diversity(Vocabulary(SPECIALS + ["cat", "dog", "cat"]))
    for bad in ("two words", "", "tab\there", " lead"):
        with pytest.raises(ValueError, match="whitespace"):
            Diversity(Vocabulary(SPECIALS + [bad]))
    with pytest.raises(ValueError, match="16 bits"):
        Diversity(Vocabulary(SPECIALS + [f"w{i}" for i in range(4, MAX_VOCAB + 1)]))
    d = Diversity(Vocabulary(SPECIALS + [f"w{i}" for i in range(4, MAX_VOCAB)]))
    assert d.V == MAX_VOCAB == 65534 and (d.start_idx, d.end_idx) == (1, 2)
    with pytest.raises(ValueError, match="no <end>"):
        Diversity(Vocabulary(["<pad>", "<start>", "cat"]))
    with pytest.raises(ValueError, match="no <start>"):
        Diversity(Vocabulary(["<pad>", "<end>", "cat"]))

    class ListVocabulary:
        idx2word = ["<end>", "cat", "<start>"]
    d = Diversity(ListVocabulary())
    assert (d.start_idx, d.end_idx, d.V) == (2, 0, 3)                   # the indices are the vocabulary's
    with pytest.raises(ValueError, match="without an update"):
        d.result()
    for n in (1, 0, 17, True, 2.0):
        with pytest.raises(ValueError, match="2 <= N <= 16"):
            d.check(n)
    assert d.check(2) == 2 and d.check(np.int64(16)) == 16 and d.sample_n is None


def payload_of(clips):
    return {"predictions": [{"filename": f"clip{b}", "captions": [{"caption": c, "cap_id": i, "tokens": c}
                                                                   for i, c in enumerate(caps)]}
                            for b, caps in enumerate(clips)]}


def test_update_payload_refusals():
    import torch
    from acvae_amd.diversity import Diversity
    d = Diversity(vocab_of(12))
    with pytest.raises(ValueError, match="'okapi' is not a word"):
        d.update_payload(payload_of([["w4 w5", "w4 okapi"]]))
    for special in ("<start>", "<end>"):
        with pytest.raises(ValueError, match="is not a word"):
            d.update_payload(payload_of([["w4 w5", f"w4 {special}"]]))
    with pytest.raises(ValueError, match="differing numbers"):
        d.update_payload(payload_of([["w4", "w5"], ["w4", "w5", "w6"]]))
    with pytest.raises(ValueError, match="one caption"):
        d.update_payload({"predictions": [{"filename": "clip0", "caption": "w4", "tokens": "w4"}]})
    with pytest.raises(ValueError, match="2 <= N <= 16"):
        d.update_payload(payload_of([["w4"] * 17]))
    with pytest.raises(ValueError, match="65 words"):
        d.update_payload(payload_of([["w4", " ".join(["w5"] * 65)]]))
    d.sample_n = 3
    with pytest.raises(ValueError, match="share one N"):
        d.update_payload(payload_of([["w4", "w5"]]))
    d.reset()
    assert d.sample_n is None and d._records == [] and d._seen is None
    with pytest.raises(RuntimeError, match="no CPU fallback"):         # host rows are not counted on the host
        d.update(torch.zeros(6, 20, dtype=torch.long), 3)
    with pytest.raises(ValueError, match="clip-major"):
        d.update(torch.zeros(7, 20, dtype=torch.long), 3)
    assert d.sample_n is None and d._records == []                      # a refused update leaves no trace


def einval_cases(lib, p):
    """Every refusal of acvae_diversity_stats, with `p` a valid pointer for every array -> [(case, return code)]."""
    def call(**kw):
        a = dict(seqs=p, ld=20, n=10, sample_n=5, max_length=20, start_idx=1, end_idx=2, V=50, record=p, seen=p, stream=None)
        a.update(kw)
        return lib.acvae_diversity_stats(*a.values())
    cases = (dict(seqs=None), dict(record=None), dict(seen=None), dict(sample_n=1), dict(sample_n=0), dict(sample_n=17, n=34),
             dict(sample_n=-5), dict(n=0), dict(n=-5), dict(n=11), dict(n=4), dict(max_length=0), dict(max_length=65, ld=65),
             dict(max_length=-1), dict(ld=19), dict(V=0), dict(V=-1), dict(V=65535))
    return [(kw, call(**kw)) for kw in cases]


def test_entry_point_refuses_bad_arguments_before_any_launch():
    import torch
    from acvae_amd import _lib
    p = torch.zeros(64, dtype=torch.float64).data_ptr()            # host memory: every refusal comes before any launch
    for kw, rc in einval_cases(_lib.lib(), p):
        assert rc == -1, kw


def test_evaluate_refusals_that_need_no_device():
    import torch
    from acvae_amd import evaluate as EV
    from acvae_amd.decoder import VAERNNBahdanauAttnDecoder
    from acvae_amd.diversity import Diversity
    from acvae_amd.encoder import Cnn10
    from acvae_amd.vae_model import Hybrid_VAEModel
    V, E = 52, 64
    dec = VAERNNBahdanauAttnDecoder(vocab_size=V, enc_mem_size=E, embed_size=E, hidden_size=E, attn_size=E)
    model = Hybrid_VAEModel(Cnn10(64, 512), dec, posterior_model="PosteriorRNN_hybrid", posterior_args={"hidden_size": E},
                            prior_model="PriorRNN", prior_args={"hidden_size": E}).eval()
    vocab = vocab_of(V)
    d = Diversity(vocab)

    def items():                                                       # no refusal may come behind the first item
        raise AssertionError("evaluate touched the items before it refused")
        yield ("clip0", torch.zeros(64, 64))

    one = (dict(), dict(method="sample", beam_size=1), dict(method="beam", beam_size=3, finish_on_end=True),
           dict(method="beam", beam_size=3, finish_on_end=True, nbest=1), dict(method="dbs", beam_size=1, group_size=1),
           dict(method="dbs", beam_size=4, group_size=1, group_nbest=False))
    many = (dict(method="sample", beam_size=17), dict(method="greedy", beam_size=20),
            dict(method="dbs", beam_size=20, group_size=5), dict(method="dbs", beam_size=34, group_size=17, group_nbest=False))
    for kw in one + many:
        with pytest.raises(ValueError, match="2 <= N <= 16"):
            EV.evaluate(model, items(), vocab, diversity=d, **kw)
    with pytest.raises(ValueError, match="max_length=65"):
        EV.evaluate(model, items(), vocab, diversity=d, method="sample", beam_size=5, max_length=65)
    with pytest.raises(ValueError, match="must be an acvae_amd.diversity.Diversity"):
        EV.evaluate(model, items(), vocab, diversity="div", method="sample", beam_size=5)
    d.sample_n = 3
    with pytest.raises(ValueError, match="share one N"):
        EV.evaluate(model, items(), vocab, diversity=d, method="sample", beam_size=5)
    with pytest.raises(ValueError, match="share one N"):
        EV.evaluate(model, items(), vocab, diversity=d, method="dbs", beam_size=6, group_size=2)
    assert d._records == [] and d._seen is None
