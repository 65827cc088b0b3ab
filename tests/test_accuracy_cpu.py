"""CPU: the yardstick of the accuracy metrics (tests/accuracy_util.py) on hand-checked cases whose answer changes under each
plausible mistake, and the host side of acvae_amd/accuracy.py: the formulas of ``summarize`` on the yardstick's integers, the
reference tables, the constructor's, ``update``'s and ``update_payload``'s refusals, the argument checks of the entry point
(no launch without a GPU) and the refusals of ``evaluate(accuracy=)`` / ``ensemble_evaluate(accuracy=)`` that need no device."""
import numpy as np
import pytest

import accuracy_util as AU
from cider_util import SPECIALS, Vocabulary


def vocab_of(V):
    return Vocabulary(SPECIALS + [f"w{i}" for i in range(4, V)])


# ---- the yardstick, by hand
def test_hand_checked_rouge():
    s = AU.cand_stats("a b c d", ["a c d e f"])
    assert (s["lcs_p"], s["lcs_r"], s["len_r"], s["testlen"]) == (3, 3, 5, 4)        # a c d;  p = 3/4, r = 3/5
    p, r = 0.75, 0.6
    assert AU.rouge_l(s) == (1 + 1.44) * p * r / (r + 1.44 * p)
    assert s["correct"] == [3, 1, 0, 0] and s["guess"] == [4, 3, 2, 1] and s["reflen"] == 5
    assert AU.record_of(s) == [4, 5, 3, 1, 0, 0, 3, 3, 5]


def test_lcs_is_neither_the_common_substring_nor_the_unigram_overlap():
    s = AU.cand_stats("a b c d e", ["a x c e b"])
    assert s["lcs_p"] == 3 and s["substring"] == [1] and s["correct"][0] == 4        # a c e;  a;  a b c e
    assert AU.lcs("a b c b d a b".split(), "b d c a b a".split()) == 4               # the textbook pair: b c b a
    assert AU.lcs([], ["a"]) == 0 and AU.lcs(["a"], []) == 0


def test_clipping_takes_the_maximum_over_references_not_their_sum():
    s = AU.cand_stats("a a a", ["a", "a a"])
    by_sum = min(3, 1 + 2)
    assert s["correct"][0] == 2 != by_sum and s["clipped"] and s["correct"][1] == 1


def test_reference_length_is_the_closest_and_ties_go_to_the_shorter():
    assert AU.cand_stats("a b c d e", ["a b", "a b c d e f"])["reflen"] == 6         # not the shortest
    assert AU.cand_stats("a b c d", ["a b c", "a b c d e"])["reflen"] == 3           # |3 - 4| == |5 - 4|: the shorter
    assert AU.cand_stats("a b c d", ["a b c d e", "a b c"])["reflen"] == 3           # whatever their order
    longer = dict(AU.cand_stats("a b c d", ["a b c", "a b c d e"]), reflen=5)        # and the penalty sees it
    assert AU.corpus_bleu([longer])[0] < AU.corpus_bleu([AU.cand_stats("a b c d", ["a b c", "a b c d e"])])[0]


def test_precision_and_recall_may_come_from_different_references():
    s = AU.cand_stats("a b c d", ["a b c x y z w v", "a b"])
    assert s["lcs"] == [3, 2] and s["lcs_p"] == 3 and (s["lcs_r"], s["len_r"]) == (2, 2)     # 3/8 < 2/2
    # equal quotients: the earlier reference
    assert [AU.cand_stats("a b", refs)["len_r"] for refs in (["a x", "a b y z"], ["a b y z", "a x"])] == [2, 4]


def test_empty_candidate():
    s = AU.cand_stats("", ["a b c", "a"])
    assert AU.record_of(s) == [0, 1, 0, 0, 0, 0, 0, 0, 3] and AU.rouge_l(s) == 0.0 and s["guess"] == [0, 0, 0, 0]
    got = AU.accuracy([[""]], ["k"], {"k": ["a b c", "a"]}, cider=False)
    assert got["Bleu_1"] < 1e-9 and got["ROUGE_L"] == 0.0


def test_out_of_vocabulary_words_match_nothing():
    s = AU.cand_stats("w4 w5", ["okapi zebra"])                                       # a reference of unknown words only
    assert AU.record_of(s) == [2, 2, 0, 0, 0, 0, 0, 0, 2]
    s = AU.cand_stats("w4 <out> w5", ["w4 <out> w5"])                                 # <out> beside <out>: no match
    assert s["correct"] == [2, 0, 0, 0] and s["lcs_p"] == 2 and s["substring"] == [1]
    by_equality = 3
    assert s["correct"][0] != by_equality


def test_corpus_bleu_is_not_the_mean_of_sentence_bleu():
    key2refs = {"k0": ["a b c d e f"], "k1": ["c d"]}
    got = AU.accuracy([["a b c d e f"], ["a b"]], ["k0", "k1"], key2refs, cider=False)
    assert abs(got["Bleu_1"] - 6 / 8) <= 1e-9                                        # C_1 = 6 + 0 over G_1 = 6 + 2
    assert got["per_clip"]["ROUGE_L"] == [[1.0], [0.0]] and got["ROUGE_L"] == 0.5


# ---- the host side of acvae_amd/accuracy.py
KEY2REFS = {"k0": ["w4 w5 w6 w7", "w4 w4 w5 okapi w6"], "k1": ["w8 w9 w10 w11 w12 w13 w14"], "k2": ["w5", "w6 w5 w4", "zebra"],
            "k3": ["w4 w5 w6 w4 w5 w6 w4 w5 w6", "w7 w8"], "k4": ["w9 w8 w7 w6 w5 w4", "w4 w5 w6 w7 w8 w9", "w4 w6 w8"]}
CLIPS = [["w4 w5 w6", "w4 w4 w4 w5", ""], ["w8 w9 w10 w11 w12 w13 w14", "w8 w10 w12 w14", "w14 w13"], ["w5", "w4 w5 w6", ""],
         ["w4 w5 w6 w4 w5 w6", "w7", "w8 w7"], ["w4 w5 w6 w7 w8 w9", "w9 w8 w4 w5 w6", "w4 w4 w6 w6 w8 w8"]]


def test_summarize_evaluates_the_formulas_on_the_integers():
    from acvae_amd.accuracy import RECORD, summarize
    assert RECORD == 9
    keys = list(KEY2REFS)
    want = AU.accuracy(CLIPS, keys, KEY2REFS)
    record = np.array([AU.record_of(s) for clip in want["stats"] for s in clip], dtype=np.int32)
    cider = np.array(want["per_clip"]["CIDEr"], dtype=np.float64).reshape(-1)
    got = summarize(record, cider, 3)
    names = ("Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L", "CIDEr")
    for key in names:
        assert abs(got[key] - want[key]) <= AU.bound(want[key]), (key, got[key], want[key])
        assert np.all(np.abs(np.array(got["per_index"][key]) - np.array(want["per_index"][key])) <= 1e-12), key
    for key in ("ROUGE_L", "CIDEr"):
        assert got["per_clip"][key].shape == (5, 3) and got["per_clip"][key].dtype == np.float64
        assert np.all(np.abs(got["per_clip"][key] - np.array(want["per_clip"][key])) <= 1e-12)
    assert got["clips"] == 5 and got["sample_n"] == 3 and want["CIDEr"] > 0 and 0 < want["Bleu_4"] < want["Bleu_1"] < 1
    assert set(got) == set(names) | {"clips", "sample_n", "per_index", "per_clip"}
    one = summarize(record[::3], cider[::3], 1)                                      # N = 1: the plain corpus scores
    first = AU.accuracy([c[:1] for c in CLIPS], keys, KEY2REFS)
    assert all(abs(one[k] - first[k]) <= AU.bound(first[k]) and one[k] == one["per_index"][k][0] for k in names)


def test_summarize_rouge_is_zero_without_a_common_word_or_without_words():
    from acvae_amd.accuracy import summarize
    got = summarize(np.array([[0, 3, 0, 0, 0, 0, 0, 0, 3], [2, 2, 0, 0, 0, 0, 0, 0, 2], [4, 5, 3, 1, 0, 0, 3, 3, 5]]),
                    np.zeros(3), 1)
    assert got["per_clip"]["ROUGE_L"][:, 0].tolist() == [0.0, 0.0, (1 + 1.44) * 0.75 * 0.6 / (0.6 + 1.44 * 0.75)]


def test_reference_tables():
    from acvae_amd.accuracy import OOV, Accuracy
    a = Accuracy(vocab_of(20), KEY2REFS)
    words, ref_off, clip_ref = a.reference_tables(["k2", "k0"])
    assert words.dtype == ref_off.dtype == clip_ref.dtype == np.int32 and OOV == -1
    assert words.tolist() == [5, 6, 5, 4, -1, 4, 5, 6, 7, 4, 4, 5, -1, 6]
    assert ref_off.tolist() == [0, 1, 4, 5, 9, 14] and clip_ref.tolist() == [0, 3, 5]


def test_constructor_refusals():
    from acvae_amd.accuracy import MAX_VOCAB, Accuracy
    refs = {"k": ["w4 w5"]}
    with pytest.raises(ValueError, match="share the word"):
        Accuracy(Vocabulary(SPECIALS + ["cat", "dog", "cat"]), refs)
    for bad in ("two words", "", "tab\there", " lead"):
        with pytest.raises(ValueError, match="whitespace"):
            Accuracy(Vocabulary(SPECIALS + [bad]), refs)
    with pytest.raises(ValueError, match="16 bits"):
        Accuracy(Vocabulary(SPECIALS + [f"w{i}" for i in range(4, MAX_VOCAB + 1)]), refs)
    a = Accuracy(Vocabulary(SPECIALS + [f"w{i}" for i in range(4, MAX_VOCAB)]), refs)
    assert a.V == MAX_VOCAB == 65534 and (a.start_idx, a.end_idx) == (1, 2)
    with pytest.raises(ValueError, match="no <end>"):
        Accuracy(Vocabulary(["<pad>", "<start>", "cat"]), refs)
    with pytest.raises(ValueError, match="no <start>"):
        Accuracy(Vocabulary(["<pad>", "<end>", "cat"]), refs)
    with pytest.raises(ValueError, match="'k1' has no references"):
        Accuracy(vocab_of(12), {"k0": ["w4"], "k1": []})
    for empty in ("", "  \t "):
        with pytest.raises(ValueError, match="a reference without words"):
            Accuracy(vocab_of(12), {"k0": ["w4", empty]})

    class ListVocabulary:
        idx2word = ["<end>", "cat", "<start>"]
    a = Accuracy(ListVocabulary(), {"k": ["cat dog"]})
    assert (a.start_idx, a.end_idx, a.V) == (2, 0, 3)                   # the indices are the vocabulary's
    with pytest.raises(ValueError, match="without an update"):
        a.result()
    for n in (0, -1, 17, True, 2.0):
        with pytest.raises(ValueError, match="1 <= N <= 16"):
            a.check(n)
    assert a.check(1) == 1 and a.check(np.int64(16)) == 16 and a.sample_n is None


def payload_of(clips, keys):
    return {"predictions": [{"filename": k, "captions": [{"caption": c, "cap_id": i, "tokens": c} for i, c in enumerate(caps)]}
                            if len(caps) > 1 else {"filename": k, "caption": caps[0], "tokens": caps[0]}
                            for k, caps in zip(keys, clips)]}


def untouched(a):
    return a.sample_n is None and a.width is None and a._rows == [] and a._keys == [] and a._seen == set()


def test_update_refusals():
    import torch
    from acvae_amd.accuracy import Accuracy
    a = Accuracy(vocab_of(20), KEY2REFS)
    rows = torch.zeros(6, 20, dtype=torch.long)
    with pytest.raises(ValueError, match="'nokey' has no references"):
        a.update(["k0", "nokey"], rows, 3)
    with pytest.raises(ValueError, match="'k0' seen twice"):
        a.update(["k0", "k0"], rows, 3)
    with pytest.raises(ValueError, match="clip-major"):
        a.update(["k0", "k1"], rows, 2)
    with pytest.raises(ValueError, match="clip-major"):
        a.update(["k0", "k1"], rows[0], 3)
    with pytest.raises(ValueError, match="rows of 65 tokens"):
        a.update(["k0", "k1"], torch.zeros(2, 65, dtype=torch.long))
    with pytest.raises(ValueError, match="1 <= N <= 16"):
        a.update(["k0"], torch.zeros(17, 20, dtype=torch.long), 17)
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # host rows are not scored on the host
        a.update(["k0", "k1"], rows, 3)
    assert untouched(a)                                                  # a refused update leaves no trace
    a.sample_n, a.width, a._seen = 3, 20, {"k4"}
    with pytest.raises(ValueError, match="share one N"):
        a.update(["k0", "k1"], rows, 2)
    with pytest.raises(ValueError, match="share one row width"):
        a.update(["k0", "k1"], torch.zeros(6, 12, dtype=torch.long), 3)
    with pytest.raises(ValueError, match="'k4' seen twice"):
        a.update(["k0", "k4"], rows, 3)
    a.reset()
    assert untouched(a)


def test_update_payload_refusals():
    from acvae_amd.accuracy import Accuracy
    a = Accuracy(vocab_of(20), KEY2REFS)
    with pytest.raises(ValueError, match="'okapi' is not a word"):
        a.update_payload(payload_of([["w4 w5", "w4 okapi"]], ["k0"]))
    for special in ("<start>", "<end>"):
        with pytest.raises(ValueError, match="is not a word"):
            a.update_payload(payload_of([[f"w4 {special}"]], ["k0"]))
    with pytest.raises(ValueError, match="differing numbers"):
        a.update_payload(payload_of([["w4", "w5"], ["w4", "w5", "w6"]], ["k0", "k1"]))
    with pytest.raises(ValueError, match="1 <= N <= 16"):
        a.update_payload(payload_of([["w4"] * 17], ["k0"]))
    with pytest.raises(ValueError, match="65 words"):
        a.update_payload(payload_of([[" ".join(["w5"] * 65)]], ["k0"]))
    a.sample_n = 3
    with pytest.raises(ValueError, match="share one N"):
        a.update_payload(payload_of([["w4", "w5"]], ["k0"]))
    a.reset()
    a.width = 3
    with pytest.raises(ValueError, match="4 words after updates with rows of 3"):
        a.update_payload(payload_of([["w4 w5 w6 w7"]], ["k0"]))
    a.reset()
    assert untouched(a)


def einval_cases(lib, p):
    """Every refusal of acvae_accuracy_stats, with `p` a valid pointer for every array -> [(case, return code)]."""
    def call(**kw):
        a = dict(seqs=p, ld=20, n=10, sample_n=5, max_length=20, start_idx=1, end_idx=2, V=50, ref_words=p, n_words=12,
                 ref_off=p, n_refs=4, clip_ref=p, n_clips=2, record=p, stream=None)
        a.update(kw)
        return lib.acvae_accuracy_stats(*a.values())
    cases = (dict(seqs=None), dict(ref_words=None), dict(ref_off=None), dict(clip_ref=None), dict(record=None),
             dict(sample_n=0), dict(sample_n=17, n=34), dict(sample_n=-5), dict(n=0, n_clips=0), dict(n=-5, n_clips=-1),
             dict(n=11), dict(n=4), dict(max_length=0), dict(max_length=65, ld=65), dict(max_length=-1), dict(ld=19),
             dict(V=0), dict(V=-1), dict(V=65535), dict(n_clips=1), dict(n_clips=3), dict(n_clips=10), dict(n_words=-1),
             dict(n_refs=-1), dict(n_words=2 ** 30 + 1))
    return [(kw, call(**kw)) for kw in cases]


def test_entry_point_refuses_bad_arguments_before_any_launch():
    import torch
    from acvae_amd import _lib
    p = torch.zeros(64, dtype=torch.float64).data_ptr()            # host memory: every refusal comes before any launch
    for kw, rc in einval_cases(_lib.lib(), p):
        assert rc == -1, kw
    assert int(_lib._defs["ACVAE_ABI_VERSION"]) == 3 == _lib.lib().acvae_abi_version()


def test_evaluate_refusals_that_need_no_device():
    import torch
    from acvae_amd import evaluate as EV
    from acvae_amd.accuracy import Accuracy
    from acvae_amd.decoder import VAERNNBahdanauAttnDecoder
    from acvae_amd.encoder import Cnn10
    from acvae_amd.ensemble import ensemble_evaluate
    from acvae_amd.vae_model import Hybrid_VAEModel
    V, E = 52, 64
    dec = VAERNNBahdanauAttnDecoder(vocab_size=V, enc_mem_size=E, embed_size=E, hidden_size=E, attn_size=E)
    model = Hybrid_VAEModel(Cnn10(64, 512), dec, posterior_model="PosteriorRNN_hybrid", posterior_args={"hidden_size": E},
                            prior_model="PriorRNN", prior_args={"hidden_size": E}).eval()
    vocab = vocab_of(V)
    a = Accuracy(vocab, {"clip0": ["w4 w5"]})

    def items():                                                       # no refusal may come behind the first item
        raise AssertionError("evaluate touched the items before it refused")
        yield ("clip0", torch.zeros(64, 64))

    many = (dict(method="sample", beam_size=17), dict(method="greedy", beam_size=20),
            dict(method="dbs", beam_size=20, group_size=5), dict(method="dbs", beam_size=34, group_size=17, group_nbest=False),
            dict(method="beam", beam_size=20, finish_on_end=True, nbest=17))
    for kw in many:
        with pytest.raises(ValueError, match="1 <= N <= 16"):
            EV.evaluate(model, items(), vocab, accuracy=a, **kw)
    for kw in many[2:]:
        with pytest.raises(ValueError, match="1 <= N <= 16"):
            ensemble_evaluate([model], items(), vocab, accuracy=a, **kw)
    for run in (lambda **kw: EV.evaluate(model, items(), vocab, **kw),
                lambda **kw: ensemble_evaluate([model], items(), vocab, **kw)):
        with pytest.raises(ValueError, match="max_length=65"):
            run(accuracy=a, method="greedy", beam_size=1, max_length=65)
        with pytest.raises(ValueError, match="must be an acvae_amd.accuracy.Accuracy"):
            run(accuracy="acc", method="greedy", beam_size=1)
        with pytest.raises(ValueError, match="zh=True"):
            run(accuracy=a, zh=True, method="greedy", beam_size=1)
    a.sample_n, a.width = 3, 20
    with pytest.raises(ValueError, match="share one N"):
        EV.evaluate(model, items(), vocab, accuracy=a, method="sample", beam_size=5, max_length=20)
    with pytest.raises(ValueError, match="share one N"):
        EV.evaluate(model, items(), vocab, accuracy=a, method="greedy", max_length=20)
    with pytest.raises(ValueError, match="share one N"):
        ensemble_evaluate([model], items(), vocab, accuracy=a, method="dbs", beam_size=6, group_size=2)
    with pytest.raises(ValueError, match="share one row width"):
        EV.evaluate(model, items(), vocab, accuracy=a, method="sample", beam_size=3, max_length=12)
    assert a._rows == [] and a._keys == []
