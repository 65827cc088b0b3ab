"""CPU: the host side of the device CIDEr-D scorer (acvae_amd/cider.py).  CiderD.prepare() builds everything that depends on
the references; here a few lines of numpy evaluate the definition from those tables ALONE (what the kernel does, on the
host, in the test - the package keeps no CPU twin) and must match the dictionary yardstick of tests/cider_util.py to
1e-12 * max(1, |score|).  Also the yardstick's own closed-form anchors, the constructor's refusals and the argument checks
of the two entry points (no launch without a GPU)."""
import numpy as np
import pytest

import cider_util as CU
from cider_util import SPECIALS, DictCiderD, Vocabulary

START, END = 1, 2


def vocab_of(V):
    return Vocabulary(SPECIALS + [f"w{i}" for i in range(4, V)])


def evaluate_tables(tab, seqs):
    """The definition from prepare()'s tables: token rows [n, T] -> float64 scores [n]."""
    h = tab.host
    seqs = np.asarray(seqs)
    out = np.zeros(len(seqs))
    for i in range(len(seqs)):
        words = []
        for w in seqs[int(h["row_src"][i])]:
            if w == START:
                continue
            if w == END:
                break
            words.append(int(w))
        vh, nh = [], []
        for k in range(1, 5):
            counts = {}
            for p in range(len(words) - k + 1):
                key = sum((words[p + j] + 1) << (16 * j) for j in range(k))
                counts[key] = counts.get(key, 0) + 1
            vec = {}
            for key, tf in counts.items():
                at = np.searchsorted(h["idf_keys"], np.uint64(key))
                hit = at < h["idf_keys"].size and int(h["idf_keys"][at]) == key
                vec[key] = tf * (float(h["idf_vals"][at]) if hit else tab.log_d)
            vh.append(vec)
            nh.append(np.sqrt(sum(v * v for v in vec.values())))
        lh = max(len(words) - 1, 0)
        d = int(h["row_doc"][i])
        refs = range(int(h["doc_ref"][d]), int(h["doc_ref"][d + 1]))
        total = np.zeros(4)
        for r in refs:
            lo, hi = int(h["ref_off"][r]), int(h["ref_off"][r + 1])
            rk, rw = h["ref_keys"][lo:hi], h["ref_w"][lo:hi]
            assert np.all(rk[1:] > rk[:-1])                       # ascending: the kernel searches by bisection
            ref = dict(zip((int(x) for x in rk), rw))
            for k in range(4):
                s = sum(min(v, ref.get(key, 0.0)) * ref.get(key, 0.0) for key, v in vh[k].items())
                if nh[k] != 0 and h["ref_norm"][r, k] != 0:
                    s /= nh[k] * h["ref_norm"][r, k]
                total[k] += s * h["len_factor"][abs(lh - int(h["ref_len"][r]))]
        out[i] = total.mean() / len(refs) * 10.0
    return out


def random_text(V, n_keys, seed, oov=False):
    rng = np.random.default_rng(seed)
    vocab = vocab_of(V)
    pool = [vocab.idx2word[i] for i in range(3, V)] + (["zebra", "quagga", "okapi"] if oov else [])
    keys = [f"clip{i}" for i in range(n_keys)]
    key2refs = {}
    for j, k in enumerate(keys):
        nref = 1 + (j + seed) % 5                                  # 1-5 references per key, ragged
        key2refs[k] = [" ".join(pool[int(x)] for x in rng.integers(0, min(len(pool), 12 + 3 * j), rng.integers(1, 14)))
                       for _ in range(nref)]
    return vocab, keys, key2refs


def random_rows(V, n, T, seed, key2refs=None, keys=None, vocab=None):
    rng = np.random.default_rng(seed + 100)
    seqs = rng.integers(0, min(V, 16), (n, T))
    if key2refs is not None:                                        # some rows that share n-grams with their references
        w2i = {w: i for i, w in vocab.idx2word.items()}
        for i in range(0, n, 2):
            ids = [w2i[w] for w in key2refs[keys[i]][0].split() if w in w2i][:T - 1]
            seqs[i, :len(ids)] = ids
            seqs[i, len(ids)] = END
    return seqs


def check(cd, vocab, keys, key2refs, seqs, mode):
    tab = cd.prepare(keys, key2refs, mode)
    got = evaluate_tables(tab, seqs)
    want = CU.row_scores(seqs, keys, key2refs, vocab, mode)
    err = np.abs(got - want)
    print(f"{mode}: {len(keys)} rows, D = {tab.n_docs}, upload {tab.nbytes} B, scores {want.min():.3f} .. {want.max():.3f}, "
          f"worst |d| / bound {float((err / CU.bound(want)).max()):.3g}")
    assert np.all(err <= CU.bound(want)), (got, want)
    return tab, want


# ---------------------------------------------------------------- the yardstick's own anchors
def test_yardstick_anchors():
    gts = {"a": ["the dog barks at the cat"], "b": ["rain falls on a tin roof"]}
    same = CU.ciderd(gts, {"a": ["the dog barks at the cat"], "b": ["rain falls on a tin roof"]})[1]
    assert np.all(np.abs(same - 10.0) <= 1e-12 * 10) and CU.ciderd(gts, {"a": ["x y z w"], "b": ["q"]})[1].tolist() == [0.0, 0.0]
    assert CU.ciderd({"a": gts["a"]}, {"a": gts["a"]})[1].tolist() == [0.0]               # D = 1: ln D = 0
    short = CU.ciderd(gts, {"a": ["the dog barks"], "b": [""]})[1]
    assert 0.0 < short[0] < 10.0 and short[1] == 0.0
    mean, per_key = DictCiderD().compute_score(gts, {"a": ["the dog barks"], "b": [""]})     # the scorer-object form
    assert np.array_equal(per_key, short) and mean == short.mean()
    import acvae_amd.cider  # noqa: F401  (the feature under test: these tests are about it)


def test_yardstick_against_pycocoevalcap():
    cider = pytest.importorskip("pycocoevalcap.cider.cider")
    import acvae_amd.cider  # noqa: F401
    vocab, keys, key2refs = random_text(50, 6, 3)
    res = {k: [key2refs[k][0]] for k in keys}
    want = cider.Cider().compute_score(key2refs, res)[1]
    got = CU.ciderd(key2refs, res)[1]
    assert np.all(np.abs(got - want) <= CU.bound(want))


# ---------------------------------------------------------------- prepare()'s tables against the yardstick
@pytest.mark.parametrize("mode", ["batch", "rows"])
@pytest.mark.parametrize("V,n_keys,T", [(50, 7, 20), (5000, 32, 30), (50, 2, 20)])
def test_tables_reproduce_the_definition(mode, V, n_keys, T):
    from acvae_amd.cider import CiderD
    vocab, keys, key2refs = random_text(V, n_keys, seed=n_keys, oov=True)
    if mode == "rows":
        keys = [k for k in keys for _ in range(3)]
    else:
        keys = keys + keys[:2] + keys[-1:]                          # duplicate keys: scored by the first row with the key
    seqs = random_rows(V, len(keys), T, n_keys, key2refs, keys, vocab)
    cd = CiderD(vocab)
    tab, want = check(cd, vocab, keys, key2refs, seqs, mode)
    assert float(want.max()) > 0
    if mode == "batch":
        assert tab.n_docs == n_keys and np.array_equal(want[n_keys:n_keys + 2], want[:2]) and want[-1] == want[n_keys - 1]
    else:
        assert tab.n_docs == len(keys)
    # the second batch is served from the cooked references and gives the same tables
    tab2 = cd.prepare(keys, key2refs, mode)
    assert all(np.array_equal(tab.host[k], tab2.host[k]) for k in tab.host)


def test_out_of_vocabulary_reference_words_keep_their_identity():
    """Two different unknown words in the same position of two references are two n-grams: both count in df and in the norms,
    neither matches a hypothesis' <unk>."""
    from acvae_amd.cider import CiderD
    vocab = vocab_of(50)
    key2refs = {"a": ["w4 zebra w6 w7 w8", "w4 quagga w6 w7 w8", "w4 <unk> w6 w7 w8"], "b": ["w9 w10 zebra w11"],
                "c": ["w12 w13 w14 w15 w16"]}
    keys = ["a", "b", "c"]
    seqs = np.array([[4, 3, 6, 7, 8, END, 0, 0], [9, 10, 3, 11, END, 0, 0, 0], [12, 13, 14, 15, 16, END, 0, 0]])
    for mode in ("batch", "rows"):
        tab, want = check(CiderD(vocab), vocab, keys, key2refs, seqs, mode)
        assert want[2] == pytest.approx(10.0, abs=1e-11) and 0 < want[0] < 10 and 0 < want[1] < 10
        # the unknown words have no device entry: reference "w9 w10 zebra w11" keeps 3 unigrams and 1 bigram out of 10 n-grams
        assert int(tab.host["ref_off"][4] - tab.host["ref_off"][3]) == 4
    merged = dict(key2refs, a=["w4 zebra w6 w7 w8", "w4 zebra w6 w7 w8", "w4 <unk> w6 w7 w8"])
    assert not np.allclose(CU.row_scores(seqs, keys, merged, vocab, "batch"), want)


def test_idf_zero_one_document_and_empty_hypotheses():
    from acvae_amd.cider import CiderD
    vocab = vocab_of(50)
    # every document's references hold "w5 w6": df = D, idf = 0 for that bigram and its words
    key2refs = {"a": ["w5 w6 w7", "w8 w5 w6"], "b": ["w5 w6 w9 w10"], "c": ["w11 w5 w6"]}
    keys = ["a", "b", "c"]
    seqs = np.array([[5, 6, 7, END], [5, 6, END, 0], [END, 5, 6, 11]])
    tab, want = check(CiderD(vocab), vocab, keys, key2refs, seqs, "batch")
    at = np.searchsorted(tab.host["idf_keys"], np.uint64((5 + 1) | ((6 + 1) << 16)))
    assert tab.host["idf_vals"][at] == 0.0 and want[1] == 0.0 and want[2] == 0.0 and want[0] > 0
    # D = 1: ln D = 0 and every score 0
    tab, want = check(CiderD(vocab), vocab, ["a"], key2refs, seqs[:1], "batch")
    assert tab.log_d == 0.0 and want.tolist() == [0.0]
    # ... but one key in three rows is three documents in "rows" mode
    tab, want = check(CiderD(vocab), vocab, ["a"] * 3, key2refs, np.repeat(seqs[:1], 3, 0), "rows")
    assert tab.n_docs == 3 and want.tolist() == [0.0] * 3          # (every n-gram is in all three documents)
    # <start> in mid-row, no <end>, one repeated word, <pad> and <unk> as words
    seqs = np.array([[5, START, 6, 7, 7, 7], [0, 3, 5, 6, 9, 10], [7, 7, 7, 7, 7, 7]])
    check(CiderD(vocab), vocab, keys, key2refs, seqs, "batch")


def test_constructor_refusals():
    from acvae_amd.cider import MAX_VOCAB, CiderD
    with pytest.raises(ValueError, match="share the word"):
        CiderD(Vocabulary(SPECIALS + ["cat", "dog", "cat"]))
    for bad in ("two words", "", "tab\there", " lead"):
        with pytest.raises(ValueError, match="whitespace"):
            CiderD(Vocabulary(SPECIALS + [bad]))
    with pytest.raises(ValueError, match="16 bits"):
        CiderD(Vocabulary([f"w{i}" for i in range(MAX_VOCAB + 1)]))
    CiderD(Vocabulary([f"w{i}" for i in range(MAX_VOCAB)]))
    with pytest.raises(ValueError, match="no references"):
        CiderD(vocab_of(10)).prepare(["a"], {"a": []})
    with pytest.raises(ValueError, match="mode"):
        CiderD(vocab_of(10)).prepare(["a"], {"a": ["w4"]}, mode="corpus")
    class ListVocabulary:
        idx2word = SPECIALS + ["cat"]
    assert CiderD(ListVocabulary()).word2id["cat"] == 4


def test_entry_points_refuse_bad_arguments_before_any_launch():
    import torch
    from acvae_amd import _lib
    from acvae_amd.cider import MAX_LENGTH
    lib = _lib.lib()
    assert lib.acvae_abi_version() == 3 and MAX_LENGTH == 64
    p = torch.zeros(64, dtype=torch.float64).data_ptr()            # host memory: every refusal comes before any launch

    def scores(**kw):
        a = dict(seqs0=p, seqs1=None, ld=20, n=4, n_sets=1, max_length=20, start_idx=1, end_idx=2, idf_keys=p, idf_vals=p,
                 n_idf=3, log_d=1.0, ref_keys=p, ref_w=p, n_entries=3, ref_off=p, ref_norm=p, ref_len=p, n_refs=2, doc_ref=p,
                 n_docs=2, row_doc=p, row_src=p, len_factor=p, n_len=64, score=p, stream=None)
        a.update(kw)
        return lib.acvae_ciderd_scores(*a.values())
    for kw in (dict(seqs0=None), dict(n=0), dict(n_sets=2), dict(n_sets=3), dict(max_length=0), dict(max_length=65, ld=65),
               dict(ld=19), dict(n_idf=-1), dict(idf_vals=None), dict(n_entries=-1), dict(ref_keys=None), dict(ref_off=None),
               dict(ref_norm=None), dict(ref_len=None), dict(n_refs=0), dict(doc_ref=None), dict(n_docs=0), dict(row_doc=None),
               dict(row_src=None), dict(len_factor=None), dict(n_len=0), dict(score=None)):
        assert scores(**kw) == -1, kw
    assert lib.acvae_ciderd_reward(None, 4, 1, p, p, None) == -1
    assert lib.acvae_ciderd_reward(p, 4, 1, None, p, None) == -1
    assert lib.acvae_ciderd_reward(p, 0, 1, p, p, None) == -1
    assert lib.acvae_ciderd_reward(p, 7, 5, p, p, None) == -1     # rows not a multiple of sample_n


def test_scorer_none_still_raises_and_names_the_package_scorer():
    from acvae_amd import train_util
    with pytest.raises(ValueError, match="acvae_amd.cider.CiderD"):
        train_util._need_scorer(None)
