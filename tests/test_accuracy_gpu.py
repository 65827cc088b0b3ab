"""GPU: captions against references on the device (acvae_accuracy_stats, acvae_amd/accuracy.py), ``evaluate(accuracy=)`` and
``ensemble_evaluate(accuracy=)``.

The kernel through the C ABI against the string yardstick of tests/accuracy_util.py on the rows read back: every integer of
every record equal.  T 1 / 2 / 3 / 4 / 5 / 20 / 63 / 64 and N 1 / 2 / 5 / 16 (all 32 pairs), B 1 / 3 / 33 clips, at most
R 1 / 2 / 5 / 17 references per clip (ragged within a call: clip 0 has R, every other clip 1 .. R), vocabularies of 7, 5000
and 65534 words; reference lengths anywhere in 1 .. 63 and, planted in every call that has the slots, 64, 65, 130, 63 and 1
(both sides of one and of two 64-word steps); ld > T with garbage in the padding; garbage ids in the rows; reference words
outside the vocabulary (-1, and ids >= V); rows, references and records between guard words that are checked.  The twelve
(B, R, V) triples of TRIPLES hold every pairing of B, R and V; the (N, T) pairs take them in turn, the costliest pairs the
cheapest triples (the yardstick's LCS table is quadratic, in Python) and the eight cheapest pairs the costliest triples.

The random cases do not pass vacuously; asserted on the yardstick's numbers, per case (``vacuity``):
  - clipping is active (c_h(g) > max_r c_r(g) for some g) in at least one row: every case;
  - at least half of the rows have 0 < LCS(h, r) < min(L, len r) for some reference r and correct_2 > 0: T >= 4 (a shared
    bigram needs two kept words, which T <= 3 leaves no room for beside the planted <end>, <start> and out-of-range words);
  - for at least one row and reference, LCS(h, r) differs from both the longest common substring and the clipped unigram
    count of h against r: T >= 4;
  - with the 7-word vocabulary at least one row has a reference count above 1 for an n-gram of each order: T >= 20.
The seeds are 1000 N + 10 T + B, but for the cases of SEEDS whose yardstick numbers miss a condition at that seed."""
import numpy as np
import pytest
import torch

import accuracy_util as AU
import cider_util as CU
from acvae_amd import _lib
from acvae_amd import evaluate as EV
from cider_util import Vocabulary
from test_accuracy_cpu import einval_cases

pytestmark = pytest.mark.gpu
START, END = 1, 2
REC = 9                                                            # include/acvae_hip.h
GARBAGE = [-1, -(2 ** 62), 2 ** 40 + 5, 2 ** 63 - 1, START, END, 4, -7]
NS, TS, BS, RS, VS = (1, 2, 5, 16), (1, 2, 3, 4, 5, 20, 63, 64), (1, 3, 33), (1, 2, 5, 17), (7, 5000, 65534)
PLANTED = (64, 65, 130, 63, 1)
TRIPLES = sorted(((B, R, VS[(i + j) % 3]) for i, B in enumerate(BS) for j, R in enumerate(RS)), key=lambda t: t[0] * t[1])
PAIRS = sorted(((N, T) for N in NS for T in TS), key=lambda p: -p[0] * p[1])
SEEDS = {(5, 5): 44205051, (16, 1): 116011, (1, 4): 401073, (2, 2): 102023, (1, 2): 24201021, (2, 1): 302013}    # by (N, T)


def case_of(N, T):
    """The (N, T) pair's triple and seed -> (B, R, V, seed)."""
    at = PAIRS.index((N, T))
    B, R, V = TRIPLES[at % 12 if at < 24 else 35 - at]
    return B, R, V, SEEDS.get((N, T), 1000 * N + 10 * T + B)


def test_the_triples_hold_every_pairing():
    used = {case_of(N, T)[:3] for N, T in PAIRS}
    assert used == set(TRIPLES) and len(used) == 12
    assert {(B, R) for B, R, V in used} == {(B, R) for B in BS for R in RS}
    assert {(B, V) for B, R, V in used} == {(B, V) for B in BS for V in VS}
    assert {(R, V) for B, R, V in used} == {(R, V) for R in RS for V in VS}


def random_case(B, N, T, V, R, seed, clean=False):
    """-> (rows [B * N, T], refs: per clip a list of word-id lists).  Rows over five words per clip (id V - 1 among them), so
    that candidates and references share n-grams and repeat their own; lengths mostly in the upper half of T; <start> and
    ids outside [0, V) sprinkled in (not with ``clean``); <end> where the row is shorter than T and garbage behind it.
    References: clip 0 has R of them, the others 1 .. R; each is a candidate's words (mostly candidate 0's) with at least one
    substitution, with deletions and insertions, brought to a length near the candidate's or anywhere in 1 .. 63; the
    first references of the call get the PLANTED lengths; a few words are outside the vocabulary (-1, or V + 5 and more)."""
    rng = np.random.default_rng(seed)
    ids = np.array([i for i in range(V) if i not in (START, END)])
    seqs = np.empty((B * N, T), dtype=np.int64)
    refs, slot = [], 0
    for b in range(B):
        pool = np.concatenate([[V - 1], rng.choice(ids, 4, replace=False)])
        kept = []
        for i in range(N):
            row = seqs[b * N + i]
            low = (T + 1) // 2 if T > 5 else max(T - 1, 1)          # (a short row has no room for a bigram beside a mismatch)
            length = int(rng.integers(0, T + 1)) if rng.random() < 0.15 else int(rng.integers(low, T + 1))
            length = max(length, 1) if b == i == 0 else length
            row[:length] = rng.choice(pool, length)
            if i > 0 and rng.random() < 0.7:
                h = int(rng.integers(1, T + 1))
                row[:min(h, length)] = seqs[b * N, :min(h, length)]
            if not clean:
                spots = rng.random(length)
                row[:length][spots < 0.03] = START
                row[:length][spots > 0.98] = [V, 2 ** 40, -3][int(rng.integers(3))]
            if b == i == 0:
                row[0] = V - 1                             # the largest id is in every case
            if length < T:
                row[length] = END
                row[length + 1:] = rng.choice(GARBAGE, T - length - 1)
            kept.append([int(w) for w in row[:length] if 0 <= w < V and w not in (START, END)])
        mine = []
        for j in range(R if b == 0 else int(rng.integers(1, R + 1))):
            base = kept[0] if rng.random() < 0.6 else kept[int(rng.integers(N))]
            words = list(base)
            for at in rng.choice(len(words), min(len(words), max(1, int(rng.binomial(len(words), 0.15)))), replace=False):
                words[at] = int(rng.choice([w for w in pool if w != words[at]]))      # at least one other word
            words = [w for w in words if rng.random() >= 0.08]
            for at in sorted(np.flatnonzero(rng.random(len(words) + 1) < 0.08), reverse=True):
                words.insert(at, int(rng.choice(pool)))
            if slot < len(PLANTED):
                want = PLANTED[slot]
                slot += 1
            elif rng.random() < 0.6:
                want = max(1, len(base) + int(rng.integers(-1, 3) if T <= 5 else rng.integers(-3, 4)))
            else:
                want = int(rng.integers(1, 64))
            while len(words) < want:
                at = int(rng.integers(0, len(words) + 1))
                words[at:at] = [int(w) for w in rng.choice(pool, min(3, want - len(words)))]
            words = words[:want]
            for at in np.flatnonzero(rng.random(want) < 0.03):
                words[at] = -1 if clean or rng.random() < 0.5 else V + 5 + int(rng.integers(3))
            mine.append(words)
        refs.append(mine)
    return seqs, refs


def reference_strings(refs, V):
    """Word-id lists -> the yardstick's strings: -1 the unknown word "oov", an id >= V the word "<out>" (which the
    yardstick matches with no candidate word, the candidate's own "<out>" included)."""
    return [[" ".join("oov" if w < 0 else AU.OUT if w >= V else f"w{w}" for w in r) for r in clip] for clip in refs]


def vacuity(stats, T, V):
    """The conditions of the module docstring on the yardstick's statistics -> the list of those missed."""
    rows = [s for clip in stats for s in clip]
    missed = []
    if not any(s["clipped"] for s in rows):
        missed.append("no clipping")
    if T >= 4:
        good = sum(1 for s in rows if s["correct"][1] > 0 and
                   any(0 < x < min(s["testlen"], n) for x, n in zip(s["lcs"], s["reflens"])))
        if 2 * good < len(rows):
            missed.append(f"0 < LCS < min(L, len r) and correct_2 > 0 in {good} of {len(rows)} rows")
        if not any(x != sub and x != uni for s in rows for x, sub, uni in zip(s["lcs"], s["substring"], s["unigrams"])):
            missed.append("the LCS is the common substring or the unigram overlap everywhere")
    if V == 7 and T >= 20 and not any(min(s["most"]) > 1 for s in rows):
        missed.append("no row with a reference count above 1 in every order")
    return missed


def yardstick(seqs, refs, N, V):
    clips = AU.clips_of_rows(seqs, N, V)
    strings = reference_strings(refs, V)
    return [[AU.cand_stats(h, r) for h in clip] for clip, r in zip(clips, strings)]


def guarded(values, dtype, guard, fill):
    """`values` on the device between `guard` words of `fill` on either side -> (the whole buffer, the view between)."""
    host = np.concatenate([np.full(guard, fill, dtype=dtype), np.asarray(values, dtype=dtype), np.full(guard, fill, dtype=dtype)])
    dev = torch.from_numpy(host).cuda()
    return dev, dev[guard:guard + len(values)], host


def launch(seqs, refs, N, V):
    """acvae_accuracy_stats on token rows [B * N, T], uploaded with ld = T + 3 (garbage in the padding), the references in
    the entry's three arrays, every array between guard words that a read outside would pick up (a word of the
    vocabulary; offsets that lead elsewhere) -> the records [B * N][9].  Guards and inputs are checked to be as they were."""
    seqs = np.ascontiguousarray(seqs, dtype=np.int64)
    n, T = seqs.shape
    wide = np.full((n + 2, T + 3), -(2 ** 50), dtype=np.int64)
    wide[1:-1, :T] = seqs
    wide[:, T] = 5                                                 # a word, not <end>: a read past T would count it
    wide[0, :T] = wide[-1, :T] = 4
    dev = torch.from_numpy(wide).cuda()
    words = [w for clip in refs for r in clip for w in r]
    ref_off = np.cumsum([0] + [len(r) for clip in refs for r in clip])
    clip_ref = np.cumsum([0] + [len(clip) for clip in refs])
    d_words, v_words, h_words = guarded(words, np.int32, 136, min(4, V - 1))
    d_off, v_off, h_off = guarded(ref_off, np.int32, 4, 7)
    d_clip, v_clip, h_clip = guarded(clip_ref, np.int32, 4, 1)
    rec = torch.full((n + 2, REC), -7, dtype=torch.int32, device="cuda")
    _lib.call("acvae_accuracy_stats", dev[1:], T + 3, n, N, T, START, END, V, v_words, len(words), v_off, len(ref_off) - 1,
              v_clip, len(clip_ref) - 1, rec[1:], _lib.current_stream())
    rec = rec.cpu().numpy()
    assert np.all(rec[0] == -7) and np.all(rec[-1] == -7)
    assert np.array_equal(dev.cpu().numpy(), wide)
    for d, h in ((d_words, h_words), (d_off, h_off), (d_clip, h_clip)):
        assert np.array_equal(d.cpu().numpy(), h)
    return rec[1:-1].tolist()


@pytest.mark.parametrize("N,T", [(N, T) for N in NS for T in TS])
def test_kernel_against_the_yardstick(N, T):
    B, R, V, seed = case_of(N, T)
    seqs, refs = random_case(B, N, T, V, R, seed)
    stats = yardstick(seqs, refs, N, V)
    assert vacuity(stats, T, V) == [], (N, T, B, R, V, seed)
    lens = {len(r) for clip in refs for r in clip}
    assert len(refs[0]) == R and all(1 <= len(c) <= R for c in refs) and lens >= set(PLANTED[:sum(len(c) for c in refs)])
    got = launch(seqs, refs, N, V)
    want = [AU.record_of(s) for clip in stats for s in clip]
    assert got == want, (N, T, B, R, V, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:3])
    assert launch(seqs, refs, N, V) == got
    assert int(seqs[0, 0]) == V - 1                                 # (id 65533 with the largest vocabulary)


@pytest.mark.parametrize("T", [5, 20, 64])
def test_planted_rows(T):
    V = 50
    w = list(range(4, 44))

    def row(ids, end=True, tail=None):
        ids = list(ids)[:T - 1 if end else T] + ([END] if end else [])
        tail = GARBAGE if tail is None else tail
        return ids + [tail[k % len(tail)] for k in range(T - len(ids))]
    rows = [
        # an empty candidate, one word, <start> inside, no <end> at full length, one word repeated to the end
        [END] + [w[0]] * (T - 1), row([w[0]]), row([w[0], START, w[1], START, START, w[2]]),
        row([w[k % 3] for k in range(T)], end=False), [w[0]] * T,
        # garbage only: T times the out-of-range word; then the out-of-range word between two words
        [-5 - k for k in range(T)], [2 ** 41 + k for k in range(T)], row([w[0], V, w[1]]), row([w[0], 65535, w[1]]),
        row([70000, w[0]]),
        # a length tie (4 words against references of 3 and 5), clipping at the maximum, precision and recall apart
        row([w[0], w[1], w[2], w[3]]), row([w[0]] * 3), row([w[0], w[1], w[2], w[3]]), row([w[0], w[1]]), row([w[5]]),
    ]
    refs = [[[w[0], w[1], w[2]], [w[0]] * 70, [w[2], w[1], w[0]]],
            [[w[0], V + 5, w[1]], [-1, -1], [w[0], 65535, w[1]], [w[1], w[0]]],
            [[w[0], w[1], w[2]], [w[0], w[1], w[2], w[3], w[4]], [w[0], w[0], w[9]], [w[0], w[9]],
             [w[0], w[1], w[2], w[9], w[9], w[9], w[9], w[9]], [w[0], w[1]]]]
    seqs = np.array(rows, dtype=np.int64)
    stats = yardstick(seqs, refs, 5, V)
    got = launch(seqs, refs, 5, V)
    assert got == [AU.record_of(s) for clip in stats for s in clip]
    assert got[0] == [0, 3, 0, 0, 0, 0, 0, 0, 3]                        # nothing in, nothing counted
    # one word T times against the same word 70 times (and against three words that hold it once: recall 1/3 beats T/70)
    assert got[4] == [T, 70 if T == 64 else 3, T, T - 1, T - 2, T - 3, T] + ([64, 70] if T == 64 else [1, 3])
    assert got[5][:7] == [T, 3, 0, 0, 0, 0, 0] == got[6][:7]             # the out-of-range word matches nothing,
    assert got[7] == [3, 3, 2, 0, 0, 0, 2, 2, 3] == got[8]               # not even the reference's own
    if T > 5:
        assert got[10] == [4, 3, 4, 3, 2, 1, 4, 3, 3]                    # the tie goes to 3, not 5; recall 3/3 beats 4/5
        assert got[12][6:] == [4, 3, 3]
    assert got[11][:3] == [3, 3, 2]                                     # min(3, max(1, 1, 2, 1, 1, 1)), not min(3, 1 + 1 + 2 ...)
    assert got[13][6:] == [2, 2, 2]                                     # 2/2 (the last reference) beats 2/3 and 2/5
    assert got[14] == [1, 2, 0, 0, 0, 0, 0, 0, 3]                       # no common word: the first reference's length stays


def test_einval_returns_without_a_launch():
    out = torch.full((4096,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for kw, rc in einval_cases(_lib.lib(), out.data_ptr()):
        assert rc == -1, kw
    torch.cuda.synchronize()
    assert bool((out == -7).all())                                   # nothing ran: every output word is as it was


# ------------------------------------------------------------------------------------- the accumulator and its result()
NAMES = ("Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L", "CIDEr")


def agree(got, want, tag):
    """result() against the yardstick's dict: BLEU and ROUGE-L within 1e-12 * max(1, |x|), CIDEr within cider_util.bound ->
    the worst, in bounds."""
    worst = 0.0
    for key in NAMES:
        for g, x in [(got[key], want[key])] + list(zip(got["per_index"][key], want["per_index"][key])):
            tol = float(CU.bound(x)) if key == "CIDEr" else AU.bound(x)
            worst = max(worst, abs(g - x) / tol)
            assert abs(g - x) <= tol, (tag, key, g, x)
    x = np.asarray(want["per_clip"]["ROUGE_L"])
    assert np.all(np.abs(got["per_clip"]["ROUGE_L"] - x) <= 1e-12), (tag, "per-clip ROUGE_L")
    x = np.asarray(want["per_clip"]["CIDEr"])
    assert np.all(np.abs(got["per_clip"]["CIDEr"] - x) <= CU.bound(x)), (tag, "per-clip CIDEr")
    assert (got["clips"], got["sample_n"]) == (want["clips"], want["sample_n"])
    print(f"{tag}: worst difference {worst:.3g} of the bound")
    return worst


def same(a, b):
    return all(a[k] == b[k] and a["per_index"][k] == b["per_index"][k] for k in NAMES) and all(
        np.array_equal(a["per_clip"][k], b["per_clip"][k]) for k in ("ROUGE_L", "CIDEr")) and a["clips"] == b["clips"]


@pytest.mark.parametrize("N,T,V,R", [(1, 20, 5000, 5), (5, 20, 7, 17), (5, 64, 65534, 2)])
def test_result_and_three_updates_against_one(N, T, V, R):
    from acvae_amd.accuracy import Accuracy
    vocab = Vocabulary(["w0", "<start>", "<end>"] + [f"w{i}" for i in range(3, V)])   # id i is the yardstick's word "w<i>"
    parts, key2refs, keys = [], {}, []
    for B in (1, 3, 13):
        seqs, refs = random_case(B, N, T, V, R, 77 * N + B, clean=True)
        mine = [f"clip{len(key2refs) + b}" for b in range(B)]
        key2refs.update(zip(mine, reference_strings(refs, V)))
        keys.append(mine)
        parts.append(seqs)
    key2refs["unseen"] = ["w4 w5 w6"]                                   # a key without an update takes no part
    whole = np.concatenate(parts)
    a = Accuracy(vocab, key2refs)
    assert a.V == V
    calls = []
    real = _lib.call
    _lib.call = lambda *args: (calls.append(args[0]), real(*args))[1]
    try:
        for k, p in zip(keys, parts):
            a.update(k, torch.from_numpy(p).cuda(), N)
        assert calls == [] and len(a._rows) == 3 and all(r.is_cuda for r in a._rows)     # update launches nothing
        got = a.result()
    finally:
        _lib.call = real
    assert calls.count("acvae_accuracy_stats") == 1 and calls.count("acvae_ciderd_scores") == N
    flat = [k for ks in keys for k in ks]
    want = AU.accuracy(AU.clips_of_rows(whole, N, V), flat, key2refs)
    agree(got, want, f"N{N} T{T} V{V}")
    assert got["clips"] == 17 and 0 < want["Bleu_4"] < want["Bleu_1"] and want["ROUGE_L"] > 0 and want["CIDEr"] > 0
    assert same(a.result(), got)                                         # result() keeps the state and is reproducible
    one = Accuracy(vocab, key2refs)
    one.update(flat, torch.from_numpy(whole).cuda(), N)
    assert same(one.result(), got)
    with pytest.raises(ValueError, match="share one N"):
        a.update(["unseen"], torch.from_numpy(parts[0][:1]).cuda().repeat(N + 1, 1), N + 1)
    with pytest.raises(ValueError, match="seen twice"):
        a.update(keys[0], torch.from_numpy(parts[0]).cuda(), N)
    a.reset()
    a.update(keys[1], torch.from_numpy(parts[1]).cuda(), N)
    assert a.result()["clips"] == 3


# ------------------------------------------------------------------- evaluate(accuracy=), ensemble_evaluate(accuracy=)
ML, MN = 12, 5
_refs = {}


def small():
    """The diversity test's small model, its vocabulary and three clips, and references for them: the clip's greedy caption
    with a word dropped, the next clip's greedy caption, and a sentence with words the vocabulary lacks."""
    from test_diversity_gpu import small as model_of
    model, voc, items = model_of()
    if not _refs:
        caps = [p["tokens"].split() for p in EV.evaluate(model, items, voc, batch_size=3, max_length=ML)["predictions"]]
        assert all(len(c) >= 2 for c in caps)
        for i, (key, _) in enumerate(items):
            _refs[key] = [" ".join(caps[i][:1] + caps[i][2:]), " ".join(caps[(i + 1) % 3]), "an okapi w4 w5 grazes w6"]
    return model, voc, items, _refs


ROUTES = [dict(method="greedy"), dict(method="beam", beam_size=3), dict(method="sample", rng="device", beam_size=MN, top_p=0.9),
          dict(method="dbs", beam_size=6, group_size=3), dict(method="dbs", beam_size=5, group_size=2),
          dict(method="beam", beam_size=4, finish_on_end=True, nbest=3), dict(method="beam", beam_size=4, finish_on_end=True)]
ENSEMBLE_ROUTES = [dict(method="greedy"), dict(method="beam", beam_size=3), dict(method="dbs", beam_size=4, group_size=2),
                   dict(method="beam", beam_size=4, finish_on_end=True, nbest=2)]


def check_route(run, kw, per_clip):
    from acvae_amd.accuracy import Accuracy
    model, voc, items, key2refs = small()
    a = Accuracy(voc, key2refs)
    calls = []
    real = _lib.call
    _lib.call = lambda *args: (calls.append(args[0]), real(*args))[1]
    try:
        torch.manual_seed(21)
        payload = run(accuracy=a, **kw)
    finally:
        _lib.call = real
    assert "acvae_accuracy_stats" not in calls and len(a._rows) == 2 and a.sample_n == per_clip    # batches of two and of one
    keys, clips = AU.clips_of_payload(payload)
    assert keys == [k for k, _ in items] == a._keys and all(len(c) >= per_clip for c in clips)
    assert all(c[per_clip:] == [""] * (len(c) - per_clip) for c in clips)          # (a diverse beam search's filler rows)
    clips = [c[:per_clip] for c in clips]
    got = a.result()
    want = AU.accuracy(clips, keys, key2refs)
    agree(got, want, "-".join(f"{k}={v}" for k, v in kw.items()))
    assert want["Bleu_1"] > 0 and want["ROUGE_L"] > 0
    fresh = Accuracy(voc, key2refs)
    fresh.update_payload({"predictions": [dict(p, captions=p["captions"][:per_clip]) if "captions" in p else p
                                          for p in payload["predictions"]]})
    again = fresh.result()                                            # the document alone gives the same numbers
    assert all(again[k] == got[k] for k in NAMES)
    torch.manual_seed(21)
    without = run(**kw)
    torch.manual_seed(21)
    none = run(accuracy=None, **kw)
    assert payload == without == none                                # the payload does not know about the keyword


@pytest.mark.parametrize("kw", ROUTES, ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_evaluate_scores_what_it_writes(kw):
    model, voc, items, _ = small()
    per_clip = {0: 1, 1: 3, 2: MN, 3: 6, 4: 4, 5: 3, 6: 1}[ROUTES.index(kw)]
    check_route(lambda **k: EV.evaluate(model, items, voc, batch_size=2, max_length=ML, **k), kw, per_clip)


def test_evaluate_writes_the_same_file_with_and_without():
    import json
    import tempfile
    from acvae_amd.accuracy import Accuracy
    model, voc, items, key2refs = small()
    with tempfile.TemporaryDirectory() as tmp:
        docs = []
        for extra in (dict(accuracy=Accuracy(voc, key2refs)), dict()):
            torch.manual_seed(21)                                     # (the prior's noise is drawn on the CPU generator)
            EV.evaluate(model, items, voc, caption_output=f"{tmp}/pred.json", batch_size=2, max_length=ML, **extra)
            docs.append(open(f"{tmp}/pred.json").read())
    assert docs[0] == docs[1] and len(json.loads(docs[0])["predictions"]) == 3


def test_evaluate_with_rerank_scores_the_picked_caption():
    from acvae_amd.accuracy import Accuracy
    from acvae_amd.consensus import Consensus
    model, voc, items, key2refs = small()
    a = Accuracy(voc, key2refs)
    torch.manual_seed(9)
    picked = EV.evaluate(model, items, voc, rerank=Consensus(voc), accuracy=a, method="sample", rng="device", beam_size=MN,
                         batch_size=3, max_length=ML)
    assert all("captions" not in p for p in picked["predictions"]) and a.sample_n == 1
    keys, clips = AU.clips_of_payload(picked)
    agree(a.result(), AU.accuracy(clips, keys, key2refs), "rerank")


@pytest.mark.parametrize("kw", ENSEMBLE_ROUTES, ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_ensemble_evaluate_scores_what_it_writes(kw):
    from acvae_amd.ensemble import ensemble_evaluate
    model, voc, items, _ = small()
    per_clip = {0: 1, 1: 1, 2: 4, 3: 2}[ENSEMBLE_ROUTES.index(kw)]
    check_route(lambda **k: ensemble_evaluate([model], items, voc, batch_size=2, max_length=ML, **k), kw, per_clip)


def test_accuracy_together_with_diversity():
    import diversity_util as DU
    from acvae_amd.accuracy import Accuracy
    from acvae_amd.diversity import Diversity
    model, voc, items, key2refs = small()
    kw = dict(method="sample", rng="device", beam_size=MN, batch_size=2, max_length=ML)
    a, d, alone_a, alone_d = Accuracy(voc, key2refs), Diversity(voc), Accuracy(voc, key2refs), Diversity(voc)
    torch.manual_seed(3)
    both = EV.evaluate(model, items, voc, accuracy=a, diversity=d, **kw)
    torch.manual_seed(3)
    assert EV.evaluate(model, items, voc, accuracy=alone_a, **kw) == both
    torch.manual_seed(3)
    assert EV.evaluate(model, items, voc, diversity=alone_d, **kw) == both
    assert same(a.result(), alone_a.result())
    got, want = d.result(), alone_d.result()
    assert all(got[k] == want[k] for k in ("Div1", "Div2", "gDiv1", "mBLeu_1", "mBLeu_4"))
    keys, clips = AU.clips_of_payload(both)
    agree(a.result(), AU.accuracy(clips, keys, key2refs), "with diversity")
    assert abs(got["Div1"] - DU.diversity(clips)["Div1"]) <= 1e-12
