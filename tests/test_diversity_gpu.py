"""GPU: the diversity statistics on the device (acvae_diversity_stats, acvae_amd/diversity.py) and ``evaluate(diversity=)``.

The kernel through the C ABI against the string yardstick of tests/diversity_util.py on the rows read back: every integer
of every record equal.  N 2 / 3 / 5 / 16, T 1 / 2 / 3 / 4 / 5 / 20 / 63 / 64, B 1 / 3 / 33, ld > T, vocabularies of 7, 5000
and 65534 words (every (N, T) runs each B and each V once; over the (N, T) every pairing of B and V comes up); planted
rows.  ``seen`` over several launches between guard words; ``result()`` against the yardstick within
1e-12 * max(1, |x|); three updates against one; ``evaluate(diversity=)`` through its three routes.

The random cases do not pass vacuously; asserted on the yardstick's numbers, per case:
  - clipping is active (c_i(g) > max_j c_j(g) for some g) in at least one (clip, candidate) pair: every case;
  - at least half of the pairs have correct_2 > 0: every case with T >= 4 (a shared bigram needs two kept words on both
    sides, which T <= 3 leaves no room for beside the planted <end>, <start> and out-of-range words);
  - with the 7-word vocabulary at least one clip has a repeated n-gram of every order: every such case with T >= 20 (a
    repeated 4-gram needs eight kept words in the clip and is a matter of luck below that).
The seeds are 1000 N + 10 T + B, but for the cases of SEEDS whose yardstick numbers miss a condition at that seed."""
import numpy as np
import pytest
import torch

import acvae_oracle as O
import diversity_util as DU
from acvae_amd import _lib
from acvae_amd import evaluate as EV
from cider_util import SPECIALS, Vocabulary
from test_diversity_cpu import einval_cases
from test_model_gpu import build_model

pytestmark = pytest.mark.gpu
START, END = 1, 2
HEAD, PER = 5, 6                                                   # include/acvae_hip.h
GARBAGE = [-1, -(2 ** 62), 2 ** 40 + 5, 2 ** 63 - 1, START, END, 4, -7]
NS, TS, BS, VS = (2, 3, 5, 16), (1, 2, 3, 4, 5, 20, 63, 64), (1, 3, 33), (7, 5000, 65534)
SEEDS = {(2, 1, 1, 7): 102011, (2, 4, 1, 7): 102041, (2, 4, 33, 65534): 302073, (2, 5, 1, 5000): 202051,
         (2, 5, 3, 65534): 202053, (3, 1, 1, 65534): 103011, (3, 2, 1, 7): 103021, (3, 3, 1, 5000): 103031,
         (3, 4, 1, 65534): 203041, (3, 5, 3, 5000): 103053, (5, 4, 3, 65534): 205043, (16, 4, 3, 5000): 116043}


def launch(seqs, sample_n, V, seen=None):
    """acvae_diversity_stats on token rows [B * sample_n, T], uploaded with ld = T + 3 (garbage in the padding) ->
    (record [B, HEAD + PER * sample_n] as a list of lists, the seen buffer with 8 guard words on either side).  The record
    too lies between guard rows, which are checked here."""
    seqs = np.ascontiguousarray(seqs, dtype=np.int64)
    n, T = seqs.shape
    B, ints = n // sample_n, HEAD + PER * sample_n
    wide = np.full((n, T + 3), -(2 ** 50), dtype=np.int64)
    wide[:, :T] = seqs
    wide[:, T] = 5                                                 # a word, not <end>: a read past T would count it
    dev = torch.from_numpy(wide).cuda()
    rec = torch.full((B + 2, ints), -7, dtype=torch.int32, device="cuda")
    if seen is None:
        seen = torch.zeros(V + 1 + 16, dtype=torch.int32, device="cuda")
        seen[:8] = -7
        seen[-8:] = -7
    _lib.call("acvae_diversity_stats", dev, T + 3, n, sample_n, T, START, END, V, rec[1:], seen[8:], _lib.current_stream())
    rec = rec.cpu().numpy()
    assert np.all(rec[0] == -7) and np.all(rec[-1] == -7)
    return rec[1:-1].tolist(), seen


def slots_of(clips, V):
    """The slots of ``seen`` that the clips' words set, from the yardstick's strings."""
    return {V if w == "<out>" else int(w[1:]) for c in clips for h in c for w in h.split()}


def check_seen(seen, slots, V):
    got = seen.cpu().numpy()
    assert np.all(got[:8] == -7) and np.all(got[-8:] == -7)        # nothing written outside [0, V]
    body = got[8:-8]
    assert set(np.flatnonzero(body).tolist()) == slots and set(body.tolist()) <= {0, 1}


def random_rows(B, N, T, V, seed):
    """Rows over five words per clip (id V - 1 among them), so that a clip's candidates share n-grams and repeat their own;
    most candidates copy the beginning of candidate 0; lengths mostly in the upper half of T, a few anywhere; <start> and
    ids outside [0, V) sprinkled in; <end> where the row is shorter than T and garbage behind it."""
    rng = np.random.default_rng(seed)
    ids = np.array([i for i in range(V) if i not in (START, END)])
    seqs = np.empty((B * N, T), dtype=np.int64)
    for b in range(B):
        pool = np.concatenate([[V - 1], rng.choice(ids, 4, replace=False)])
        for i in range(N):
            row = seqs[b * N + i]
            length = int(rng.integers(0, T + 1)) if rng.random() < 0.15 else int(rng.integers((T + 1) // 2, T + 1))
            length = max(length, 1) if b == i == 0 else length
            row[:length] = rng.choice(pool, length)
            if i > 0 and rng.random() < 0.7:
                h = int(rng.integers(1, T + 1))
                row[:min(h, length)] = seqs[b * N, :min(h, length)]
            spots = rng.random(length)
            row[:length][spots < 0.03] = START
            row[:length][spots > 0.98] = [V, 2 ** 40, -3][int(rng.integers(3))]
            if b == i == 0:
                row[0] = V - 1                             # the largest id is in every case
            if length < T:
                row[length] = END
                row[length + 1:] = rng.choice(GARBAGE, T - length - 1)
    return seqs


def vacuity(stats, T, V):
    """The conditions of the module docstring on the yardstick's statistics -> the list of those missed."""
    pairs = [c for s in stats for c in s["cands"]]
    missed = []
    if not any(c["clipped"] for c in pairs):
        missed.append("no clipping")
    if T >= 4 and 2 * sum(c["correct"][1] > 0 for c in pairs) < len(pairs):
        missed.append("correct_2 > 0 in fewer than half of the pairs")
    if V == 7 and T >= 20 and not any(all(s["repeated"]) for s in stats):
        missed.append("no clip with a repeated n-gram of every order")
    return missed


def cases_of(N, T):
    at = NS.index(N) * len(TS) + TS.index(T)
    for r, B in enumerate(BS):
        V = VS[(r + at) % 3]
        yield B, V, SEEDS.get((N, T, B, V), 1000 * N + 10 * T + B)


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("N", NS)
def test_kernel_against_the_yardstick(N, T):
    for B, V, seed in cases_of(N, T):
        seqs = random_rows(B, N, T, V, seed)
        clips = DU.clips_of_rows(seqs, N, V)
        stats = [DU.clip_stats(c) for c in clips]
        assert vacuity(stats, T, V) == [], (N, T, B, V, seed)
        got, seen = launch(seqs, N, V)
        again, _ = launch(seqs, N, V)
        want = [DU.record_of(s) for s in stats]
        assert got == want, (N, T, B, V, [(g, w) for g, w in zip(got, want) if g != w][:2])
        assert again == got
        check_seen(seen, slots_of(clips, V), V)
        assert V - 1 in slots_of(clips, V)                           # (id 65533 with the largest vocabulary)


@pytest.mark.parametrize("T", [5, 20, 64])
def test_planted_rows(T):
    V = 50
    w = list(range(4, 44))

    def row(ids, end=True, tail=None):
        ids = list(ids)[:T - 1 if end else T] + ([END] if end else [])
        tail = GARBAGE if tail is None else tail
        return ids + [tail[k % len(tail)] for k in range(T - len(ids))]
    clips = [
        # an empty candidate, one word, <start> inside, no <end> at full length, one word repeated to the end
        [[END] + [w[0]] * (T - 1), row([w[0]]), row([w[0], START, w[1], START, START, w[2]]),
         row([w[k % 3] for k in range(T)], end=False), [w[0]] * T],
        # all candidates empty (the last one by <start> alone)
        [row([]), row([]), [END] * T, row([], tail=[-1]), row([START, START])],
        # garbage only: negative ids and ids above 2^40, no <end>: T times the out-of-range word
        [[-5 - k for k in range(T)], [2 ** 41 + k for k in range(T)], row([V]), row([V + 1, w[0]]), row([65535, 70000])],
        # hypotheses shorter than the order, and a length tie: 4 words against references of 3 and 5
        [row([w[0], w[1], w[2], w[3]]), row([w[0], w[1], w[2]]), row([w[0], w[1], w[2], w[3], w[4]][:T - 1]), row([w[0]]),
         row([w[0], w[1]])],
        # counts above 1 on both sides: clipping at the maximum over the references, not their sum
        [row([w[0]] * 3), row([w[0]]), row([w[0]]), row([w[1], w[0]]), row([w[1]] * 3)],
    ]
    seqs = np.array([r for c in clips for r in c], dtype=np.int64)
    strings = DU.clips_of_rows(seqs, 5, V)
    stats = [DU.clip_stats(c) for c in strings]
    got, seen = launch(seqs, 5, V)
    assert got == [DU.record_of(s) for s in stats]
    check_seen(seen, slots_of(strings, V), V)
    assert seen[8 + V].item() == 1                                       # the out-of-range word's slot
    assert got[1] == [0] * 5 + [0, 0, 0, 0, 0, 0] * 5                    # nothing in, nothing counted
    assert got[2][:2] == [2 * T + 5, 2] and got[2][HEAD:HEAD + 3] == [T, T, T]     # one word, T times, in two candidates
    if T > 5:
        assert got[3][HEAD:HEAD + 2] == [4, 3] and got[3][HEAD + 2:HEAD + PER] == [4, 3, 2, 1]    # the tie goes to 3, not 5
    assert got[4][HEAD:HEAD + 3] == [3, 3, 1]                           # min(3, max(1, 1, 1, 0)), not min(3, 1 + 1 + 1)
    # sixteen candidates, the last two identical and unlike the rest
    rows16 = [row([w[2 * j], w[2 * j + 1]]) for j in range(14)] + [row([w[35], w[36], w[37]])] * 2
    got16, _ = launch(np.array(rows16), 16, V)
    assert got16 == [DU.record_of(DU.clip_stats(DU.clips_of_rows(np.array(rows16), 16, V)[0]))]
    assert got16[0][:3] == [34, 31, 16] and got16[0][HEAD + PER * 15:] == [3, 3, 3, 2, 1, 0]


def test_seen_accumulates_over_launches():
    """The kernel never clears ``seen``: after each of three launches of different shapes it holds the words of all rows so
    far, the out-of-range slot among them, and the guard words on either side stand."""
    V, seen, slots = 5000, None, set()
    for k, (B, N, T) in enumerate([(3, 5, 20), (1, 16, 64), (33, 2, 5)]):
        seqs = random_rows(B, N, T, V, 900 + k)
        _, seen = launch(seqs, N, V, seen)
        before = len(slots)
        slots |= slots_of(DU.clips_of_rows(seqs, N, V), V)
        assert len(slots) > before
        check_seen(seen, slots, V)
    assert V in slots


def test_einval_returns_without_a_launch():
    out = torch.full((4096,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for kw, rc in einval_cases(_lib.lib(), out.data_ptr()):
        assert rc == -1, kw
    torch.cuda.synchronize()
    assert bool((out == -7).all())                                   # nothing ran: every output word is as it was


# ------------------------------------------------------------------------------------- the accumulator and its result()
KEYS = ("Div1", "Div2", "gDiv1", "mBLeu_1", "mBLeu_2", "mBLeu_3", "mBLeu_4")


def agree(got, want, tag):
    """result() against the yardstick's dict, every number within 1e-12 * max(1, |x|) -> the worst, in bounds."""
    worst = 0.0
    for key in KEYS:
        err = abs(got[key] - want[key])
        worst = max(worst, err / DU.bound(want[key]))
        assert err <= DU.bound(want[key]), (tag, key, got[key], want[key])
    for key in ("div1", "div2"):
        err = np.abs(np.asarray(got["per_clip"][key]) - np.asarray(want["per_clip"][key]))
        assert np.all(err <= 1e-12), (tag, key)
    assert (got["clips"], got["sample_n"]) == (want["clips"], want["sample_n"])
    print(f"{tag}: worst difference {worst:.3g} of the bound")
    return worst


def same(a, b):
    return all(a[k] == b[k] for k in KEYS + ("clips", "sample_n")) and all(
        np.array_equal(a["per_clip"][k], b["per_clip"][k]) for k in ("div1", "div2"))


@pytest.mark.parametrize("N,T,V", [(5, 20, 5000), (16, 64, 7), (2, 5, 65534)])
def test_result_and_three_updates_against_one(N, T, V):
    from acvae_amd.diversity import Diversity
    vocab = Vocabulary(SPECIALS + [f"w{i}" for i in range(4, V)])
    parts = [random_rows(B, N, T, V, 77 * N + B) for B in (1, 3, 33)]
    whole = np.concatenate(parts)
    d = Diversity(vocab)
    assert d.V == V
    for p in parts:
        d.update(torch.from_numpy(p).cuda(), N)
    assert len(d._records) == 3 and all(r.is_cuda for r in d._records) and d._seen.is_cuda
    got = d.result()
    want = DU.diversity(DU.clips_of_rows(whole, N, V))
    agree(got, want, f"N{N} T{T} V{V}")
    assert got["clips"] == 37 and got["gDiv1"] == len(slots_of(DU.clips_of_rows(whole, N, V), V))
    one = Diversity(vocab)
    one.update(torch.from_numpy(whole).cuda(), N)
    assert same(one.result(), got)
    raw = d.stats(torch.from_numpy(parts[1]).cuda(), N)              # the raw record of one call; the object's state stays
    assert raw["record"].cpu().numpy().tolist() == [DU.record_of(s) for s in want["stats"][1:4]]
    assert int(raw["seen"].sum()) == len(slots_of(DU.clips_of_rows(parts[1], N, V), V)) and same(d.result(), got)
    with pytest.raises(ValueError, match="share one N"):
        d.update(torch.from_numpy(parts[1][:6]).cuda(), 3 if N != 3 else 2)
    d.reset()
    d.update(torch.from_numpy(parts[0]).cuda(), N)
    assert d.result()["clips"] == 1


# ---------------------------------------------------------------------------------------------- evaluate(diversity=)
MV, ME, ML, MN = 40, 64, 12, 5
_model = {}


def small():
    """The consensus test's small model (closed-form weights, V = 40, E = 64; the bias of <end> lowered so that captions
    differ in length), its vocabulary and three clips."""
    if not _model:
        state = O.closed_form_state(O.state_shapes(MV, ME, ME, None, ME, 512))
        state["decoder.classifier.bias"] = state["decoder.classifier.bias"].clone()
        state["decoder.classifier.bias"][O.END_IDX] -= 2.0
        voc = EV.Vocabulary()
        for word in SPECIALS + [f"w{i}" for i in range(4, MV)]:
            voc.add_word(word)
        g = torch.Generator().manual_seed(5)
        items = [(f"clip{i}", torch.randn(64, 64, generator=g)) for i in range(3)]
        _model["m"] = (build_model(MV, ME, state).eval(), voc, items)
    return _model["m"]


ROUTES = [dict(method="sample", rng="device", beam_size=MN, top_p=0.9), dict(method="greedy", beam_size=3),
          dict(method="dbs", beam_size=6, group_size=3), dict(method="dbs", beam_size=4, group_size=2, group_nbest=False),
          dict(method="beam", beam_size=4, finish_on_end=True, nbest=3)]


@pytest.mark.parametrize("kw", ROUTES, ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_evaluate_counts_what_it_writes(kw):
    from acvae_amd.diversity import Diversity
    model, voc, items = small()
    d = Diversity(voc)
    calls = []
    real = _lib.call
    _lib.call = lambda *a: (calls.append(a[0]), real(*a))[1]
    try:
        torch.manual_seed(21)
        payload = EV.evaluate(model, items, voc, batch_size=2, max_length=ML, diversity=d, **kw)
    finally:
        _lib.call = real
    assert calls.count("acvae_diversity_stats") == 2 and len(d._records) == 2          # batches of two clips and of one
    clips = DU.clips_of_payload(payload)
    assert len(clips) == 3 and len(clips[0]) == d.sample_n
    assert all(any(c for c in clip) for clip in clips)               # there are words to count,
    if kw["method"] == "sample":
        assert all(len(set(clip)) > 1 for clip in clips)             # and a clip's samples are not all alike
    got = d.result()
    agree(got, DU.diversity(clips), kw["method"])
    fresh = Diversity(voc)
    fresh.update_payload(payload)                                    # the document alone gives the same numbers
    assert same(fresh.result(), got)
    torch.manual_seed(21)
    without = EV.evaluate(model, items, voc, batch_size=2, max_length=ML, **kw)
    torch.manual_seed(21)
    none = EV.evaluate(model, items, voc, batch_size=2, max_length=ML, diversity=None, **kw)
    assert payload == without == none                                # the payload does not know about the keyword


def test_evaluate_dbs_counts_only_the_filled_rows():
    """beam_size 5 in groups of 2: four beams and one filler row of <end> per clip, which the file shows as an empty fifth
    caption and the statistics leave out."""
    from acvae_amd.diversity import Diversity
    model, voc, items = small()
    d = Diversity(voc)
    payload = EV.evaluate(model, items, voc, batch_size=3, max_length=ML, diversity=d, method="dbs", beam_size=5, group_size=2)
    clips = DU.clips_of_payload(payload)
    assert all(len(c) == 5 and c[4] == "" for c in clips) and d.sample_n == 4
    agree(d.result(), DU.diversity([c[:4] for c in clips]), "dbs 5 / 2")


def test_evaluate_with_rerank_counts_the_candidates():
    from acvae_amd.consensus import Consensus
    from acvae_amd.diversity import Diversity
    model, voc, items = small()
    kw = dict(method="sample", rng="device", beam_size=MN, batch_size=3, max_length=ML)
    d, plain = Diversity(voc), Diversity(voc)
    torch.manual_seed(9)
    picked = EV.evaluate(model, items, voc, rerank=Consensus(voc), diversity=d, **kw)
    torch.manual_seed(9)
    payload = EV.evaluate(model, items, voc, diversity=plain, **kw)
    assert all("captions" not in p for p in picked["predictions"])   # one picked caption per clip in the file,
    assert d.sample_n == MN and same(d.result(), plain.result())     # the N rollouts in the statistics
    agree(d.result(), DU.diversity(DU.clips_of_payload(payload)), "rerank")
