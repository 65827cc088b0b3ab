"""GPU: Ensemble.rollout and ensemble_evaluate(sample_n=) (one acvae_ensemble_rollout call per batch), golden-size members
from test_ensemble_gpu's helpers.

Against the host-loop twin (ensemble_rollout_util.rollout_twin, the oracle's steps mixed and scored in float64), fed the
device's words step by step so that one differing decision changes no later one.  A word is compared wherever the twin's
float64 score margin exceeds twice the bound: the kernel test's score_bound, plus STEP / temp, STEP = MARGIN = 20 x LP_TOL
of test_fullsize_decode_gpu.py being the allowance of test_ensemble_gpu.py for the members' step kernels against the
oracle over a caption's steps, which carries over to the mixture (the log of a convex combination of probabilities each
within a factor e^d is within d) and is divided by temp with it.  At most 2 % of a case's decisions may be left out, and the
bound stays below 1e-2.

Exact, with no yardstick: greedy with one row per clip is Ensemble.forward's greedy bit for bit; top_k = 1 picks greedy's
words; banned words never appear; the picked rows are Consensus.select's; one library call per batch."""
import numpy as np
import pytest
import torch

import acvae_oracle as O
import ensemble_rollout_util as RU
import ensemble_util as EU
from acvae_amd import _lib
from acvae_amd.batch import collate_fn
from acvae_amd.ensemble import Ensemble, ensemble_evaluate
from acvae_amd.evaluate import collect_predictions, predictions_payload
from test_ensemble_gpu import V, MAXLEN, member, _threads            # noqa: F401  (_threads: the autouse fixture)
from test_ensemble_rollout_kernels_gpu import MAX_BOUND, MAX_LEFT_OUT, mixture_and_bound, score_bound
from test_fullsize_decode_gpu import MARGIN as STEP

pytestmark = pytest.mark.gpu

MEMBERS = {1: [("Cnn10", 64, 11)], 2: [("Cnn10", 64, 11), ("Cnn10", 64, 12)],
           3: [("Cnn10", 64, 13), ("Cnn14_16k", 64, 14), ("Cnn10", 128, 15)]}       # unequal embed widths and frame rates
_setups = {}


def setup(M, B):
    """Members, features and the oracle's encoder memories, once per (M, B)."""
    if (M, B) not in _setups:
        ms = [member(*m) for m in MEMBERS[M]]
        feats, _, fl, _ = O.synthetic_batch(B, 128 if M == 3 else 96, V, 7, seed=40 + B, ragged=B > 1)
        states = [s for _, s in ms]
        _setups[(M, B)] = dict(models=[m for m, _ in ms], states=states, feats=feats, fl=fl, dims=[m[1] for m in MEMBERS[M]],
                               encoded=[EU.encode(s, feats, fl) for s in states])
    return _setups[(M, B)]


def noise_of(d, B, n, method, T=MAXLEN, seed=0):
    """Replayed noise: (eps per member [B, T, n, E_m], word noise [T, B * n, V]) - Gumbel or Exp(1), None for greedy."""
    g = torch.Generator().manual_seed(1000 * B + 10 * n + seed)
    eps = [torch.randn(B, T, n, E, generator=g) for E in d["dims"]]
    if method == "greedy":
        return eps, None
    if method == "gumbel":
        word = -torch.log(-torch.log(torch.rand(T, B * n, V, generator=g) + 1e-20) + 1e-20)
    else:
        word = torch.empty(T, B * n, V).exponential_(1, generator=g)
    return eps, word


def rollout(d, eps, word, n, **kw):
    ens = Ensemble(d["models"])
    ens.noise = {"eps": eps} if word is None else {"eps": eps, "sample_noise": word}
    out = ens.rollout(d["feats"].cuda(), d["fl"].copy(), sample_n=n, max_length=kw.pop("max_length", MAXLEN), **kw)
    assert ens.noise is None
    return out


def twin_and_bounds(d, eps, word, n, method, temp, seqs, T=MAXLEN):
    """-> (the twin fed the device's words `seqs`, the bound [R, T] of each of its decisions: see the file's docstring)."""
    twin = RU.rollout_twin(d["states"], d["encoded"], n, T, eps, None if word is None else word.numpy(), method, temp,
                           feed=seqs)
    rule = "gumbel" if word is None else method                          # (greedy: the mixture itself, no noise)
    bounds = np.zeros(seqs.shape)
    for t in range(T):
        v, mixb = mixture_and_bound(twin["logits"][t])
        z = np.zeros_like(twin["logits"][t][0]) if word is None else word[t].numpy()
        sb = score_bound(mixb, v, z, rule, temp) + STEP / temp
        order = np.argsort(-RU.log_scores(v, z, rule, temp), -1, kind="stable")[:, :2]
        bounds[:, t] = np.take_along_axis(sb, order, -1).max(-1)
    assert bounds.max() <= MAX_BOUND
    return twin, bounds


def against_twin(d, eps, word, n, method, temp, seqs, logprobs, T=MAXLEN):
    """The device's rows against the twin fed the device's words -> the share of decisions left out."""
    twin, bounds = twin_and_bounds(d, eps, word, n, method, temp, seqs, T)
    left_out = 0
    for t in range(T):
        held = seqs[:, t - 1] == O.END_IDX if t > 0 else np.zeros(len(seqs), bool)     # (what the twin was fed)
        assert (seqs[held, t] == O.END_IDX).all()
        decided = (twin["gap"][:, t] > 2 * bounds[:, t]) | held
        assert np.array_equal(seqs[decided, t], twin["seqs"][decided, t]), (t, n, method)
        same = seqs[:, t] == twin["seqs"][:, t]                           # the same word: the same log-probability
        assert (np.abs(logprobs[same, t] - twin["logprobs"][same, t]) <= STEP).all(), t
        left_out += int((~decided).sum())
    return left_out / seqs.size


@pytest.mark.parametrize("M,B,n,method,temp", [(1, 1, 1, "sample", 1.0), (2, 3, 2, "gumbel", 0.7), (3, 2, 5, "sample", 1.0),
                                               (2, 7, 5, "sample", 0.5), (3, 7, 5, "gumbel", 2.0), (1, 3, 2, "sample", 2.0),
                                               (3, 7, 5, "greedy", 1.0)])
def test_device_words_vs_host_loop_twin(M, B, n, method, temp):
    d = setup(M, B)
    eps, word = noise_of(d, B, n, method)
    out = rollout(d, eps, word, n, method=method, temp=temp)
    seqs, logprobs = out["seqs"].cpu().numpy(), out["logprobs"].cpu().numpy().astype(np.float64)
    assert seqs.shape == logprobs.shape == (B * n, MAXLEN) and set(out) == {"seqs", "logprobs"}
    left_out = against_twin(d, eps, word, n, method, temp, seqs, logprobs)
    print(f"M={M} B={B} n={n} {method} temp={temp}: {left_out:.2%} of the decisions left out")
    assert left_out <= MAX_LEFT_OUT
    if method != "greedy" and B * n > 2:
        assert len({tuple(r) for r in seqs.tolist()}) > 1                   # samples, not one caption repeated


@pytest.mark.parametrize("M,B", [(1, 3), (3, 7)])
def test_greedy_with_one_row_per_clip_is_forward_greedy_bit_for_bit(M, B):
    d = setup(M, B)
    eps, _ = noise_of(d, B, 1, "greedy")
    ens = Ensemble(d["models"])
    ens.noise = {"eps": eps}
    want = ens(d["feats"].cuda(), d["fl"].copy(), method="greedy", max_length=MAXLEN)
    got = rollout(d, eps, None, 1, method="greedy")
    assert torch.equal(got["seqs"], want["seqs"])
    assert torch.equal(got["logprobs"].view(torch.int32), want["logprobs"].view(torch.int32))


@pytest.mark.parametrize("method", ["sample", "gumbel"])
def test_top_k_1_is_greedy_word_for_word(method):
    d = setup(2, 3)
    eps, word = noise_of(d, 3, 2, method)
    greedy = rollout(d, eps, None, 2, method="greedy")
    got = rollout(d, eps, word, 2, method=method, top_k=1, temp=0.7)
    assert torch.equal(got["seqs"], greedy["seqs"])
    assert float((got["logprobs"] - greedy["logprobs"]).abs().max()) <= 1e-5   # (log_softmax of the normalised row again)
    nucleus = rollout(d, eps, word, 2, method=method, top_p=1e-6)            # rank 0 alone is the same row
    assert torch.equal(nucleus["seqs"], greedy["seqs"])
    # top_k = 3: every word an unfinished row draws is among the three most probable of the twin's mixture
    three = rollout(d, eps, word, 2, method=method, top_k=3)
    seqs, lp = three["seqs"].cpu().numpy(), three["logprobs"].cpu().numpy()
    twin = RU.rollout_twin(d["states"], d["encoded"], 2, MAXLEN, eps, word.numpy(), method, 1.0, feed=seqs)
    assert not torch.equal(three["seqs"], greedy["seqs"])                     # (and it does sample)
    for t in range(MAXLEN):
        third = np.sort(twin["v"][t], -1)[:, -3]
        free = seqs[:, t - 1] != O.END_IDX if t > 0 else np.ones(len(seqs), bool)
        assert (lp[free, t] >= third[free] - 2 * STEP).all(), t


@pytest.mark.parametrize("method", ["greedy", "sample"])
def test_constraints_ban_words_and_hold_the_minimum_length(method):
    d = setup(2, 3)
    eps, word = noise_of(d, 3, 5, method)
    free = rollout(d, eps, word, 5, method=method)["seqs"].cpu().numpy()
    ids, counts = np.unique(free[free != O.END_IDX], return_counts=True)
    banned = [int(w) for w in ids[np.argsort(-counts)][:4]]                 # the words the free rollout uses most
    got = rollout(d, eps, word, 5, method=method, suppress_tokens=banned, min_length=MAXLEN - 2,
                  no_repeat_ngram_size=1)["seqs"].cpu().numpy()
    assert not np.isin(got, banned).any()
    assert (got[:, :MAXLEN - 2] != O.END_IDX).all()
    for row in got.tolist():
        body = row[:row.index(O.END_IDX)] if O.END_IDX in row else row
        assert len(set(body)) == len(body)                                 # no word twice
        if O.END_IDX in row:
            assert row[row.index(O.END_IDX):] == [O.END_IDX] * (MAXLEN - row.index(O.END_IDX))


@pytest.mark.parametrize("method", ["sample", "gumbel"])
def test_one_member_is_the_single_model_rollout(method):
    """Ensemble([m]) against m.rollout_shared_encoder on the same replayed noise: other kernels (the decode loop's own
    log-softmax and draw), the same rule.  A row is compared up to its first decision that the twin leaves undecided (from
    there on the two may have been fed different words), and up to and including its first <end>."""
    B, n, temp = 3, 5, 1.0
    d = setup(1, B)
    m = d["models"][0]
    eps, word = noise_of(d, B, n, method, seed=3)
    got = rollout(d, eps, word, n, method=method, temp=temp)
    seqs = got["seqs"].cpu().numpy()
    m.noise = {"eps_p": eps[0].transpose(0, 1).reshape(MAXLEN, B * n, -1), "sample_noise": word}
    with torch.no_grad():
        single = m.rollout_shared_encoder(d["feats"].cuda(), d["fl"].copy(), n, method=method, temp=temp, max_length=MAXLEN)
    want = single["seqs"].cpu().numpy()
    twin, bounds = twin_and_bounds(d, eps, word, n, method, temp, seqs)
    compared = 0
    for r in range(B * n):
        for t in range(MAXLEN):
            if twin["gap"][r, t] <= 2 * bounds[r, t]:
                break
            assert seqs[r, t] == want[r, t], (r, t)
            compared += 1
            if seqs[r, t] == O.END_IDX:
                break
    print(f"{method}: {compared} decisions compared")
    assert compared >= 0.5 * sum((row.tolist().index(O.END_IDX) + 1 if O.END_IDX in row else MAXLEN) for row in seqs)


def test_rerank_picks_what_consensus_select_picks():
    from acvae_amd.consensus import Consensus
    from test_ensemble_gpu import vocabulary
    B, n = 3, 5
    d = setup(2, B)
    eps, word = noise_of(d, B, n, "sample")
    plain = rollout(d, eps, word, n, method="sample")
    c = Consensus(vocabulary())
    out = rollout(d, eps, word, n, method="sample", rerank=c)
    assert torch.equal(out["candidates"], plain["seqs"]) and torch.equal(out["logprobs"], plain["logprobs"])
    want = c.select(out["candidates"], n, O.START_IDX, O.END_IDX)
    assert out["seqs"].shape == (B, MAXLEN) and torch.equal(out["seqs"], want["seqs"])
    assert torch.equal(out["consensus_best"], want["best"]) and torch.equal(out["consensus_scores"], want["scores"])
    rows = out["candidates"].reshape(B, n, MAXLEN)
    assert torch.equal(out["seqs"], rows[torch.arange(B), out["consensus_best"].cpu()])


def test_rng_host_and_device_draw_under_a_seed_and_replay():
    d = setup(2, 3)
    outs = {}
    for rng in ("device", "host"):
        for rep in range(2):
            torch.manual_seed(5)
            ens = Ensemble(d["models"])
            outs[rng, rep] = ens.rollout(d["feats"].cuda(), d["fl"].copy(), sample_n=2, method="gumbel", rng=rng,
                                         max_length=MAXLEN)["seqs"]
        assert torch.equal(outs[rng, 0], outs[rng, 1])
        assert outs[rng, 0].shape == (6, MAXLEN) and int(outs[rng, 0].min()) >= 0 and int(outs[rng, 0].max()) < V


def test_ensemble_evaluate_sample_n(tmp_path):
    import json
    from acvae_amd.accuracy import Accuracy
    from acvae_amd.consensus import Consensus
    from acvae_amd.diversity import Diversity
    from test_accuracy_gpu import same
    from test_ensemble_gpu import vocabulary
    d = setup(2, 3)
    models, voc, ML = d["models"], vocabulary(), MAXLEN
    items = [(f"clip{i}", d["feats"][i, :int(d["fl"][i])].clone()) for i in range(3)]
    key2refs = {key: ["w4 w5 w6 w7", f"w{8 + i} w9 w10", "an okapi w4 grazes"] for i, (key, _) in enumerate(items)}
    start_idx, end_idx = O.START_IDX, O.END_IDX
    n = 4
    kw = dict(sample_n=n, method="sample", temp=0.8, max_length=ML, batch_size=2)
    calls = []
    real = _lib.call
    _lib.call = lambda *args: (calls.append(args[0]), real(*args))[1]
    try:
        a, dv = Accuracy(voc, key2refs), Diversity(voc)
        torch.manual_seed(4)
        payload = ensemble_evaluate(models, items, voc, caption_output=tmp_path / "n.json", accuracy=a, diversity=dv, **kw)
    finally:
        _lib.call = real
    # one library call per batch (two batches), and nothing of the step API
    assert calls.count("acvae_ensemble_rollout") == 2
    assert not [c for c in calls if c in ("acvae_prior_step_fwd", "acvae_decoder_step_fwd", "acvae_attn_precompute",
                                          "acvae_ensemble_search", "acvae_ensemble_mix", "acvae_ensemble_mix_sample")]
    assert json.load(open(tmp_path / "n.json")) == payload
    assert all(len(p["captions"]) == n for p in payload["predictions"])
    # by hand: the same batches through rollout, the downloaded rows to fresh objects
    torch.manual_seed(4)
    ens, key2pred = Ensemble(models), {}
    a2, dv2 = Accuracy(voc, key2refs), Diversity(voc)
    for lo in range(0, len(items), 2):
        batch = collate_fn([1])(list(items[lo:lo + 2]))
        rows = ens.rollout(batch[1].cuda(), batch[-1], sample_n=n, method="sample", temp=0.8, max_length=ML)["seqs"].cpu().numpy()
        a2.update(list(batch[0]), torch.from_numpy(rows).cuda(), n)
        dv2.update(torch.from_numpy(rows).cuda(), n)
        collect_predictions(batch[0], rows.reshape(len(batch[0]), n, ML), voc, False, key2pred)
    assert payload == predictions_payload(key2pred, False)
    assert same(a.result(), a2.result())
    got, want = dv.result(), dv2.result()
    assert all(got[k] == want[k] for k in ("Div1", "Div2", "gDiv1", "mBLeu_1", "mBLeu_4")) and got["sample_n"] == n
    # with rerank: one caption per clip, the one Consensus.select picks; accuracy scores it, diversity the candidates
    c = Consensus(voc)
    a3, dv3 = Accuracy(voc, key2refs), Diversity(voc)
    torch.manual_seed(4)
    picked = ensemble_evaluate(models, items, voc, rerank=c, accuracy=a3, diversity=dv3, **kw)
    assert all("captions" not in p for p in picked["predictions"]) and a3.sample_n == 1
    torch.manual_seed(4)
    ens, key2pred, a4 = Ensemble(models), {}, Accuracy(voc, key2refs)
    for lo in range(0, len(items), 2):
        batch = collate_fn([1])(list(items[lo:lo + 2]))
        cand = ens.rollout(batch[1].cuda(), batch[-1], sample_n=n, method="sample", temp=0.8, max_length=ML)["seqs"]
        rows = c.select(cand, n, start_idx, end_idx)["seqs"].cpu().numpy()
        a4.update(list(batch[0]), torch.from_numpy(rows).cuda(), 1)
        collect_predictions(batch[0], rows, voc, False, key2pred)
    assert picked == predictions_payload(key2pred, False)
    assert same(a3.result(), a4.result())
    assert all(dv3.result()[k] == want[k] for k in ("Div1", "Div2", "gDiv1", "mBLeu_1", "mBLeu_4"))
    # sample_n = None: the payload, and the calls, of today
    torch.manual_seed(4)
    today = ensemble_evaluate(models, items, voc, method="greedy", max_length=ML, batch_size=2)
    torch.manual_seed(4)
    ens, key2pred = Ensemble(models), {}
    for lo in range(0, len(items), 2):
        batch = collate_fn([1])(list(items[lo:lo + 2]))
        collect_predictions(batch[0], ens(batch[1].cuda(), batch[-1], method="greedy", max_length=ML)["seqs"].cpu().numpy(), voc,
                            False, key2pred)
    assert today == predictions_payload(key2pred, False)
    torch.manual_seed(4)
    assert today == ensemble_evaluate(models, items, voc, method="greedy", max_length=ML, batch_size=2, sample_n=None,
                                      rerank=None, diversity=None)


def test_one_library_call_per_rollout():
    d = setup(2, 3)
    eps, word = noise_of(d, 3, 2, "sample")
    for kw, extra in ((dict(method="sample"), []), (dict(method="greedy"), []), (dict(method="gumbel", top_k=5), []),
                      (dict(method="sample", rng="device"), ["acvae_sample_noise"])):
        calls = []
        real = _lib.call
        _lib.call = lambda *args: (calls.append(args[0]), real(*args))[1]
        try:
            if "rng" in kw:
                Ensemble(d["models"]).rollout(d["feats"].cuda(), d["fl"].copy(), sample_n=2, max_length=MAXLEN, **kw)
            else:
                rollout(d, eps, None if kw["method"] == "greedy" else word, 2, **kw)
        finally:
            _lib.call = real
        text = [c for c in calls if c.startswith(("acvae_ensemble", "acvae_prior_step", "acvae_decoder_step", "acvae_sample",
                                                  "acvae_attn_precompute", "acvae_beam", "acvae_decode"))]
        assert sorted(text) == sorted(["acvae_ensemble_rollout_scratch_bytes", "acvae_ensemble_rollout"] + extra), (kw, text)
