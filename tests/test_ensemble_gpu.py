"""GPU: acvae_amd.ensemble (one acvae_ensemble_search call per batch) against the single-model search where the two must agree
exactly, and against the CPU restatement of tests/ensemble_util.py where the members differ.

Exact, with no yardstick: Ensemble([m]) is m.beam_search token for token (replayed noise, and under a seed: the generator-order
contract); three deep copies of a model fed the same noise decode as one.
Against the helper: tokens exact on every clip whose smallest decision margin is at least MARGIN = 20 x LP_TOL, LP_TOL = 1e-5
being the log-softmax error of one step call against the oracle (test_fullsize_decode_gpu.py).  That bound carries over to the
mixture: the log of a convex combination of probabilities, each within a factor e^d, is within d.  At most 10 % of a case's
clips, rounded down, may be excluded - none at 3 to 5 clips, so the seeds below were picked with the helper alone, on the
CPU, for margins above MARGIN on every clip (the smallest are printed)."""
import copy
import csv
import json
import os

import numpy as np
import pytest
import torch

import acvae_oracle as O
import ensemble_util as EU
from acvae_amd.batch import collate_fn
from acvae_amd.ensemble import Ensemble, ensemble_evaluate
from acvae_amd.evaluate import Vocabulary, collect_predictions, predictions_payload
from test_fullsize_decode_gpu import LP_TOL, MARGIN, guarded
from test_model_gpu import _beam_call_vs_step_loop, build_model

pytestmark = pytest.mark.gpu
V, MAXLEN = 50, 8

_members, _cases = {}, {}


@pytest.fixture(autouse=True)
def _threads():                   # the helper's CPU steps: no more threads than the test box grants
    n = torch.get_num_threads()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    yield
    torch.set_num_threads(n)


def member(encoder, E, seed, end_bump=0.0, vocab=V):
    """(model on the GPU in eval mode, its state dict on the CPU), built once per (encoder, E, seed, end_bump).  E: one number
    for every width of the text side, or (E, H, A): embed, decoder-GRU and attention widths apart (tests/widths_util.py)."""
    key = (encoder, E, seed, end_bump, vocab)
    if key not in _members:
        torch.manual_seed(seed)
        if isinstance(E, tuple):
            import widths_util as W
            model = W.build_model(V, E[0], E[1], E[2], E[0], encoder=encoder).eval()
        elif vocab == V:
            model = build_model(V, E, encoder=encoder).eval()
        else:
            from test_fullsize_gpu import build
            model = build(seed).eval()
        if end_bump:
            with torch.no_grad():
                model.decoder.classifier.bias[O.END_IDX] += end_bump
        _members[key] = (model, {k: v.detach().cpu().clone() for k, v in model.state_dict().items()})
    return _members[key]


CASES = {     # members (encoder, E, seed[, end_bump]), clips, T, seed of the features, seed of the noise
    "m2_cnn10": dict(members=[("Cnn10", 64, 11), ("Cnn10", 64, 12)], N=4, T=96, fseed=21, eseed=31),
    "m3_mixed": dict(members=[("Cnn10", 64, 13), ("Cnn14_16k", 64, 14), ("Cnn10", 128, 15)], N=3, T=128, fseed=22, eseed=32),
    "m2_end_bump": dict(members=[("Cnn10", 64, 11, 0.6), ("Cnn10", 64, 12)], N=5, T=96, fseed=23, eseed=33),
    # members whose GRU and attention widths differ from their embed width and from each other's (seeds: see the test)
    "m2_widths": dict(members=[("Cnn10", (64, 96, 160), 16), ("Cnn10", (64, 32, 96), 17)], N=4, T=96, fseed=25, eseed=35),
    "full_size": dict(members=[("Cnn10", 512, 5), ("Cnn10", 512, 6)], N=11, T=160, fseed=24, eseed=39, vocab=5000, maxlen=20),
}


def case_data(name):
    """Members, features and the members' encoder memories by the oracle (computed once per case, never modified)."""
    if name not in _cases:
        c = CASES[name]
        vocab = c.get("vocab", V)
        ms = [member(*m, vocab=vocab) for m in c["members"]]
        feats, _, fl, _ = O.synthetic_batch(c["N"], c["T"], vocab, 7, seed=c["fseed"], ragged=True)
        states = [s for _, s in ms]
        _cases[name] = dict(models=[m for m, _ in ms], states=states, feats=feats, fl=fl, maxlen=c.get("maxlen", MAXLEN),
                            dims=[m[1][0] if isinstance(m[1], tuple) else m[1] for m in c["members"]], encoded=[EU.encode(s, feats, fl) for s in states], ref={})
    return _cases[name]


def noise(name, beam):
    d, c = case_data(name), CASES[name]
    g = torch.Generator().manual_seed(c["eseed"] + 100 * beam)
    return [torch.randn(c["N"], d["maxlen"], beam, E, generator=g) for E in d["dims"]]


def reference(name, method, beam):
    """(seqs, logprobs, margins) of the helper, once per (case, method, beam)."""
    d = case_data(name)
    key = (method, beam)
    if key not in d["ref"]:
        rec = {}
        eps = noise(name, beam)
        if method == "greedy":
            seqs, lp = EU.ensemble_greedy(d["states"], d["encoded"], d["maxlen"], eps, record=rec)
        else:
            seqs, lp = EU.ensemble_beam(d["states"], d["encoded"], beam, d["maxlen"], eps, record=rec)
        d["ref"][key] = (seqs, lp, rec["margins"])
    return d["ref"][key]


def run(models, feats, fl, method, beam, maxlen, eps=None):
    ens = Ensemble(models)
    if eps is not None:
        ens.noise = {"eps": eps}
    out = ens(feats.cuda(), fl.copy(), method=method, beam_size=beam, max_length=maxlen)
    assert ens.noise is None
    return out["seqs"].cpu(), out["logprobs"].cpu()


# ------------------------------------------------------------------------------------------------ exact, no yardstick
@pytest.mark.parametrize("beam", [1, 3])
def test_one_member_is_the_single_model_beam_search(beam):
    """Replayed noise, then the same seed without replay (the generator-order contract: the same draws, and the generator
    left in the same state)."""
    d = case_data("m2_cnn10")
    m, feats, fl = d["models"][0], d["feats"], d["fl"]
    eps = noise("m2_cnn10", beam)[0]
    m.noise = dict(eps_beam=eps)
    want = m(feats.cuda(), fl.copy(), method="beam", beam_size=beam, max_length=MAXLEN)["seqs"].cpu()
    got, score = run([m], feats, fl, "beam", beam, MAXLEN, [eps])
    assert torch.equal(got, want)
    assert score.shape == (len(fl),) and bool(torch.isfinite(score).all()) and bool((score < 0).all())
    torch.manual_seed(77)
    want2 = m(feats.cuda(), fl.copy(), method="beam", beam_size=beam, max_length=MAXLEN)["seqs"].cpu()
    after = torch.get_rng_state()
    torch.manual_seed(77)
    got2, _ = run([m], feats, fl, "beam", beam, MAXLEN)
    assert torch.equal(got2, want2) and torch.equal(torch.get_rng_state(), after)
    if beam == 1:          # greedy is the beam-1 search up to and including each row's first <end>, then <end>
        g, lp = run([m], feats, fl, "greedy", 1, MAXLEN, [eps])
        assert lp.shape == (len(fl), MAXLEN)
        for a, b in zip(g.tolist(), want.tolist()):
            n = b.index(O.END_IDX) + 1 if O.END_IDX in b else MAXLEN
            assert a[:n] == b[:n] and a[n:] == [O.END_IDX] * (MAXLEN - n)


def test_one_member_beam_is_the_step_api_loop():
    """Ensemble([m]) against the reference's loop written with the sub-module step API and the two-kernel score route
    (acvae_row_logsoftmax_argmax + acvae_logprob_add), as test_model_gpu.py builds it for the single-model entry: beam 0's
    tokens and final score bit for bit, which pins the mix kernel's M = 1 identity end to end.  The small case: 5 ragged
    clips x beam 3 = 15 rows, top-k over 900 scores per clip."""
    beam, ml = 3, 12
    loop = _beam_call_vs_step_loop(V=300, beam=beam, ml=ml, feat_lens=[160, 150, 97, 64, 33], seed=3)
    seqs, score = run([loop["model"]], loop["feats"], loop["feat_lens"], "beam", beam, ml, [loop["eps"]])
    assert torch.equal(seqs, loop["seqs"][0::beam].cpu())
    assert torch.equal(score, loop["top_k"][0::beam].cpu())


@pytest.mark.parametrize("method,beam", [("greedy", 1), ("beam", 3)])
def test_three_copies_of_a_model_decode_as_one(method, beam):
    d = case_data("m2_cnn10")
    m, feats, fl = d["models"][1], d["feats"], d["fl"]
    eps = noise("m2_cnn10", beam)[1]
    one, lp1 = run([m], feats, fl, method, beam, MAXLEN, [eps])
    three, lp3 = run([m, copy.deepcopy(m), copy.deepcopy(m)], feats, fl, method, beam, MAXLEN, [eps, eps.clone(), eps.clone()])
    assert torch.equal(one, three)
    assert torch.equal(lp1, lp3)           # s = 3 exactly, s / 3 = 1: the mixture is the member bit for bit


# ------------------------------------------------------------------------------------------------ against the helper
def check_against_helper(name, method, beam):
    d = case_data(name)
    want, want_lp, margins = reference(name, method, beam)
    got, got_lp = run(d["models"], d["feats"], d["fl"], method, beam, d["maxlen"], noise(name, beam))
    keep = guarded(f"{name} {method} beam {beam}", margins)
    assert torch.equal(got[keep], want[keep]), (name, method, beam, [i for i in keep if not torch.equal(got[i], want[i])])
    T = d["maxlen"]
    if method == "greedy":
        # logprobs up to and including the row's <end>; the states drift over the steps, so the allowance is the token
        # rule's 20 x LP_TOL
        worst = 0.0
        for i in keep:
            row = want[i].tolist()
            n = row.index(O.END_IDX) + 1 if O.END_IDX in row else T
            worst = max(worst, float((got_lp[i, :n].double() - want_lp[i, :n]).abs().max()))
        print(f"{name} greedy: |logprobs - helper| max {worst:.2e} (bound {MARGIN:.1e})")
        assert worst <= MARGIN
    else:
        # beam 0's final score is a sum of T step log-probabilities, each within the same allowance
        err = float((got_lp[keep].double() - want_lp[keep]).abs().max())
        print(f"{name} beam {beam}: |final score - helper| max {err:.2e} (bound {T * MARGIN:.1e})")
        assert err <= T * MARGIN
    return got, want


@pytest.mark.parametrize("method,beam", [("greedy", 1), ("beam", 2), ("beam", 3)])
@pytest.mark.parametrize("name", ["m2_cnn10", "m3_mixed"])
def test_distinct_members_vs_helper(name, method, beam):
    """m2_cnn10: two seeds of Cnn10 at E = 64.  m3_mixed: Cnn10 at E = 64, Cnn14_16k at E = 64 and Cnn10 at E = 128, so that
    S (T / 16 and T / 32 frames) and E differ per member."""
    check_against_helper(name, method, beam)


@pytest.mark.parametrize("method,beam", [("greedy", 1), ("beam", 3)])
def test_members_of_unequal_widths_vs_helper(method, beam):
    """Two members with (E, H, A) = (64, 96, 160) and (64, 32, 96): acvae_ensemble_search gathers [H] and [E] state rows per
    member and sizes every member's scratch by its own widths.  With the helper alone on the CPU the smallest margin of any
    clip is 2.2e-3 (greedy) and 2.4e-3 (beam 3): no decision is left out at MARGIN = 2e-4."""
    import widths_util as W
    assert [m[1] for m in CASES["m2_widths"]["members"]] == W.ENSEMBLE_MEMBERS
    d = case_data("m2_widths")
    for st, (E, H, A) in zip(d["states"], W.ENSEMBLE_MEMBERS):
        assert st["decoder.attn.h2attn.weight"].shape == (A, E + H) and st["decoder.model.weight_hh_l0"].shape == (3 * H, H)
    check_against_helper("m2_widths", method, beam)


def test_greedy_rows_that_end_early_keep_end():
    """Member 0's <end> bias raised (the end_bump of test_fullsize_decode_gpu.model_and_state): some rows end before the last
    step; they hold <end> from there on, and what the kernels computed behind the end does not matter."""
    got, want = check_against_helper("m2_end_bump", "greedy", 1)
    early = [r for r in want.tolist() if O.END_IDX in r[:-1]]
    assert 0 < len(early)
    assert any(r.index(O.END_IDX) > 0 for r in early)
    for r in got.tolist():
        if O.END_IDX in r:
            assert r[r.index(O.END_IDX):] == [O.END_IDX] * (MAXLEN - r.index(O.END_IDX))


@pytest.mark.parametrize("method,beam", [("beam", 3), ("greedy", 1)])
def test_full_size_two_members_vs_helper(method, beam):
    """V = 5000, E = 512, two seeds of test_fullsize_gpu.build, 11 clips x beam 3 = 33 rows, T = 160, max_length 20."""
    check_against_helper("full_size", method, beam)


# ------------------------------------------------------------------------------------------------ ensemble_evaluate
def vocabulary():
    vocab = Vocabulary()
    for w in ["<pad>", "<start>", "<end>", "<unk>"] + [f"w{i}" for i in range(4, V)]:
        vocab.add_word(w)
    return vocab


def test_ensemble_evaluate_payload_csv_and_feat_lens(tmp_path):
    d = case_data("m2_cnn10")
    feats, fl = d["feats"], d["fl"]
    items = [(f"clip{i}", feats[i, :int(fl[i])].clone()) for i in range(len(fl))]
    vocab = vocabulary()
    kw = dict(method="beam", beam_size=2, max_length=MAXLEN)
    torch.manual_seed(3)
    path = tmp_path / "pred.json"
    payload = ensemble_evaluate(d["models"], items, vocab, caption_output=path, batch_size=3, **kw)
    # the same batches by hand: collate_fn([1]), no replication
    torch.manual_seed(3)
    ens, key2pred = Ensemble(d["models"]), {}
    for lo in range(0, len(items), 3):
        batch = collate_fn([1])(list(items[lo:lo + 3]))
        lens = np.array(batch[-1]).copy()
        seqs = ens(batch[1].cuda(), batch[-1], **kw)["seqs"]
        assert np.array_equal(batch[-1], lens)                   # the caller's feat_lens is left untouched
        collect_predictions(batch[0], seqs.cpu().numpy(), vocab, False, key2pred)
    want = predictions_payload(key2pred, False)
    assert payload == want and json.load(open(path)) == want
    assert [p["filename"] for p in payload["predictions"]] == [k for k, _ in items]
    torch.manual_seed(3)
    cpath = tmp_path / "pred.csv"
    ensemble_evaluate(Ensemble(d["models"]), items, vocab, caption_output=cpath, dcase_format=True, batch_size=3, **kw)
    rows = list(csv.reader(open(cpath, newline="")))
    assert rows[0] == ["file_name", "caption_predicted"]
    assert rows[1:] == [[p["filename"], p["caption"]] for p in want["predictions"]]
