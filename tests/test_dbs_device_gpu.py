"""GPU: diverse beam search as one library call (acvae_dbs_search / acvae_ensemble_dbs_search), everything bit-exact.

1. acvae_dbs_scores_sparse against acvae_dbs_scores fed the dense counts built on the host from the same tables.
2. acvae_dbs_advance and acvae_dbs_finish against the numpy twin (tests/dbs_util.py) on planted tables.
3. model(..., method="dbs") against dbs_impl="host" under the same seed: seqs, scores and lengths.
4. A spy on _lib.call: one acvae_dbs_search call and no step-API, score or top-k call in the device route.
5. Ensembles: M = 2 with members of different E against the host loop over M members; Ensemble([m]) against m;
   ensemble_evaluate(method="dbs").
6. The workspace contract of both entries (guarded scratch of exactly the declared bytes, garbage inside; one byte short),
   the G = 17 / bdash = 17 refusals, and the Python fallback to the host loop at group_size = 17."""
import numpy as np
import pytest
import torch

import acvae_oracle as O
import dbs_util as D
import widths_util as W
from acvae_amd import _lib
from acvae_amd.ensemble import Ensemble, ensemble_evaluate
from acvae_amd.evaluate import Vocabulary, collect_predictions, predictions_payload
from test_model_gpu import DBS_CASES
from ws_guard import FILLS, guarded, ws_guards  # noqa: F401  (the autouse fixture checks every guard after each test)

pytestmark = pytest.mark.gpu
V, ML, END = 44, 6, O.END_IDX
CASES = DBS_CASES + [dict(beam_size=16, group_size=1), dict(beam_size=5, group_size=5)]
CASE_IDS = [f"b{c.get('beam_size', 5)}g{c.get('group_size', 5)}" for c in CASES]
FEAT_LENS = [160, 97, 64]
st = _lib.current_stream


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same(a, b, what=""):
    a, b = bits(a), bits(b)
    assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b), what


# ------------------------------------------------------------------------------------------------ 1. the score op
def random_tables(rng, N, G, bdash, T, n_words, V):
    """Parents inside the row's clip, words from a small set (repeats inside a group and across groups): the tables of a
    search that ran to the end."""
    R = N * bdash
    base = (np.arange(R) // bdash) * bdash
    par = (base[None, None, :] + rng.integers(0, bdash, size=(G, T, R))).astype(np.int32)
    word = rng.integers(0, min(n_words, V), size=(G, T, R)).astype(np.int32)
    return par, word


@pytest.mark.parametrize("bdash", [1, 3, 16])
@pytest.mark.parametrize("Vv", [5, 257, 5000])
def test_sparse_penalty_scores_vs_dense_counts(Vv, bdash):
    N, G, T = 2, 16, 4
    R = N * bdash
    rng = np.random.default_rng(1000 * bdash + Vv)
    g_t = torch.Generator().manual_seed(bdash * 7 + Vv)
    logits = (torch.randn(R, Vv + 3, generator=g_t) * 3).cuda()         # ld > V
    prev = torch.randn(R, generator=g_t).cuda()
    for n_words in (3, 200):
        par, word = random_tables(rng, N, G, bdash, T, n_words, Vv)
        par_d, word_d = torch.from_numpy(par).cuda(), torch.from_numpy(word).cuda()
        for g in (0, 1, 15):
            for lt in (0, T - 1):
                for temp, lam in ((1.0, 0.5), (1.5, 0.8)):
                    counts = None
                    if g > 0:
                        c = D.dense_counts(par, word, N, bdash, T, Vv, g, lt)
                        assert c.sum() == N * g * bdash and (n_words > 3 or g * bdash <= 3 or c.max() > 1)
                        counts = torch.from_numpy(c).cuda()
                    want = torch.full((R, Vv), float("nan"), device="cuda")
                    got = torch.full((R, Vv), float("nan"), device="cuda")
                    _lib.call("acvae_dbs_scores", logits, Vv + 3, temp, counts, lam, prev, want, R, Vv, bdash if g > 0 else 0,
                              st())
                    _lib.call("acvae_dbs_scores_sparse", logits, Vv + 3, temp, lam, prev, got, par_d, word_d, N, bdash, T, Vv,
                              G, g, lt, st())
                    same(got, want, (Vv, bdash, n_words, g, lt, temp))
    # g = 0 takes no tables; prev may be NULL
    want, got = torch.empty(R, Vv, device="cuda"), torch.empty(R, Vv, device="cuda")
    _lib.call("acvae_dbs_scores", logits, Vv + 3, 1.0, None, 0.5, None, want, R, Vv, 0, st())
    _lib.call("acvae_dbs_scores_sparse", logits, Vv + 3, 1.0, 0.5, None, got, None, None, N, bdash, T, Vv, G, 0, 0, st())
    same(got, want)


def test_sparse_penalty_follows_the_parents_not_the_step_s_own_choice():
    """Group 0 chose the words [5, 6] at its step 0, but both of its beams after step 1 descend from row 1: group 1 at
    lt = 0 is penalised twice at word 6 and not at word 5."""
    Vv, bdash, T = 8, 2, 3
    par, word = np.zeros((2, T, 2), np.int32), np.zeros((2, T, 2), np.int32)
    word[0, 0] = [5, 6]
    par[0, 1] = [1, 1]
    logits = torch.zeros(2, Vv, device="cuda")
    got = torch.empty(2, Vv, device="cuda")
    _lib.call("acvae_dbs_scores_sparse", logits, Vv, 1.0, 1.0, None, got, torch.from_numpy(par).cuda(),
              torch.from_numpy(word).cuda(), 1, bdash, T, Vv, 2, 1, 0, st())
    base = float(-np.log(np.float32(Vv)))
    d = (got.cpu() - base).round().tolist()
    assert d[0] == d[1] == [0, 0, 0, 0, 0, 0, -2, 0]


# ------------------------------------------------------------------------------------------------ 2. advance and finish
def test_advance_op_vs_twin():
    rng = np.random.default_rng(5)
    for R in (1, 7, 300):
        for last in (0, 1):
            c = (rng.standard_normal(R) * 5).astype(np.float32)
            c[0] = -np.inf
            parent = rng.integers(0, R, size=R).astype(np.int64)
            word = rng.integers(0, 4, size=R).astype(np.int64)
            want = D.advance(c, parent, word, END, last)
            c_d = torch.from_numpy(c).cuda()
            par_o, word_o = (torch.full((R,), -7, dtype=torch.int32, device="cuda") for _ in range(2))
            rec_o = torch.zeros(R, device="cuda")
            _lib.call("acvae_dbs_advance", c_d, torch.from_numpy(parent).cuda(), torch.from_numpy(word).cuda(), par_o, word_o,
                      rec_o, END, last, R, st())
            same(par_o, want[0]), same(word_o, want[1])
            got_rec, want_rec = rec_o.cpu().numpy(), want[2]
            assert np.array_equal(np.isnan(got_rec), np.isnan(want_rec))
            same(np.nan_to_num(got_rec, nan=0.0), np.nan_to_num(want_rec, nan=0.0))
            same(c_d, want[3], (R, last))


def planted(N, G, bdash, T, seed):
    """Tables with records that tie in the fp64 key (c = -0.5 * (lt + 1) at several steps and beams), others that differ
    in the last bit of the quotient only, clip 1's records all from the last step, and a -inf record."""
    rng = np.random.default_rng(seed)
    R = N * bdash
    par, word = random_tables(rng, N, G, bdash, T, 9, 40)
    rec = np.full((G, T, R), D.NONE, np.float32)
    for g in range(G):
        for lt in range(T):
            for r in range(R):
                if r // bdash == 1 % N and N > 1:
                    continue
                u = rng.random()
                if u < 0.45:
                    rec[g, lt, r] = np.float32(-0.5 * (lt + 1))                       # key -0.5 exactly, whatever lt
                elif u < 0.48:
                    rec[g, lt, r] = np.nextafter(np.float32(-0.5 * (lt + 1)), np.float32(0))
                elif u < 0.6:
                    rec[g, lt, r] = np.float32(rng.standard_normal() * 3 - 1000.0)    # a retired row's record
        rec[g, T - 1, :] = (rng.standard_normal(R) * 2 - 3 - 2 * T).astype(np.float32)    # the last step records every row
    rec[0, T - 1, 0] = -np.inf
    return par, word, rec


@pytest.mark.parametrize("N,G,bdash,T", [(3, 2, 3, 6), (2, 16, 1, 4), (1, 1, 16, 20), (4, 3, 2, 1), (2, 5, 4, 33)])
@pytest.mark.parametrize("group_nbest", [1, 0])
def test_finish_op_vs_twin(N, G, bdash, T, group_nbest):
    par, word, rec = planted(N, G, bdash, T, seed=N * 100 + G)
    want = D.finish(par, word, rec, N, G, bdash, T, group_nbest, END)
    rows = G * (bdash if group_nbest else 1)
    seqs = torch.full((N, rows, T), -9, dtype=torch.long, device="cuda")
    scores = torch.zeros(N, rows, dtype=torch.float64, device="cuda")
    lengths = torch.full((N, rows), -9, dtype=torch.int32, device="cuda")
    _lib.call("acvae_dbs_finish", torch.from_numpy(par).cuda(), torch.from_numpy(word).cuda(), torch.from_numpy(rec).cuda(),
              seqs, scores, lengths, N, G, bdash, T, group_nbest, END, st())
    same(seqs, want[0]), same(scores, want[1]), same(lengths, want[2])
    if N > 1:
        assert (want[2][1] == T).all()                               # the clip whose records all come from the last step
    if bdash > 1 and group_nbest and T > 1:
        s = want[1][0]
        assert any(s[g * bdash + q] == s[g * bdash + q + 1] for g in range(G) for q in range(bdash - 1))   # ties were ranked


# ------------------------------------------------------------------------------------------------ 3. the whole search
_models, _inputs = {}, {}


def model_of(E=64, H=64, A=64, end_bump=0.0):
    key = (E, H, A, end_bump)
    if key not in _models:
        state = W.make_state(V, E, H, A, E)
        state["decoder.classifier.bias"] = state["decoder.classifier.bias"].clone()
        state["decoder.classifier.bias"][END] += float(end_bump)
        _models[key] = W.build_model(V, E, H, A, E, state).eval()
    return _models[key]


def inputs(feat_lens=tuple(FEAT_LENS)):
    if feat_lens not in _inputs:
        feats = torch.randn(len(feat_lens), max(feat_lens), 64, generator=torch.Generator().manual_seed(11))
        _inputs[feat_lens] = (feats.cuda(), np.array(feat_lens))
    return _inputs[feat_lens]


def device_vs_host(model, kw, feat_lens=tuple(FEAT_LENS), seed=50):
    feats, fl = inputs(feat_lens)
    out = []
    for impl in ("device", "host"):
        torch.manual_seed(seed)
        with torch.no_grad():
            out.append(model(feats, fl.copy(), method="dbs", max_length=ML, dbs_impl=impl, **kw))
    dev, host = out
    bdash = kw.get("beam_size", 5) // kw.get("group_size", 5)
    rows = kw.get("beam_size", 5) if kw.get("group_nbest", True) else kw.get("group_size", 5)
    assert dev["seqs"].shape == (len(fl), rows, ML) and dev["seqs"].is_cuda and dev["scores"].is_cuda
    assert dev["scores"].dtype == torch.float64 and dev["lengths"].dtype == torch.int32
    for k in ("seqs", "scores", "lengths"):
        same(dev[k], host[k], (k, kw))
    return dev


@pytest.mark.parametrize("kw", CASES, ids=CASE_IDS)
def test_search_vs_host_loop(kw):
    dev = device_vs_host(model_of(), kw)
    print(f"dbs {kw}: lengths {np.bincount(dev['lengths'].cpu().numpy().reshape(-1), minlength=ML + 1).tolist()}")


@pytest.mark.parametrize("bump", [2.0, 6.0])
@pytest.mark.parametrize("kw", CASES, ids=CASE_IDS)
def test_search_vs_host_loop_with_beams_that_end_early_and_repeatedly(kw, bump):
    """<end> bias raised by 6: nearly every beam ends at its first or second step, so all rows of a group retire and are
    expanded, end and are recorded again (scores near -1000 / length among the records); by 2: most beams end at once
    and some run to the last step."""
    dev = device_vs_host(model_of(end_bump=bump), kw, seed=51)
    lengths = dev["lengths"].cpu().numpy()
    print(f"dbs {kw} end bump {bump}: lengths {np.bincount(lengths.reshape(-1), minlength=ML + 1).tolist()}, "
          f"lowest score {float(dev['scores'].min()):.4g}")
    assert lengths.min() < ML                                         # beams did end early
    seqs = dev["seqs"].cpu().numpy()
    for n in range(seqs.shape[0]):                                    # behind its length a row holds <end> only
        for r in range(seqs.shape[1]):
            assert (seqs[n, r, lengths[n, r]:] == END).all()


def test_group_size_that_does_not_divide_beam_size_keeps_the_shape_of_the_host_loop():
    """beam_size 5 in 2 groups: bdash = 2, four beams and a fifth row of <end>, as the loop has always returned it."""
    for nbest in (True, False):
        dev = device_vs_host(model_of(end_bump=2.0), dict(beam_size=5, group_size=2, group_nbest=nbest), seed=55)
        if nbest:
            assert (dev["seqs"][:, 4] == END).all() and (dev["lengths"][:, 4] == 0).all()
            assert torch.isinf(dev["scores"][:, 4]).all() and (dev["lengths"][:, :4] > 0).all()


def test_search_vs_host_loop_at_unequal_widths():
    for kw in (CASES[0], CASES[1], CASES[5]):
        device_vs_host(model_of(64, 96, 160), kw, seed=52)
        device_vs_host(model_of(64, 96, 160, end_bump=6.0), kw, seed=53)


def test_search_vs_host_loop_with_the_split_attention():
    fl = (576, 560, 300)                                              # S = 18 > 16 frames: the split-over-frames attention
    feats, _ = inputs(fl)
    with torch.no_grad():
        S = model_of().encoder(feats, np.array(fl))["audio_embeds"].shape[1]
    assert S > 16 and _lib.call("acvae_attn_fwd_workspace_bytes", 3 * 2, 1, S, 64, 64) > 0
    for kw in (CASES[0], CASES[3]):
        device_vs_host(model_of(), kw, feat_lens=fl, seed=54)


# ------------------------------------------------------------------------------------------------ 4. the launch spy
class Spy:
    def __init__(self, monkeypatch):
        self.calls = []
        real = _lib.call

        def call(name, *args):
            self.calls.append((name, args))
            return real(name, *args)
        monkeypatch.setattr(_lib, "call", call)

    def names(self):
        return [n for n, _ in self.calls]

    def args_of(self, name):
        hits = [a for n, a in self.calls if n == name]
        assert len(hits) == 1, (name, len(hits))
        return hits[0]


STEP_CALLS = ("acvae_prior_step_fwd", "acvae_decoder_step_fwd", "acvae_dbs_scores", "acvae_topk_flat_batched", "acvae_topk_flat",
              "acvae_attn_precompute", "acvae_ensemble_mix")


def test_device_route_is_one_library_call(monkeypatch):
    spy = Spy(monkeypatch)
    feats, fl = inputs()
    torch.manual_seed(60)
    with torch.no_grad():
        model_of()(feats, fl.copy(), method="dbs", max_length=ML, **CASES[0])
    names = spy.names()
    assert names.count("acvae_dbs_search") == 1 and names.count("acvae_dbs_search_scratch_bytes") == 1
    assert not [n for n in names if n in STEP_CALLS], names
    spy.calls.clear()
    torch.manual_seed(60)
    with torch.no_grad():
        model_of()(feats, fl.copy(), method="dbs", max_length=ML, dbs_impl="host", **CASES[0])
    names = spy.names()
    assert "acvae_dbs_search" not in names and names.count("acvae_dbs_scores") == ML * CASES[0]["group_size"]


# ------------------------------------------------------------------------------------------------ 5. ensembles
def members():
    return [model_of(64, 96, 160, end_bump=2.0), model_of(128, 64, 64, end_bump=2.0)]


@pytest.mark.parametrize("kw", [CASES[0], CASES[1], CASES[5]], ids=[CASE_IDS[0], CASE_IDS[1], CASE_IDS[5]])
def test_ensemble_of_two_vs_host_loop_over_two_members(kw):
    models = members()
    assert models[0].decoder.embed_size != models[1].decoder.embed_size
    feats, fl = inputs()
    torch.manual_seed(70)
    got = Ensemble(models)(feats, fl.copy(), method="dbs", max_length=ML, **kw)
    torch.manual_seed(70)
    want = D.host_loop(models, feats, fl, ML, kw.get("beam_size", 5), kw.get("group_size", 5), kw.get("diversity_lambda", 0.5),
                       kw.get("temperature", 1.0), kw.get("group_nbest", True))
    for k, w in zip(("seqs", "scores", "lengths"), want):
        same(got[k], w, (k, kw))
    print(f"ensemble dbs {kw}: lengths {np.bincount(want[2].reshape(-1), minlength=ML + 1).tolist()}")
    # the mixture is not one member's search
    torch.manual_seed(70)
    alone = D.host_loop(models[:1], feats, fl, ML, kw.get("beam_size", 5), kw.get("group_size", 5),
                        kw.get("diversity_lambda", 0.5), kw.get("temperature", 1.0), kw.get("group_nbest", True))
    assert not np.array_equal(bits(alone[1]), bits(want[1]))


@pytest.mark.parametrize("kw", [CASES[0], CASES[3]], ids=[CASE_IDS[0], CASE_IDS[3]])
def test_ensemble_of_one_is_the_member(kw, monkeypatch):
    m = model_of(end_bump=2.0)
    feats, fl = inputs()
    torch.manual_seed(71)
    with torch.no_grad():
        want = m(feats, fl.copy(), method="dbs", max_length=ML, **kw)
    spy = Spy(monkeypatch)
    torch.manual_seed(71)
    got = Ensemble([m])(feats, fl.copy(), method="dbs", max_length=ML, **kw)
    for k in ("seqs", "scores", "lengths"):
        same(got[k], want[k], k)
    assert spy.names().count("acvae_ensemble_dbs_search") == 1 and not [n for n in spy.names() if n in STEP_CALLS]
    torch.manual_seed(71)                                             # the CPU generator is consumed alike
    with torch.no_grad():
        m(feats, fl.copy(), method="dbs", max_length=ML, **kw)
    a = torch.rand(4)
    torch.manual_seed(71)
    Ensemble([m])(feats, fl.copy(), method="dbs", max_length=ML, **kw)
    assert torch.equal(a, torch.rand(4))


def vocabulary():
    vocab = Vocabulary()
    for w in ["<pad>", "<start>", "<end>", "<unk>"] + [f"w{i}" for i in range(4, V)]:
        vocab.add_word(w)
    assert vocab.word2idx["<end>"] == END and vocab.word2idx["<start>"] == O.START_IDX
    return vocab


def test_ensemble_evaluate_writes_every_beam_as_a_caption(tmp_path):
    import json
    from acvae_amd.batch import collate_fn
    models = members()
    feats, fl = inputs()
    feats = feats.cpu()
    items = [(f"clip{i}", feats[i, :int(fl[i])].clone()) for i in range(len(fl))]
    vocab = vocabulary()
    kw = dict(method="dbs", beam_size=4, group_size=2, diversity_lambda=0.7, max_length=ML)
    torch.manual_seed(72)
    path = tmp_path / "pred.json"
    payload = ensemble_evaluate(models, items, vocab, caption_output=path, batch_size=2, **kw)
    torch.manual_seed(72)
    ens, key2pred = Ensemble(models), {}
    for lo in range(0, len(items), 2):
        batch = collate_fn([1])(list(items[lo:lo + 2]))
        seqs = ens(batch[1].cuda(), batch[-1], **kw)["seqs"]
        assert seqs.shape[1:] == (4, ML)
        collect_predictions(batch[0], seqs.cpu().numpy(), vocab, False, key2pred)
    want = predictions_payload(key2pred, False)
    assert payload == want and json.load(open(path)) == want
    assert all(len(p["captions"]) == 4 for p in payload["predictions"])
    assert [p["filename"] for p in payload["predictions"]] == [k for k, _ in items]


# ------------------------------------------------------------------------------------------------ 6. the workspace contract
def captured_call(monkeypatch, ensemble, kw):
    """The arguments of the one library call behind a forward, and its outputs."""
    spy = Spy(monkeypatch)
    feats, fl = inputs()
    torch.manual_seed(80)
    with torch.no_grad():
        if ensemble:
            out = Ensemble(members())(feats, fl.copy(), method="dbs", max_length=ML, **kw)
        else:
            out = model_of(end_bump=2.0)(feats, fl.copy(), method="dbs", max_length=ML, **kw)
    name = "acvae_ensemble_dbs_search" if ensemble else "acvae_dbs_search"
    args = list(spy.args_of(name))
    monkeypatch.undo()
    keep = None
    if ensemble:             # the call's host tables lived inside Ensemble.forward: the members' parameter tables and widths again
        import ctypes
        models = members()
        tables = [_lib.ptr_table(m._text_table()) for m in models]
        params = (ctypes.c_void_p * len(models))(*[ctypes.cast(t, ctypes.c_void_p).value for t in tables])
        S = [mem.shape[1] for mem in args[1]]
        dims = [np.ascontiguousarray(d, dtype=np.int32) for d in
                (S, [m.decoder.embed_size for m in models], [m.decoder.model.hidden_size for m in models],
                 [m.decoder.attn.attn_size for m in models])]
        args[0] = params
        args[4:8] = [d.ctypes.data for d in dims]
        keep = (tables, dims)
    return name, args, out, (19 if ensemble else 18), keep


@pytest.mark.parametrize("ensemble", [False, True], ids=["one", "ensemble"])
def test_workspace_contract(ensemble, monkeypatch):
    kw = CASES[0]
    name, args, out, o, _keep = captured_call(monkeypatch, ensemble, kw)
    sb = args[o + 4]
    bytes_args = ([args[8]] if ensemble else []) + list(args[11:15] if ensemble else args[6:10])
    bytes_args += list(args[4:8] if ensemble else args[10:14]) + [args[15] if ensemble else args[14]]
    assert sb == _lib.call(name + "_scratch_bytes", *bytes_args) and args[o + 3].numel() >= sb
    for fill in FILLS:
        ws = guarded(sb, fill, what=f"{name} fill {fill:#x}")
        fresh = [torch.full_like(out["seqs"], -9), torch.full_like(out["scores"], -9.0), torch.full_like(out["lengths"], -9)]
        call = list(args)
        call[o:o + 5] = fresh + [ws.view, sb]
        _lib.call(name, *call)
        torch.cuda.synchronize()
        for k, got in zip(("seqs", "scores", "lengths"), fresh):
            same(got, out[k], (name, fill, k))
        ws.check()
    # one byte short: refused before any launch, nothing written
    ws = guarded(sb - 1, 0xFF, what=f"{name} one byte short")
    fresh = [torch.full_like(out["seqs"], -9), torch.full_like(out["scores"], -9.0), torch.full_like(out["lengths"], -9)]
    call = list(args)
    call[o:o + 5] = fresh + [ws.view, sb - 1]
    with pytest.raises(RuntimeError, match="ACVAE_EWORKSPACE"):
        _lib.call(name, *call)
    torch.cuda.synchronize()
    assert (fresh[0] == -9).all() and (fresh[1] == -9.0).all() and (fresh[2] == -9).all()
    assert (ws.view == 0xFF).all()
    ws.check()
    # G = 17 and bdash = 17: refused, nothing written (the scratch is more than either would need were it allowed)
    gi = 12 if ensemble else 7
    for at in (gi, gi + 1):
        call = list(args)
        call[o:o + 3] = fresh
        call[at] = 17
        with pytest.raises(RuntimeError, match="ACVAE_EUNSUPPORTED"):
            _lib.call(name, *call)
        bad = list(bytes_args)
        bad[(2 if ensemble else 1) + (at - gi)] = 17
        assert _lib.call(name + "_scratch_bytes", *bad) == -1
    torch.cuda.synchronize()
    assert (fresh[0] == -9).all() and (fresh[1] == -9.0).all() and (fresh[2] == -9).all()


def test_group_size_17_falls_back_to_the_host_loop(monkeypatch):
    spy = Spy(monkeypatch)
    feats, fl = inputs()
    m = model_of(end_bump=2.0)
    kw = dict(beam_size=17, group_size=17, max_length=4)
    torch.manual_seed(81)
    with torch.no_grad():
        got = m(feats, fl.copy(), method="dbs", **kw)
    assert "acvae_dbs_search" not in spy.names() and spy.names().count("acvae_dbs_scores") == 4 * 17
    torch.manual_seed(81)
    with torch.no_grad():
        want = m(feats, fl.copy(), method="dbs", dbs_impl="host", **kw)
    for k in ("seqs", "scores", "lengths"):
        same(got[k], want[k], k)
    assert got["seqs"].shape == (3, 17, 4)
    with pytest.raises(ValueError, match="at most 16"):
        Ensemble([m])(feats, fl.copy(), method="dbs", **kw)
