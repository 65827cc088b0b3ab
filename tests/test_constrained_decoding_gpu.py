"""GPU: constrained decoding (repetition_penalty, no_repeat_ngram_size, min_length, suppress_tokens).

1. acvae_constrain_logits alone against the numpy twin of tests/constrain_util.py, bit for bit as int32 views (-inf
   included, the gaps between the rows and every element the twin leaves alone too).
2. The stepwise driver (greedy / "sample" / "gumbel" / "sample" with top_k) checked from its own outputs: the returned
   logits are the twin of the unconstrained rows, the words are the method's selection on them.
3. acvae_beam_search_constrained / acvae_ensemble_search_constrained against host loops over the step API with the twin
   applied to every member's downloaded logits at every step.
4. evaluate() / rollout_shared_encoder() end to end, and the refusals in front of the first launch."""
import numpy as np
import pytest
import torch

import acvae_oracle as O
import constrain_util as CU
import truncate_util as TU
from acvae_amd import _lib
from acvae_amd import evaluate as EV
from acvae_amd.encoder import ptr_table
from acvae_amd.ensemble import Ensemble
from test_fullsize_decode_gpu import LP_TOL
from test_model_gpu import build_model

pytestmark = pytest.mark.gpu
NEG_INF = np.float32(-np.inf)


def st():
    return _lib.current_stream()


def ids_arg(ids):
    arr = np.ascontiguousarray(ids, dtype=np.int32)
    return arr, (arr.ctypes.data if len(ids) else None), len(ids)


# ------------------------------------------------------------------------------------------------ 1. the kernel alone
HT = 133                                  # history row stride (> the longest t)
STEPS = (0, 1, 19, 64, 65, 130)           # 64 / 65 / 130 step past one lane per position


def planted_histories(R, V, end_idx, rng):
    """Row r's kind is r % 8: one word repeated; a period-2 and a period-3 cycle; blocks "a b c x" whose last word
    changes (the suffix occurs many times with different followers); end_idx, suppressed words and words outside [0, V)
    inside the history; a small alphabet (many repeats); the whole vocabulary (few); a copy of row 0 with another word."""
    h = np.zeros((R, HT), np.int64)
    for r in range(R):
        kind, i = r % 8, np.arange(HT)
        if kind == 0:
            h[r] = 5
        elif kind == 1:
            h[r] = np.where(i % 2 == 0, 7, 8)
        elif kind == 2:
            h[r] = 9 + i % 3
        elif kind == 3:
            h[r] = np.where(i % 4 == 3, 15 + (i // 4) % 6, 12 + i % 4)
        elif kind == 4:
            h[r] = rng.integers(0, 8, HT)
            h[r, 2::7] = end_idx
            h[r, 3::11] = V                # outside the vocabulary: skipped
            h[r, 5::13] = -1
            h[r, 6::17] = V + (1 << 33)
        elif kind == 5:
            h[r] = rng.integers(20, 26, HT)
        elif kind == 6:
            h[r] = rng.integers(0, V, HT)
        else:
            h[r] = 6
    return h


def constrain_call(x, ld, hist, t, R, V, end_idx, theta, n, m, sup):
    arr, ptr, cnt = ids_arg(sup)
    _lib.call("acvae_constrain_logits", x, ld, hist, HT, t, R, V, end_idx, float(theta), n, m, ptr, cnt, st())
    torch.cuda.synchronize()               # (the host list is read before the call returns; arr lives until here anyway)
    return arr


@pytest.mark.parametrize("V", [40, 257, 5000])
@pytest.mark.parametrize("R", [1, 3, 70])
def test_kernel_equals_the_twin_bit_for_bit(V, R):
    ld, end_idx = V + 3, 2
    rng = np.random.default_rng(1000 * V + R)
    hist = planted_histories(R, V, end_idx, rng)
    rows = (rng.standard_normal((R, V)) * 2).astype(np.float32)
    rows[:, 5] = 0.0                      # +0.0, -0.0 and an existing -inf at words the histories hold, and beside them
    rows[:, 7] = -0.0
    rows[:, 9] = NEG_INF
    rows[:, 12] = np.abs(rows[:, 12]) + 0.5
    rows[:, 30] = -0.0
    rows[:, 31] = NEG_INF
    host = np.full(R * ld, 77.0, np.float32)
    host.reshape(R, ld)[:, :V] = rows
    hist_d = torch.from_numpy(hist).cuda()
    checked = 0
    for n in (1, 2, 3, 4):
        for t in sorted({t for t in STEPS + (n - 2, n - 1, n) if t >= 0}):
            combos = [(1.3, n, t + 1, (0, 1, 3, 8, end_idx)), (1.0, n, 0, ()), (1.0, 0, t, ())]
            if n == 1:
                combos += [(0.7, 0, 0, ()), (1.3, 0, 0, ()), (1.0, 0, 0, (4, 39, 0)), (1.0, 0, t + 1, ())]
            for theta, nn, m, sup in combos:
                x = torch.from_numpy(host).cuda()
                constrain_call(x, ld, hist_d, t, R, V, end_idx, theta, nn, m, sup)
                want = host.copy().reshape(R, ld)
                for r in range(R):
                    want[r, :V] = CU.constrain_row(rows[r], hist[r], t, end_idx, theta, nn, m, sup)
                got = x.cpu().numpy().reshape(R, ld)
                same = got.view(np.int32) == want.view(np.int32)
                assert same.all(), (n, t, theta, nn, m, sup, np.argwhere(~same)[:5], got[~same][:5], want[~same][:5])
                checked += 1
    # all off: nothing is launched, the buffer is untouched
    x = torch.from_numpy(host).cuda()
    constrain_call(x, ld, hist_d, 64, R, V, end_idx, 1.0, 0, 0, ())
    assert np.array_equal(x.cpu().numpy().view(np.int32), host.view(np.int32))
    assert checked >= 60


def test_kernel_planted_cases_do_what_they_are_planted_for():
    """The planted rows are not vacuous: the repeated word is banned by n = 1 and penalised once; the period-2 row bans its
    next word for n = 2 and nothing for n = 4 at t = 2; the block row bans several followers of one suffix; a word both
    penalised and banned ends at -inf; rows of one launch differ."""
    V, R, end_idx = 40, 8, 2
    hist = planted_histories(R, V, end_idx, np.random.default_rng(3))
    rows = np.tile(np.linspace(1.0, 4.0, V, dtype=np.float32), (R, 1))
    x = torch.from_numpy(rows.copy()).cuda()
    constrain_call(x, V, torch.from_numpy(hist).cuda(), 65, R, V, end_idx, 2.0, 4, 0, ())
    got = x.cpu().numpy()
    assert got[0, 5] == NEG_INF and np.isneginf(got[0]).sum() == 1              # "5 5 5" + 5 exists
    assert got[7, 6] == NEG_INF and got[7, 5] == rows[7, 5]                     # another row, another word
    assert got[1, 8] == NEG_INF and got[1, 7] == rows[1, 7] / np.float32(2.0)   # t = 65: h[64] = 7, so 8 would repeat
    banned3 = set(np.flatnonzero(np.isneginf(got[3])).tolist())
    assert len(banned3) >= 1 and banned3 <= set(range(12, 21))
    x = torch.from_numpy(rows.copy()).cuda()
    constrain_call(x, V, torch.from_numpy(hist).cuda(), 67, R, V, end_idx, 1.0, 4, 0, ())
    assert set(np.flatnonzero(np.isneginf(x.cpu().numpy()[3])).tolist()) == set(range(15, 21))   # six followers of "12 13 14"
    x = torch.from_numpy(rows.copy()).cuda()
    constrain_call(x, V, torch.from_numpy(hist).cuda(), 2, R, V, end_idx, 1.0, 4, 0, ())
    assert not np.isneginf(x.cpu().numpy()).any()                               # t < n - 1


# ------------------------------------------------------------------------------------------------ 2. the stepwise driver
MV, ME, ML, MB = 40, 64, 12, 3
FULL = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_length=4, suppress_tokens=[0, 1, 3])
CONTROL_SETS = (FULL, dict(repetition_penalty=1.3), dict(no_repeat_ngram_size=2), dict(min_length=4),
                dict(suppress_tokens=[0, 1, 3]))
METHODS = {"greedy": dict(method="greedy"), "sample": dict(method="sample", temp=1.2),
           "gumbel": dict(method="gumbel", temp=0.8), "sample_top_k": dict(method="sample", temp=1.2, top_k=5)}

_small = {}


def small(end_bump=0.0):
    """The small model (closed-form weights, V = 40, E = 64) on the GPU, its features, and the bias of <end> moved."""
    if end_bump not in _small:
        state = O.closed_form_state(O.state_shapes(MV, ME, ME, None, ME, 512))
        state["decoder.classifier.bias"] = state["decoder.classifier.bias"].clone()
        state["decoder.classifier.bias"][O.END_IDX] += end_bump
        feats, _, feat_lens, _ = O.synthetic_batch(MB, 64, MV, 6, seed=5, ragged=False)
        _small[end_bump] = (build_model(MV, ME, state).eval(), feats.cuda(), feat_lens)
    return _small[end_bump]


def planted_noise(method, seed, N=MB):
    g = torch.Generator().manual_seed(seed)
    eps = torch.randn(ML, N, ME, generator=g)
    if method == "greedy":
        return eps, None
    if method == "gumbel":
        return eps, -torch.log(-torch.log(torch.rand(ML, N, MV, generator=g) + 1e-20) + 1e-20)
    return eps, torch.empty(ML, N, MV).exponential_(1, generator=g)


def infer(model, feats, lens, noise, **kw):
    model.noise = dict(eps_p=noise[0]) if noise[1] is None else dict(eps_p=noise[0], sample_noise=noise[1])
    with torch.no_grad():
        return model(feats, lens.copy(), max_length=ML, **kw)


def controls_of(kw):
    return (kw.get("repetition_penalty", 1.0), kw.get("no_repeat_ngram_size", 0), kw.get("min_length", 0),
            tuple(kw.get("suppress_tokens", ())))


def caption(row, end_idx):
    row = [int(w) for w in row]
    return row[:row.index(end_idx)] if end_idx in row else row


def check_properties(seqs, end_idx, kw):
    theta, n, m, sup = controls_of(kw)
    for row in seqs:
        words = caption(row, end_idx)
        if n > 0:
            assert not CU.repeats_ngram(words, n), (n, words)
        assert not set(words) & set(sup), (sup, words)
        assert len(words) >= min(m, len(row)), (m, words)                    # no <end> before step m


def check_run(model, out, mkw, kw, noise):
    """(a) - (e) of the module docstring's part 2 for one run, every row and step."""
    theta, n, m, sup = controls_of(kw)
    end_idx, N = int(model.end_idx), out["seqs"].shape[0]
    logits, seqs, slp = (out[k].cpu().numpy() for k in ("logits", "seqs", "sampled_logprobs"))
    assert logits.shape == (N, ML, MV) and seqs.shape == (N, ML)
    W, b = model.decoder.classifier.weight.detach().contiguous(), model.decoder.classifier.bias.detach().contiguous()
    outputs = out["outputs"].contiguous()
    H = outputs.shape[2]
    raw = torch.full((N, ML, MV), 55.0, device="cuda")
    code = {"greedy": 0, "gumbel": TU.GUMBEL, "sample": TU.MULTINOMIAL}[mkw["method"]]
    temp, top_k = float(mkw.get("temp", 1.0)), int(mkw.get("top_k", 0))
    for t in range(ML):
        # (d) the unconstrained rows, by the driver's own product: same kernel, same shape, same strides
        _lib.call("acvae_gemm_nt", outputs[:, t], ML * H, W, H, b, raw[:, t], ML * MV, N, MV, H, 0, st())
        live = ~(seqs[:, :t] == end_idx).any(1)
        if code:                              # (b) the stand-alone selection kernel on the returned rows and the step's noise
            w = torch.empty(N, dtype=torch.long, device="cuda")
            x = out["logits"][:, t].contiguous()
            z = noise[1][t].contiguous().cuda()
            if top_k:
                _lib.call("acvae_sample_next_word_truncated", x, MV, 0, z, MV, 0, code, temp, w, None, 1, 0, N, 1, MV, top_k,
                          1.0, None, st())
            else:
                _lib.call("acvae_sample_next_word", x, MV, 0, z, MV, 0, code, temp, w, None, 1, 0, N, 1, MV, st())
            pick = w.cpu().numpy()
        else:
            pick = logits[:, t].argmax(-1)    # numpy: the first maximum
        raw_t = raw[:, t].cpu().numpy()
        for r in range(N):
            row = logits[r, t]
            bans = CU.ban_set(seqs[r], t, end_idx, n, m, sup, MV)
            assert set(np.flatnonzero(np.isneginf(row)).tolist()) == bans, (r, t)                       # (a)
            want = CU.constrain_row(raw_t[r], seqs[r], t, end_idx, theta, n, m, sup)
            assert np.array_equal(row.view(np.int32), want.view(np.int32)), (r, t, np.abs(row - want).max())   # (d)
            if not live[r]:
                assert seqs[r, t] == end_idx
                continue
            assert seqs[r, t] == pick[r], (r, t, int(seqs[r, t]), int(pick[r]))                         # (b)
            assert row[seqs[r, t]] > NEG_INF
            if top_k:
                order = TU.stable_order(row)
                assert int(np.flatnonzero(order == seqs[r, t])[0]) < top_k
            lp = torch.log_softmax(torch.from_numpy(row).double(), -1)[seqs[r, t]]
            assert abs(float(lp) - float(slp[r, t])) < 1e-5, (r, t)                                     # (c)
    check_properties(seqs, end_idx, kw)                                                                 # (e)


@pytest.mark.parametrize("name", list(METHODS))
def test_stepwise_driver_from_its_own_outputs(name):
    """(d) held bit for bit: the classifier product of a step is the 32x32-tile kernel without a K split with and without the
    driver's workspace (K = 64), so acvae_gemm_nt on outputs[:, t] with the driver's strides reproduces the unconstrained
    row exactly, and the returned row is its twin."""
    model, feats, lens = small(-4.0)
    mkw = METHODS[name]
    for i, kw in enumerate(CONTROL_SETS):
        noise = planted_noise(mkw["method"], 40 + i)
        out = infer(model, feats, lens, noise, **mkw, **kw)
        check_run(model, out, mkw, kw, noise)
        assert ("kept" in out) == ("top_k" in mkw)


def test_the_constraint_bites_where_the_plain_run_repeats():
    """Prior-free: the unconstrained greedy run of the same model on the same noise repeats a bigram in every row (asserted
    first, so the test cannot pass vacuously); with no_repeat_ngram_size = 2 none does, and the two runs agree up to the
    first step at which the plain run completes a repeated bigram."""
    model, feats, lens = small(-4.0)
    noise = planted_noise("greedy", 7)
    end = int(model.end_idx)
    plain = infer(model, feats, lens, noise, method="greedy")["seqs"].cpu().numpy()
    got = infer(model, feats, lens, noise, method="greedy", no_repeat_ngram_size=2)["seqs"].cpu().numpy()
    for r in range(MB):
        words = caption(plain[r], end)
        assert CU.repeats_ngram(words, 2), ("the plain run must repeat a bigram", words)
        first = next(t for t in range(len(words) + 1) if CU.repeats_ngram(words[:t], 2)) - 1
        assert list(got[r, :first]) == words[:first] and got[r, first] != plain[r, first]
        assert not CU.repeats_ngram(caption(got[r], end), 2)


def test_min_length_bites_where_the_plain_run_ends_early():
    model, feats, lens = small(6.0)
    noise = planted_noise("greedy", 8)
    end = int(model.end_idx)
    plain = infer(model, feats, lens, noise, method="greedy")["seqs"].cpu().numpy()
    assert all(len(caption(row, end)) < 4 for row in plain), plain
    got = infer(model, feats, lens, noise, method="greedy", min_length=4)["seqs"].cpu().numpy()
    assert all(len(caption(row, end)) >= 4 for row in got), got


def test_all_off_keywords_are_the_unconstrained_call_bit_for_bit():
    model, feats, lens = small(-4.0)
    off = dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, suppress_tokens=())
    calls = []
    real = _lib.call
    for name, mkw in METHODS.items():
        noise = planted_noise(mkw["method"], 21)
        a = infer(model, feats, lens, noise, **mkw)
        _lib.call = lambda *x: (calls.append(x[0]), real(*x))[1]
        try:
            b = infer(model, feats, lens, noise, **mkw, **off)
        finally:
            _lib.call = real
        for key in ("seqs", "logits", "sampled_logprobs", "outputs", "p_z") + (("kept",) if "top_k" in mkw else ()):
            assert torch.equal(a[key], b[key]), (name, key)
    assert "acvae_decode_fwd_constrained" not in calls                      # the entries of today, not a new one
    assert {"acvae_decode_fwd_sampled", "acvae_decode_fwd_truncated"} <= set(calls)


# ------------------------------------------------------------------------------------------------ 3. beam and ensemble
SV, SML = 50, 10
SEARCH = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_length=3, suppress_tokens=[0, 1, 3])
_search = {}


def search_case():
    if not _search:
        models = []
        for seed, bump in ((11, -1.0), (12, 0.5)):
            torch.manual_seed(seed)
            m = build_model(SV, 64).eval()
            with torch.no_grad():
                m.decoder.classifier.bias[O.END_IDX] += bump
            models.append(m)
        feats, _, fl, _ = O.synthetic_batch(4, 96, SV, 7, seed=21, ragged=True)
        _search.update(models=models, feats=feats.cuda(), fl=fl, loops={})
    return _search


def search_noise(N, beam, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(N, SML, beam, 64, generator=g) for _ in range(2)]


@torch.no_grad()
def host_loop(models, feats, fl, eps, beam, greedy, kw):
    """The search as a host loop over the step API: per step every member's prior and decoder step, the twin on the member's
    downloaded logits (history: the row's own words so far), acvae_ensemble_mix on the edited rows, then the greedy pick or
    the flat top-k with the states AND the histories gathered by parent.  -> seqs, scores, steps at which parents permute."""
    theta, n, m, sup = controls_of(kw)
    on = bool(kw)
    M, V = len(models), SV
    end, start = int(models[0].end_idx), int(models[0].start_idx)
    mem, lens, state, hid, lz = [], [], [], [], []
    for mod in models:
        enc = mod.encoder(feats, np.asarray(fl).copy())
        mm = mod._projected_memory(enc)
        mem.append(mm.repeat_interleave(beam, 0).contiguous())
        lens.append(torch.as_tensor(enc["audio_embeds_lens"]).repeat_interleave(beam))
    N = feats.shape[0]
    R = N * beam
    for mod in models:
        state.append(mod.decoder.init_hidden(R).cuda())
        hid.append(mod.pnet.init_hidden(R, "cuda"))
        lz.append(torch.zeros(R, mod.decoder.embed_size, device="cuda"))          # (the members' own embed widths)
    w = torch.full((R,), start, dtype=torch.long, device="cuda")
    hist = np.zeros((R, 0), np.int64)
    top_k = torch.zeros(R, device="cuda")
    seqs = torch.full((R, SML), end, dtype=torch.long)
    scores = torch.zeros(R, SML)
    done = torch.zeros(R, dtype=torch.bool)
    ld = np.full(M, V, np.int64)
    permuted = []
    for t in range(SML):
        edited, new = [], []
        for k, mod in enumerate(models):
            pn = mod.pnet(w.unsqueeze(1), mem[k], hid[k], lz[k], lens[k], eps=eps[k][:, t].reshape(R, -1))
            dn = mod.decoder(word=w.unsqueeze(1), state=state[k], enc_mem=mem[k], enc_mem_lens=lens[k], z=pn["z"])
            x = dn["logits"].squeeze(1).contiguous()
            if on:
                h = x.cpu().numpy()
                x = torch.from_numpy(np.stack([CU.constrain_row(h[r], hist[r], t, end, theta, n, m, sup)
                                               for r in range(R)])).cuda()
            edited.append(x)
            new.append((dn["state"], pn["hiddens_state"], pn["z"]))
        if greedy:
            arg = torch.empty(R, dtype=torch.long, device="cuda")
            best = torch.empty(R, device="cuda")
            _lib.call("acvae_ensemble_mix", ptr_table(edited), ld.ctypes.data, M, None, None, 0, arg, best, 1, R, V, st())
            pick = torch.where(done, torch.full((R,), end, dtype=torch.long), arg.cpu())
            seqs[:, t], scores[:, t] = pick, best.cpu()
            done = done | (pick == end)
            w = pick.cuda()
            hist = np.concatenate([hist, pick.numpy()[:, None]], 1)
            for k in range(M):
                state[k], hid[k], lz[k] = new[k][0], new[k][1], new[k][2]
            continue
        sc = torch.empty(R, V, device="cuda")
        vals = torch.empty(R, device="cuda")
        idx, prev, w = (torch.empty(R, dtype=torch.long, device="cuda") for _ in range(3))
        _lib.call("acvae_ensemble_mix", ptr_table(edited), ld.ctypes.data, M, top_k, sc, V, None, None, 0, R, V, st())
        _lib.call("acvae_topk_flat_batched", sc, beam * V, beam * V, beam, V, vals, idx, prev, w, N, beam, st())
        top_k = vals
        p = prev.cpu().numpy()
        if t > 0 and not np.array_equal(p, np.arange(R)):
            permuted.append(t)
        hist = np.concatenate([hist[p], w.cpu().numpy()[:, None]], 1)
        for k in range(M):
            state[k] = new[k][0][:, prev].contiguous()
            hid[k] = (new[k][1][0][:, prev].contiguous(), new[k][1][1][:, prev].contiguous())
            lz[k] = new[k][2][prev].contiguous()
    if greedy:
        return seqs, scores, permuted
    return torch.from_numpy(hist)[0::beam], top_k.cpu()[0::beam], permuted


def ensemble_run(models, feats, fl, method, beam, eps, **kw):
    ens = Ensemble(models)
    ens.noise = {"eps": eps}
    out = ens(feats, np.asarray(fl).copy(), method=method, beam_size=beam, max_length=SML, **kw)
    return out["seqs"].cpu(), out["logprobs"].cpu()


@pytest.mark.parametrize("kw", [SEARCH, dict(no_repeat_ngram_size=1), dict(repetition_penalty=0.8)],
                         ids=["all", "ngram1", "penalty"])
def test_ensemble_greedy_equals_the_host_loop(kw):
    c = search_case()
    eps = search_noise(4, 1, 31)
    want, lp, _ = host_loop(c["models"], c["feats"], c["fl"], eps, 1, True, kw)
    got, glp = ensemble_run(c["models"], c["feats"], c["fl"], "greedy", 1, eps, **kw)
    assert torch.equal(got, want)
    live = torch.from_numpy(np.stack([~(want[:, :t] == O.END_IDX).any(1).numpy() for t in range(SML)], 1))
    assert float((glp - lp).abs()[live].max()) <= LP_TOL
    check_properties(got.numpy(), O.END_IDX, kw)
    if "no_repeat_ngram_size" in kw:                                         # the bans change the captions
        plain, _ = ensemble_run(c["models"], c["feats"], c["fl"], "greedy", 1, eps)
        assert not torch.equal(plain, got)


@pytest.mark.parametrize("kw", [SEARCH, dict(no_repeat_ngram_size=3, repetition_penalty=1.5)], ids=["all", "ngram3"])
def test_ensemble_beam_equals_the_host_loop(kw):
    """Beam 3, two members: the histories follow their parents - the loop reports steps at which the parents are not the
    identity, where a history left in place would ban the wrong words."""
    c = search_case()
    eps = search_noise(4, 3, 32)
    want, score, permuted = host_loop(c["models"], c["feats"], c["fl"], eps, 3, False, kw)
    assert len(permuted) >= 2, permuted
    got, gscore = ensemble_run(c["models"], c["feats"], c["fl"], "beam", 3, eps, **kw)
    assert torch.equal(got, want)
    assert float((gscore - score).abs().max()) <= LP_TOL
    # beam 0 holds no repeated n-gram, no suppressed word and no early <end> (beams do not finish: the words behind an
    # <end> are words of the same row, which the rules cover alike)
    n, sup, m = kw.get("no_repeat_ngram_size", 0), set(kw.get("suppress_tokens", ())), kw.get("min_length", 0)
    for row in got.tolist():
        assert not CU.repeats_ngram(row, n) and not set(row) & sup and O.END_IDX not in row[:m]


def test_single_model_beam_search_equals_the_loop_and_the_one_member_ensemble():
    c = search_case()
    m = c["models"][0]
    eps = search_noise(4, 3, 33)[:1]
    want, _, permuted = host_loop([m], c["feats"], c["fl"], eps, 3, False, SEARCH)
    assert permuted
    m.noise = dict(eps_beam=eps[0])
    with torch.no_grad():
        out = m(c["feats"], np.asarray(c["fl"]).copy(), method="beam", beam_size=3, max_length=SML, **SEARCH)
    assert torch.equal(out["seqs"].cpu(), want)
    assert out["attn_weights"].shape[0] == 4 and out["attn_weights"].shape[2] == SML
    one, _ = ensemble_run([m], c["feats"], c["fl"], "beam", 3, eps, **SEARCH)
    assert torch.equal(one, want)


def test_unconstrained_searches_are_untouched():
    """All-off keywords take the entries of today and give their results bit for bit; those entries against the step loop
    are tests/test_ensemble_gpu.py and tests/test_model_gpu.py, unchanged."""
    c = search_case()
    off = dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, suppress_tokens=None)
    calls = []
    real = _lib.call
    for method, beam in (("greedy", 1), ("beam", 3)):
        eps = search_noise(4, beam, 34)
        a = ensemble_run(c["models"], c["feats"], c["fl"], method, beam, eps)
        want, score, _ = host_loop(c["models"], c["feats"], c["fl"], eps, beam, method == "greedy", {})
        _lib.call = lambda *x: (calls.append(x[0]), real(*x))[1]
        try:
            b = ensemble_run(c["models"], c["feats"], c["fl"], method, beam, eps, **off)
        finally:
            _lib.call = real
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[0], want)
    m = c["models"][0]
    eps = search_noise(4, 3, 35)[0]
    res = []
    for kw in ({}, off):
        m.noise = dict(eps_beam=eps)
        with torch.no_grad():
            res.append(m(c["feats"], np.asarray(c["fl"]).copy(), method="beam", beam_size=3, max_length=SML, **kw))
    assert torch.equal(res[0]["seqs"], res[1]["seqs"]) and torch.equal(res[0]["attn_weights"], res[1]["attn_weights"])
    assert not any("constrained" in name for name in calls)


# ------------------------------------------------------------------------------------------------ 4. wrappers and refusals
def test_evaluate_and_the_shared_encoder_rollout_end_to_end():
    model, feats, lens = small(-4.0)
    voc = EV.Vocabulary()
    for w in ["<pad>", "<start>", "<end>", "<unk>"] + [f"w{i}" for i in range(MV - 4)]:
        voc.add_word(w)
    g = torch.Generator().manual_seed(5)
    items = [(f"clip{i}", torch.randn(64, 64, generator=g)) for i in range(2)]
    torch.manual_seed(9)
    plain = EV.evaluate(model, items, voc, method="greedy", max_length=ML)
    assert any(CU.repeats_ngram(p["caption"].split(), 2) for p in plain["predictions"])
    for kw in (dict(method="greedy"), dict(method="beam", beam_size=3), dict(method="sample", beam_size=3, rng="device")):
        torch.manual_seed(9)
        got = EV.evaluate(model, items, voc, max_length=ML, no_repeat_ngram_size=2, **kw)
        assert [p["filename"] for p in got["predictions"]] == ["clip0", "clip1"]
        for p in got["predictions"]:
            caps = [c["caption"] for c in p["captions"]] if "captions" in p else [p["caption"]]
            assert all(not CU.repeats_ngram(c.split(), 2) for c in caps), caps
    torch.manual_seed(10)
    with torch.no_grad():
        rep = model.rollout_shared_encoder(feats, lens.copy(), 2, method="sample", rng="device", max_length=ML, min_length=3)
    seqs = rep["seqs"].cpu().numpy()
    assert seqs.shape == (2 * MB, ML) and not (seqs[:, :3] == model.end_idx).any()
    assert bool(torch.isneginf(rep["logits"][:, :3, model.end_idx]).all())
    assert not bool(torch.isneginf(rep["logits"][:, 3:, model.end_idx]).any())


def test_refusals_on_the_device_model():
    """Every refusal of the keywords is raised in front of the first launch: nothing is queued on the stream."""
    model, feats, lens = small(-4.0)
    caps, cap_lens = torch.ones(MB, 5, dtype=torch.long), np.array([5] * MB)
    calls = []
    real = _lib.call
    _lib.call = lambda *a: (calls.append(a[0]), real(*a))[1]
    try:
        for kw in CONTROL_SETS[1:]:
            key = next(iter(kw))
            with pytest.raises(ValueError, match=key):
                model(feats, lens.copy(), max_length=ML, method="dbs", **kw)
            with pytest.raises(ValueError, match=key):
                model(feats, lens.copy(), caps, cap_lens, ss_ratio=1.0, dis_ratio=0, **kw)
            model.train()
            try:
                with pytest.raises(ValueError, match="differentiable rollout"):
                    model(feats, lens.copy(), max_length=ML, method="sample", **kw)
            finally:
                model.eval()
        with pytest.raises(ValueError, match="suppress_tokens"):
            model(feats, lens.copy(), max_length=ML, suppress_tokens=[int(model.end_idx)])
        with pytest.raises(ValueError, match="min_length"):
            model(feats, lens.copy(), max_length=ML, min_length=ML + 1)
        with pytest.raises(ValueError, match="no_repeat_ngram_size"):
            model(feats, lens.copy(), max_length=MV - 1, no_repeat_ngram_size=2)       # a row must keep a word
    finally:
        _lib.call = real
        model.eval()
    assert calls == []
    buf = torch.zeros(4096, device="cuda")
    hist = torch.zeros(64, dtype=torch.long, device="cuda")
    for theta, n, m in ((0.0, 0, 0), (float("nan"), 0, 0), (1.0, -1, 0), (1.0, 0, -1)):
        with pytest.raises(RuntimeError, match="EINVAL"):
            _lib.call("acvae_constrain_logits", buf, 40, hist, 8, 3, 2, 40, 2, theta, n, m, None, 0, st())
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0
