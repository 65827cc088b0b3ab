"""GPU: the finishing beam search (finish_on_end / length_penalty / nbest).

1. acvae_beam_retire and acvae_beam_finish alone on planted histories, bit for bit against the numpy twin of
   tests/beam_finish_util.py.
2. acvae_ensemble_mix with prev = -inf: -inf in every column, never NaN (the mode rests on it).
3. acvae_beam_search_finishing / acvae_ensemble_search_finishing against a host loop over the step API with the twin's
   retire step behind each top-k and the twin's ranking at the end.
4. The tie to today's search: with <end> suppressed nothing finishes, and hypothesis 0 is today's beam 0 bit for bit.
5. With finishing off, spelled out or omitted, today's calls and results.
6. evaluate() / ensemble_evaluate() end to end."""
import ctypes
import itertools
import json

import numpy as np
import pytest
import torch

import acvae_oracle as O
import beam_finish_util as BF
import constrain_util as CU
from acvae_amd import _lib
from acvae_amd import evaluate as EV
from acvae_amd.encoder import ptr_table
from acvae_amd.ensemble import Ensemble, ensemble_evaluate
from acvae_amd.search import _constraint_args, _search_noise
from test_constrained_decoding_gpu import SEARCH, SML, SV, caption, controls_of, host_loop, search_noise, st
from test_fullsize_decode_gpu import LP_TOL
from test_model_gpu import build_model

pytestmark = pytest.mark.gpu
NEG = BF.NEG_INF
END = O.END_IDX


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


# ------------------------------------------------------------------------------------------------ 1. the kernels alone
KV = 40                                                     # words of the planted histories
KINDS = ("t0_and_last", "ties", "all_retired", "few", "dead")


def planted_clip(kind, beam, T, norm, rng):
    """One clip's caller-built steps: c float32 [T, beam] as a top-k would leave it, words int64 [T, beam].  Scores are
    multiples of 1/4 (many equal ones); <end> is sprinkled over every kind but "few"."""
    c = -(rng.integers(1, 40, (T, beam)).astype(np.float32) * np.float32(0.25))
    w = rng.integers(3, KV, (T, beam)).astype(np.int64)
    if kind != "few":
        w[rng.random((T, beam)) < 0.15] = END
    if kind == "t0_and_last":                                # a hypothesis finishing at t = 0 and one at T - 1
        w[0, 0] = END
        w[T - 1, beam - 1] = 5
    elif kind == "ties":                                     # every <end> row and the whole last step score exactly -1
        w[:, 0] = END
        ends = w == END
        ends[T - 1] = True
        c = np.where(ends, -norm[:, None], c).astype(np.float32)
    elif kind == "all_retired":                              # every row ends at one step; dead rows from there on
        w[T // 2] = END
        c[T // 2 + 1:] = NEG
    elif kind == "few":                                      # one alive row that never ends: one record, at T - 1
        c[:, 1:] = NEG
    elif kind == "dead":
        c[:] = NEG
    return c, w


def planted(N, beam, T, S, lp, first_kind, seed):
    rng = np.random.default_rng(seed)
    norm = BF.length_norm(T, lp)
    kinds = [KINDS[(first_kind + n) % len(KINDS)] for n in range(N)]
    cs, ws = zip(*(planted_clip(k, beam, T, norm, rng) for k in kinds))
    c, w = np.concatenate(cs, 1), np.concatenate(ws, 1)      # [T, R]
    R = N * beam
    parent = (rng.integers(0, beam, (T, R)) + (np.arange(R) // beam) * beam).astype(np.int64)
    attw = rng.random((T, R, S)).astype(np.float32)
    return kinds, norm, c, w, parent, attw


def run_kernels(N, beam, T, S, nbest, norm, c, w, parent, attw, hist_stride=None):
    """acvae_beam_retire on every step, then acvae_beam_finish on the records it wrote -> (c after, f, outputs)."""
    R = N * beam
    hs = R if hist_stride is None else hist_stride
    c_d, w_d = torch.from_numpy(c).cuda(), torch.from_numpy(w).cuda()
    f_d = torch.full((T, R), 7.0, device="cuda")
    for t in range(T):
        _lib.call("acvae_beam_retire", c_d[t], w_d[t], f_d[t], END, int(t == T - 1), R, st())
    par_h = torch.full((T, hs), -5, dtype=torch.long)
    word_h = torch.full((T, hs), -5, dtype=torch.long)
    par_h[:, :R], word_h[:, :R] = torch.from_numpy(parent), torch.from_numpy(w)
    par_d, word_d, attw_d = par_h.cuda(), word_h.cuda(), torch.from_numpy(attw).cuda()
    out = dict(seqs=torch.full((N, T), -9, dtype=torch.long, device="cuda"), logprobs=torch.full((N,), 7.0, device="cuda"),
               attw0=torch.full((N, S, T), 7.0, device="cuda"),
               nbest_seqs=torch.full((N, nbest, T), -9, dtype=torch.long, device="cuda"),
               scores=torch.full((N, nbest), 7.0, device="cuda"), nbest_logprobs=torch.full((N, nbest), 7.0, device="cuda"),
               lengths=torch.full((N, nbest), -9, dtype=torch.int32, device="cuda"))
    norm_d = torch.zeros(T, device="cuda")
    _lib.call("acvae_beam_finish", par_d, word_d, hs, f_d, norm.ctypes.data, norm_d, attw_d, out["seqs"], out["logprobs"],
              out["attw0"], out["nbest_seqs"], out["scores"], out["nbest_logprobs"], out["lengths"], N, beam, T, S, nbest, END,
              st())
    torch.cuda.synchronize()
    assert np.array_equal(bits(norm_d.cpu().numpy()), bits(norm))
    return c_d.cpu().numpy(), f_d.cpu().numpy(), {k: v.cpu().numpy() for k, v in out.items()}


def check_kernels(N, beam, T, S, nbest, lp, first_kind, seed):
    kinds, norm, c, w, parent, attw = planted(N, beam, T, S, lp, first_kind, seed)
    c_after, f, got = run_kernels(N, beam, T, S, nbest, norm, c, w, parent, attw, hist_stride=N * beam + (seed % 3))
    f_want = np.zeros_like(f)
    for t in range(T):
        c2, f_want[t] = BF.retire_step(c[t], w[t], END, t == T - 1)
        assert np.array_equal(bits(c_after[t]), bits(c2)), ("c", t)
    assert np.array_equal(bits(f), bits(f_want))
    want = BF.finish(parent, w, f_want, norm, N, beam, nbest, END, attw=attw)
    where = (N, beam, T, S, nbest, lp, kinds)
    assert np.array_equal(got["nbest_seqs"], want["seqs"]), where
    assert np.array_equal(got["lengths"], want["lengths"]), where
    assert np.array_equal(bits(got["scores"]), bits(want["scores"])), where
    assert np.array_equal(bits(got["nbest_logprobs"]), bits(want["logprobs"])), where
    assert np.array_equal(got["seqs"], want["seqs"][:, 0]) and np.array_equal(bits(got["logprobs"]), bits(want["logprobs"][:, 0]))
    assert np.array_equal(bits(got["attw0"]), bits(want["attw0"])), where
    # each planted clip is what it was planted for
    for n, kind in enumerate(kinds):
        fn = f_want[:, n * beam:(n + 1) * beam]
        recs = [(t, j) for t in range(T) for j in range(beam) if fn[t, j] > NEG]
        s = {(t, j): np.float32(fn[t, j] / norm[t]) for t, j in recs}
        L, sc = want["lengths"][n], want["scores"][n]
        if kind == "t0_and_last":
            assert fn[0, 0] > NEG and fn[T - 1, beam - 1] > NEG
            assert {1, T} <= {t + 1 for t, _ in recs}
        elif kind == "ties":
            assert all(v == np.float32(-1.0) for v in s.values()) and len(recs) >= min(T + beam - 1, T * beam)
            assert (sc[:min(nbest, len(recs))] == np.float32(-1.0)).all()
            picked = sorted(recs)[:nbest]                    # equal scores: the earlier step, then the lower row
            assert L[:len(picked)].tolist() == [t + 1 for t, _ in picked]
            if T > 1:
                assert len({t for t, _ in recs}) > 1         # equal normalised scores at different t ...
            if beam > 1:
                assert len({j for _, j in recs}) > 1         # ... and at different j
        elif kind == "all_retired":
            assert (fn[T // 2] > NEG).all() and (fn[T // 2 + 1:] == NEG).all() and (c_after[T // 2:, n * beam:(n + 1) * beam] == NEG).all()
        elif kind == "few":
            assert recs == [(T - 1, 0)]
            assert L.tolist() == [T] + [0] * (nbest - 1) and np.isneginf(sc[1:]).all()
            assert (want["seqs"][n, 1:] == END).all()
        elif kind == "dead":
            assert not recs and (L == 0).all() and np.isneginf(sc).all() and (want["seqs"][n] == END).all()
            assert (want["attw0"][n] == 0).all()
        if L[0] > 0:                                         # zeros in the columns behind hypothesis 0's length
            assert (want["attw0"][n][:, L[0]:] == 0).all() and (want["attw0"][n][:, :L[0]] > 0).all()


@pytest.mark.parametrize("beam", [1, 3, 16])
def test_retire_and_finish_kernels_equal_the_twin(beam):
    k = 0
    for T, N, nbest, S in itertools.product((1, 2, 10, 64, 70), (1, 5), sorted({1, beam}), (1, 7)):
        check_kernels(N, beam, T, S, nbest, (0.0, 0.7, 1.0)[k % 3], first_kind=k, seed=1000 * beam + k)
        k += 1
    assert k >= 2 * len(KINDS)                               # N = 1 walks through every kind too


def test_finish_clamps_a_parent_outside_the_rows():
    N, beam, T, S = 2, 3, 6, 4
    kinds, norm, c, w, parent, attw = planted(N, beam, T, S, 1.0, 0, 77)
    parent[2], parent[3, 0], parent[4, 1] = -3, 1 << 40, N * beam
    _, f, got = run_kernels(N, beam, T, S, beam, norm, c, w, parent, attw)
    want = BF.finish(parent, w, f, norm, N, beam, beam, END, attw=attw)
    assert np.array_equal(got["nbest_seqs"], want["seqs"]) and np.array_equal(bits(got["attw0"]), bits(want["attw0"]))


# ------------------------------------------------------------------------------------------------ 2. the mix at prev = -inf
@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("V", [50, 257, 1030])
def test_mix_with_prev_minus_inf_is_minus_inf_everywhere(M, V):
    """A retired row's children: every column -inf, never NaN (-inf + -inf, not inf - inf), also where the row holds banned
    logits; the alive rows beside it are untouched by it."""
    R = 6
    g = torch.Generator().manual_seed(V + M)
    logits = [torch.randn(R, V, generator=g) * 3 for _ in range(M)]
    for x in logits:
        x[0, 3::5] = -np.inf                                 # banned words in a retired row, in every member
        x[1, 4::7] = -np.inf                                 # ... and in an alive row
    logits[0][2, 7] = -np.inf                                # banned in one member only (M = 2: the mixture stays finite)
    logits[0][3, 9] = -np.inf
    prev = torch.tensor([-np.inf, -1.5, -np.inf, 0.0, -np.inf, -2.0])
    dev = [x.cuda() for x in logits]
    out = torch.full((R, V), 7.0, device="cuda")
    ld = np.full(M, V, np.int64)
    _lib.call("acvae_ensemble_mix", ptr_table(dev), ld.ctypes.data, M, prev.cuda(), out, V, None, None, 0, R, V, st())
    got = out.cpu()
    assert not torch.isnan(got).any()
    assert torch.isneginf(got[[0, 2, 4]]).all()
    ref = torch.log(torch.stack([torch.softmax(x.double(), -1) for x in logits]).mean(0)) + prev.double()[:, None]
    live = [1, 3, 5]
    finite = torch.isfinite(ref[live])
    assert torch.equal(torch.isneginf(got[live]), ~finite) and (~finite).any() == True
    assert float((got[live].double() - ref[live])[finite].abs().max()) <= LP_TOL


# ------------------------------------------------------------------------------------------------ 3. against the host loop
# <end> bias bumps of the two members and the seed of the prior's noise per beam width, chosen (from a scan of the host loop
# alone) so that the loop shows what check_against_loop asserts: hypotheses that end early, differ from today's answer and
# between the penalties, with margins the tolerance cannot bridge.  Larger bumps (2.5 and up) end every caption at once.
BUMPS = (0.5, 1.0)
NOISE = {3: 53, 16: 42}
_case = {}


def finishing_case():
    if not _case:
        models = []
        for seed, bump in zip((11, 12), BUMPS):
            torch.manual_seed(seed)
            m = build_model(SV, 64).eval()
            with torch.no_grad():
                m.decoder.classifier.bias[END] += bump
            models.append(m)
        feats, _, fl, _ = O.synthetic_batch(4, 96, SV, 7, seed=21, ragged=True)
        _case.update(models=models, feats=feats.cuda(), fl=fl, loops={})
    return _case


@torch.no_grad()
def finishing_loop(models, feats, fl, eps, beam, kw):
    """host_loop's beam search (tests/test_constrained_decoding_gpu.py) with the twin's retire step behind each top-k.
    -> parent, word [T, R], f [T, R], the steps at which the parents are not the identity."""
    theta, n, m, sup = controls_of(kw)
    M, V, T = len(models), SV, SML
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
    ld = np.full(M, V, np.int64)
    parent, word, frec = (np.zeros((T, R), np.int64), np.zeros((T, R), np.int64), np.zeros((T, R), np.float32))
    permuted = []
    for t in range(T):
        edited, new = [], []
        for k, mod in enumerate(models):
            pn = mod.pnet(w.unsqueeze(1), mem[k], hid[k], lz[k], lens[k], eps=eps[k][:, t].reshape(R, -1))
            dn = mod.decoder(word=w.unsqueeze(1), state=state[k], enc_mem=mem[k], enc_mem_lens=lens[k], z=pn["z"])
            x = dn["logits"].squeeze(1).contiguous()
            if kw:
                h = x.cpu().numpy()
                x = torch.from_numpy(np.stack([CU.constrain_row(h[r], hist[r], t, end, theta, n, m, sup)
                                               for r in range(R)])).cuda()
            edited.append(x)
            new.append((dn["state"], pn["hiddens_state"], pn["z"]))
        sc = torch.empty(R, V, device="cuda")
        vals = torch.empty(R, device="cuda")
        idx, prev, w = (torch.empty(R, dtype=torch.long, device="cuda") for _ in range(3))
        _lib.call("acvae_ensemble_mix", ptr_table(edited), ld.ctypes.data, M, top_k, sc, V, None, None, 0, R, V, st())
        assert not torch.isnan(sc).any()
        _lib.call("acvae_topk_flat_batched", sc, beam * V, beam * V, beam, V, vals, idx, prev, w, N, beam, st())
        p = prev.cpu().numpy()
        c, frec[t] = BF.retire_step(vals.cpu().numpy(), w.cpu().numpy(), end, t == T - 1)
        top_k = torch.from_numpy(c).cuda()
        parent[t], word[t] = p, w.cpu().numpy()
        if t > 0 and not np.array_equal(p, np.arange(R)):
            permuted.append(t)
        hist = np.concatenate([hist[p], word[t][:, None]], 1)
        for k in range(M):
            state[k] = new[k][0][:, prev].contiguous()
            hid[k] = (new[k][1][0][:, prev].contiguous(), new[k][1][1][:, prev].contiguous())
            lz[k] = new[k][2][prev].contiguous()
    return parent, word, frec, permuted


def looped(members, beam, constrained):
    """The host loop of a member set (a tuple of indices), shared by the tests; never changed."""
    c = finishing_case()
    key = (members, beam, constrained)
    if key not in c["loops"]:
        models = [c["models"][k] for k in members]
        eps = search_noise(4, beam, NOISE[beam])[:len(members)]
        kw = SEARCH if constrained else {}
        c["loops"][key] = (models, eps, kw) + finishing_loop(models, c["feats"], c["fl"], eps, beam, kw)
    return c["loops"][key]


def margins(frec, norm, N, beam, nbest):
    """Per clip the gaps between neighbours in the full ranking that decide the first nbest slots."""
    out = []
    for n in range(N):
        s = sorted((float(np.float32(frec[t, n * beam + j] / norm[t])) for t in range(frec.shape[0]) for j in range(beam)
                    if frec[t, n * beam + j] > NEG), reverse=True)
        out += [a - b for a, b in zip(s[:nbest], s[1:nbest + 1])]
    return out


def device_run(models, eps, beam, single, **kw):
    c = finishing_case()
    if single:
        models[0].noise = dict(eps_beam=eps[0])
        with torch.no_grad():
            out = models[0](c["feats"], np.asarray(c["fl"]).copy(), method="beam", beam_size=beam, max_length=SML, **kw)
    else:
        ens = Ensemble(models)
        ens.noise = {"eps": eps}
        out = ens(c["feats"], np.asarray(c["fl"]).copy(), method="beam", beam_size=beam, max_length=SML, **kw)
    return {k: v.cpu() for k, v in out.items()}


def check_against_loop(members, beam, constrained, single=False):
    models, eps, kw, parent, word, frec, permuted = looped(members, beam, constrained)
    N, T = 4, SML
    assert len(permuted) >= 2, permuted
    today, _, _ = host_loop(models, finishing_case()["feats"], finishing_case()["fl"], eps, beam, False, kw)
    picks = {}
    for lp in (0.0, 1.0):
        norm = BF.length_norm(T, lp)
        want = BF.finish(parent, word, frec, norm, N, beam, beam, END)
        gaps = margins(frec, norm, N, beam, beam)
        print(f"members {members} beam {beam} constrained {constrained} lp {lp}: lengths {want['lengths'].tolist()} "
              f"min margin {min(gaps):.3e} permuted {permuted}")
        assert min(gaps) > 20 * LP_TOL, min(gaps)
        got = device_run(models, eps, beam, single, finish_on_end=True, length_penalty=lp, nbest=beam, **kw)
        assert np.array_equal(got["nbest_seqs"].numpy(), want["seqs"])            # every clip, every slot, in order
        assert np.array_equal(got["nbest_lengths"].numpy(), want["lengths"])
        assert float(np.abs(got["nbest_scores"].numpy() - want["scores"]).max()) <= LP_TOL
        assert float(np.abs(got["nbest_logprobs"].numpy() - want["logprobs"]).max()) <= LP_TOL
        assert torch.equal(got["seqs"], got["nbest_seqs"][:, 0]) and torch.equal(got["scores"], got["nbest_scores"][:, 0])
        assert torch.equal(got["lengths"], got["nbest_lengths"][:, 0])
        assert (want["lengths"] > 0).all()                                        # `beam` finite continuations everywhere
        if single:
            aw, L = got["attn_weights"].numpy(), want["lengths"][:, 0]
            for i in range(N):
                assert (aw[i][:, L[i]:] == 0).all() and (aw[i][:, :L[i]].sum(0) > 0.99).all()
        else:
            assert torch.equal(got["logprobs"], got["nbest_logprobs"][:, 0])
        if constrained:                                                           # min_length: nothing shorter than the ban
            assert (want["lengths"] >= SEARCH["min_length"] + 1).all()
            for row in want["seqs"].reshape(-1, T).tolist():
                words = caption(row, END)
                assert not CU.repeats_ngram(words, SEARCH["no_repeat_ngram_size"])
                assert not set(words) & set(SEARCH["suppress_tokens"])
        picks[lp] = want
    ends_early = [i for i in range(N) if picks[1.0]["lengths"][i, 0] < T or picks[0.0]["lengths"][i, 0] < T]
    differs = [i for i in range(N) if caption(picks[1.0]["seqs"][i, 0], END) != caption(today[i].tolist(), END)
               or caption(picks[0.0]["seqs"][i, 0], END) != caption(today[i].tolist(), END)]
    split = [i for i in range(N) if picks[0.0]["seqs"][i, 0].tolist() != picks[1.0]["seqs"][i, 0].tolist()]
    print(f"  ends early {ends_early} differs from today {differs} penalties differ {split}")
    return ends_early, differs, split, got


@pytest.mark.parametrize("constrained", [False, True], ids=["plain", "constrained"])
def test_two_member_ensemble_equals_the_host_loop(constrained):
    ends_early, differs, split, _ = check_against_loop((0, 1), 3, constrained)
    assert ends_early and differs and split


@pytest.mark.parametrize("constrained", [False, True], ids=["plain", "constrained"])
def test_single_model_and_one_member_ensemble_equal_the_host_loop(constrained):
    ends_early, differs, split, single = check_against_loop((0,), 3, constrained, single=True)
    assert ends_early and differs and split
    _, _, _, one = check_against_loop((0,), 3, constrained)
    for key in ("seqs", "scores", "lengths", "nbest_seqs", "nbest_scores", "nbest_logprobs", "nbest_lengths"):
        assert torch.equal(single[key], one[key]), key                            # Ensemble([m]) is m, bit for bit


def test_beam_16_equals_the_host_loop():
    ends_early, differs, _, _ = check_against_loop((0, 1), 16, True)
    assert ends_early and differs


# ------------------------------------------------------------------------------------------------ 4. the tie to today's search
def test_with_end_suppressed_hypothesis_0_is_todays_beam_0():
    """suppress_tokens=[end_idx] (the C entries take it; the Python keyword refuses it) and length_penalty = 0: no row can
    finish, every record sits at the last step, and the best of them is the row today's search returns."""
    c = finishing_case()
    m = c["models"][0]
    N, T, beam, V = 4, SML, 3, SV
    eps = search_noise(N, beam, 43)[0]
    enc = m.encoder(c["feats"], np.asarray(c["fl"]).copy())
    mem = m._projected_memory(enc)
    lens = torch.as_tensor(enc["audio_embeds_lens"]).to(device="cuda", dtype=torch.long).contiguous()
    S, E = mem.shape[1], mem.shape[2]
    eps_d = _search_noise(N, T, beam, E, mem.device, eps)
    con = (1.0, 0, 0, (END,))
    norm = BF.length_norm(T, 0.0)
    dims = (N, beam, T, S, E, E, E, V)

    def outs():
        return torch.empty(N, T, dtype=torch.long, device="cuda"), torch.empty(N, S, T, device="cuda")

    seqs0, attw0 = outs()
    sb = _lib.call("acvae_beam_search_constrained_scratch_bytes", *dims)
    scratch = torch.empty(sb, dtype=torch.uint8, device="cuda")
    _lib.call("acvae_beam_search_constrained", m._text_table(), mem, lens, eps_d, int(m.start_idx), seqs0, attw0, scratch, sb,
              *dims, st(), END, *_constraint_args(con))
    seqs1, attw1 = outs()
    nb = (torch.empty(N, beam, T, dtype=torch.long, device="cuda"), torch.empty(N, beam, device="cuda"),
          torch.empty(N, beam, device="cuda"), torch.empty(N, beam, dtype=torch.int32, device="cuda"))
    sb = _lib.call("acvae_beam_search_finishing_scratch_bytes", *dims)
    scratch = torch.empty(sb, dtype=torch.uint8, device="cuda")
    _lib.call("acvae_beam_search_finishing", m._text_table(), mem, lens, eps_d, int(m.start_idx), seqs1, attw1, scratch, sb,
              *dims, st(), END, *_constraint_args(con), norm.ctypes.data, beam, *nb)
    torch.cuda.synchronize()
    assert torch.equal(seqs0, seqs1) and torch.equal(attw0, attw1)
    assert not (seqs1 == END).any() and (nb[3] == T).all()
    assert torch.equal(nb[1], nb[2])                                              # raw scores: s is f
    # the ensemble entries: logprobs is beam 0's final score today, hypothesis 0's record with finishing
    table = ptr_table(m._text_table())
    params = (ctypes.c_void_p * 1)(ctypes.cast(table, ctypes.c_void_p).value)
    host = [np.array([v], np.int32) for v in (S, E, E, E)]
    hp = [a.ctypes.data for a in host]
    lp0, lp1 = torch.empty(N, device="cuda"), torch.empty(N, device="cuda")
    seqs2, seqs3 = outs()[0], outs()[0]
    sb = _lib.call("acvae_ensemble_search_constrained_scratch_bytes", 1, N, beam, T, *hp, V)
    scratch = torch.empty(sb, dtype=torch.uint8, device="cuda")
    _lib.call("acvae_ensemble_search_constrained", params, [mem], [lens], [eps_d], *hp, 1, int(m.start_idx), END, 0, seqs2, lp0,
              scratch, sb, N, beam, T, V, st(), *_constraint_args(con))
    sb = _lib.call("acvae_ensemble_search_finishing_scratch_bytes", 1, N, beam, T, *hp, V)
    scratch = torch.empty(sb, dtype=torch.uint8, device="cuda")
    nb2 = (torch.empty(N, beam, T, dtype=torch.long, device="cuda"), torch.empty(N, beam, device="cuda"),
           torch.empty(N, beam, device="cuda"), torch.empty(N, beam, dtype=torch.int32, device="cuda"))
    _lib.call("acvae_ensemble_search_finishing", params, [mem], [lens], [eps_d], *hp, 1, int(m.start_idx), END, 0, seqs3, lp1,
              scratch, sb, N, beam, T, V, st(), *_constraint_args(con), norm.ctypes.data, beam, *nb2)
    torch.cuda.synchronize()
    assert torch.equal(seqs2, seqs0) and torch.equal(seqs3, seqs0)
    assert torch.equal(nb2[2][:, 0], lp0) and torch.equal(lp1, lp0) and torch.equal(nb[2][:, 0], lp0)
    assert torch.equal(nb2[0], nb[0])


# ------------------------------------------------------------------------------------------------ 5. off is untouched
def test_off_is_untouched():
    c = finishing_case()
    calls = []
    real = _lib.call
    m = c["models"][0]
    eps = search_noise(4, 3, 44)
    for kw in ({}, SEARCH):
        res = []
        for off in ({}, dict(finish_on_end=False), dict(finish_on_end=False, length_penalty=None, nbest=None)):
            _lib.call = lambda *x: (calls.append(x[0]), real(*x))[1]
            try:
                res.append((device_run([m], eps[:1], 3, True, **kw, **off), device_run(c["models"], eps, 3, False, **kw, **off)))
            finally:
                _lib.call = real
        for one, ens in res[1:]:
            assert set(one) == {"seqs", "attn_weights"} and set(ens) == {"seqs", "logprobs"}
            assert torch.equal(one["seqs"], res[0][0]["seqs"]) and torch.equal(one["attn_weights"], res[0][0]["attn_weights"])
            assert torch.equal(ens["seqs"], res[0][1]["seqs"]) and torch.equal(ens["logprobs"], res[0][1]["logprobs"])
    assert not any("finishing" in name for name in calls)
    assert {"acvae_beam_search", "acvae_beam_search_constrained", "acvae_ensemble_search",
            "acvae_ensemble_search_constrained"} <= set(calls)


# ------------------------------------------------------------------------------------------------ 6. end to end
def test_evaluate_and_ensemble_evaluate_end_to_end(tmp_path):
    c = finishing_case()
    voc = EV.Vocabulary()
    for w in ["<pad>", "<start>", "<end>", "<unk>"] + [f"w{i}" for i in range(SV - 4)]:
        voc.add_word(w)
    assert voc("<end>") == END
    g = torch.Generator().manual_seed(5)
    items = [(f"clip{i}", torch.randn(64 + 8 * i, 64, generator=g)) for i in range(3)]
    m = c["models"][0]
    seen = []
    for run, model in ((EV.evaluate, m), (ensemble_evaluate, c["models"])):
        cls = type(m) if run is EV.evaluate else Ensemble
        real = cls.forward

        def spy(self, *a, real=real, **k):                                        # the rows the forward returned
            out = real(self, *a, **k)
            seen.append({key: v.cpu().numpy() for key, v in out.items()})
            return out

        for nbest in (1, 3):
            del seen[:]
            path = tmp_path / f"{run.__name__}_{nbest}.json"
            cls.forward = spy
            try:
                torch.manual_seed(9)
                got = run(model, items, voc, caption_output=path, batch_size=2, method="beam", beam_size=3, max_length=SML,
                          finish_on_end=True, nbest=nbest, min_length=2)
            finally:
                cls.forward = real
            assert [p["filename"] for p in got["predictions"]] == ["clip0", "clip1", "clip2"]
            rows = np.concatenate([o["nbest_seqs"] for o in seen], 0)             # [3 clips, nbest, T], as returned
            assert rows.shape == (3, nbest, SML)
            for p, clip in zip(got["predictions"], rows):
                want = [" ".join(voc.idx2word[w] for w in caption(r, END) if voc.idx2word[w] != "<start>") for r in clip]
                if nbest == 1:
                    assert "captions" not in p and p["caption"] == want[0]
                else:
                    assert [e["caption"] for e in p["captions"]] == want and [e["cap_id"] for e in p["captions"]] == [0, 1, 2]
                assert all(len(caption(r, END)) >= 2 for r in clip)                   # min_length reached the search
            assert json.load(open(path)) == got
