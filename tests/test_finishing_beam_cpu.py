"""CPU: the finishing beam search without a GPU.

1. The numpy twin (tests/beam_finish_util.py: parent pointers, -inf rows, the device's arithmetic) against the naive search
   (lists of hypotheses with their own words) over seeded and planted table language models; three mutants of the twin
   must be caught by the same cases.
2. The library: the new symbols, the ABI version, the scratch arithmetic and every refusal code (host code: nothing is
   launched).
3. Every ValueError of the Python keywords, raised in front of any device work."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import beam_finish_util as BF
from acvae_amd import _lib
from test_ensemble_cpu import Args, BeamArgs, cpu_model

EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -3, -4
V, END = 12, 2
BEAMS, LENGTHS, PENALTIES = (1, 3, 5), (1, 2, 7), (0.0, 0.7, 1.0)
NEG = BF.NEG_INF


# ------------------------------------------------------------------------------------------------ the table models
def tables(kind, beam, T, lp, seed=0):
    first, logp = BF.random_tables(V, beam, 100 + seed + 7 * beam + T)
    if kind == "end_best":                                   # <end> the best word everywhere: every row finishes at once
        first[:, END] = 0.5
        logp[:, END] = 0.5
    elif kind == "end_impossible":
        first[:, END] = NEG
        logp[:, END] = NEG
    elif kind == "tie":                                      # row 0 ends at once with score -1; row 1 says word 5, then
        norm = BF.length_norm(max(T, 2), lp)                 # <end>, with f = -norm[1]: the same normalised score
        first[:] -= 8.0
        logp[:] -= 8.0
        first[0, END] = -1.0
        first[min(1, beam - 1), 5] = -norm[1] if beam > 1 else -0.5
        logp[5, END] = 0.0
        if beam == 1:                                        # one row: it cannot both end and go on; the tie needs two
            first[0, END] = -9.0
    elif kind == "few":                                      # fewer finite continuations than `beam`
        first[:] = NEG
        first[0, 5] = -0.5                                   # "5 7 <end>" and "5 7 8 8 ..." are all there is
        logp[:] = NEG
        logp[5, 7], logp[7, END], logp[7, 8], logp[8, 8] = -0.25, -1.0, -0.75, -0.1
    else:
        assert kind.startswith("random")
    return first, logp


KINDS = ("random0", "random1", "end_best", "end_impossible", "tie", "few")
GRID = list(itertools.product(KINDS, BEAMS, LENGTHS, PENALTIES))


def both(kind, beam, T, lp, mutant=None, record=None):
    first, logp = tables(kind, beam, T, lp, seed=int(kind[-1]) if kind.startswith("random") else 0)
    got = BF.twin_search(first, logp, END, beam, T, lp, beam, mutant=mutant, record=record)
    want = BF.naive_search(first, logp, END, beam, T, lp, beam)
    return got, want


def same(got, want):
    return all(np.array_equal(got[k].view(np.int32) if got[k].dtype == np.float32 else got[k],
                              want[k].view(np.int32) if want[k].dtype == np.float32 else want[k])
               for k in ("seqs", "lengths", "scores", "logprobs"))


@pytest.mark.parametrize("kind", KINDS)
def test_twin_equals_the_naive_search(kind):
    """Words, lengths, order, scores and raw log-probabilities, bit for bit (both add and divide in float32), for every
    beam, length and penalty; each planted table is also what it was planted for."""
    for beam, T, lp in itertools.product(BEAMS, LENGTHS, PENALTIES):
        rec = {}
        got, want = both(kind, beam, T, lp, record=rec)
        for k in ("seqs", "lengths"):
            assert np.array_equal(got[k], want[k]), (kind, beam, T, lp, k, got[k], want[k])
        assert same(got, want), (kind, beam, T, lp)
        L = got["lengths"]
        for q in range(beam):                               # a row is its words, then <end> to the end
            assert (got["seqs"][q, L[q]:] == END).all()
            assert L[q] == 0 or END not in got["seqs"][q, :L[q] - 1]
        order = [(-float(s), int(l)) for s, l in zip(got["scores"], L) if l > 0]
        assert order == sorted(order)                       # score descending, the earlier step first among equals
        if kind == "end_best":
            assert (L == 1).all() and (got["seqs"][:, 0] == END).all()
            if T > 1:                                       # from step 1 on dead rows fill the beam
                assert all((c == NEG).all() for c in rec["c"])
        if kind == "end_impossible":
            assert (L == T).all() and END not in got["seqs"]
        if kind == "tie" and beam > 1 and T > 1:
            assert got["scores"][0] == got["scores"][1] == np.float32(-1.0)
            assert L[0] == 1 and L[1] == 2
        if kind == "few" and beam > 1:
            assert (L == 0).any() and np.isneginf(got["scores"][L == 0]).all()
            assert (got["seqs"][L == 0] == END).all()
            assert (L > 0).any()


def test_the_tie_goes_to_the_earlier_step_at_every_penalty():
    for lp in PENALTIES:
        got, _ = both("tie", 3, 7, lp)
        assert got["scores"][0] == got["scores"][1] and got["lengths"][0] == 1 and got["lengths"][1] == 2
        assert got["seqs"][1, :2].tolist() == [5, END]


@pytest.mark.parametrize("mutant", ["record_after_retire", "rank_raw", "trace_last"])
def test_mutants_of_the_twin_are_caught(mutant):
    caught = [g for g in GRID if not same(*both(*g, mutant=mutant))]
    assert caught, mutant
    assert any(g[0].startswith("random") for g in caught), (mutant, caught)      # not by a planted table alone


def test_retire_step_by_hand():
    c = np.array([-1.0, -2.0, -np.inf, -3.0], np.float32)
    w = np.array([END, 4, END, 5])
    c2, f = BF.retire_step(c, w, END, False)
    assert f.tolist() == [-1.0, -np.inf, -np.inf, -np.inf] and c2.tolist() == [-np.inf, -2.0, -np.inf, -3.0]
    c2, f = BF.retire_step(c, w, END, True)                 # the last step records every alive row; a dead one never
    assert f.tolist() == [-1.0, -2.0, -np.inf, -3.0] and c2.tolist() == [-np.inf, -2.0, -np.inf, -3.0]


def test_length_norm_matches_the_package():
    from acvae_amd.search import length_norm
    for lp in (0.0, 0.5, 0.7, 1.0, 2.3):
        a, b = length_norm(70, lp), BF.length_norm(70, lp)
        assert a.dtype == np.float32 and np.array_equal(a.view(np.int32), b.view(np.int32))
    assert (BF.length_norm(9, 0.0) == 1).all() and BF.length_norm(9, 1.0).tolist() == list(range(1, 10))


# ------------------------------------------------------------------------------------------------ the library
NEW = ("acvae_beam_retire", "acvae_beam_finish", "acvae_beam_search_finishing", "acvae_beam_search_finishing_scratch_bytes",
       "acvae_ensemble_search_finishing", "acvae_ensemble_search_finishing_scratch_bytes")


def test_symbols_abi_and_scratch_bytes():
    ge.build()
    lib = _lib.lib()
    for name in NEW:
        assert name in _lib.PROTOS and hasattr(lib, name), name
    assert lib.acvae_abi_version() == 3 and int(_lib._defs["ACVAE_ABI_VERSION"]) == 3
    for N, beam, T in ((1, 1, 1), (3, 3, 8), (32, 16, 30)):
        dims = (N, beam, T, 4, 64, 64, 64, 50)
        plain, con, fin = (getattr(lib, f"acvae_beam_search{s}_scratch_bytes")(*dims) for s in ("", "_constrained", "_finishing"))
        assert fin >= con + 4 * (T * N * beam + T) and con >= plain > 0
        S, E = np.full(2, 4, np.int32), np.full(2, 64, np.int32)
        edims = (2, N, beam, T, S.ctypes.data, E.ctypes.data, E.ctypes.data, E.ctypes.data, 50)
        plain, con, fin = (getattr(lib, f"acvae_ensemble_search{s}_scratch_bytes")(*edims)
                           for s in ("", "_constrained", "_finishing"))
        assert fin >= con + 4 * (T * N * beam + T) and con >= plain > 0
    assert lib.acvae_beam_search_finishing_scratch_bytes((1 << 20) // 4 + 1, 4, 8, 4, 64, 64, 64, 50) == -1


class Fin:
    """The finishing arguments: a host norm table and fake non-null outputs (as Args: refused before any launch)."""

    def __init__(self, T, nbest=2):
        self.norm = np.ones(T, np.float32)
        self.norm_ptr = self.norm.ctypes.data
        self.nbest = nbest
        self.nb_seqs = self.nb_scores = self.nb_logprobs = self.nb_lengths = 0x1000

    def tail(self):
        return (self.norm_ptr, self.nbest, self.nb_seqs, self.nb_scores, self.nb_logprobs, self.nb_lengths)


def beam_call(a, f, end=2, con=(1.0, 0, 0, None, 0)):
    return _lib.lib().acvae_beam_search_finishing(a.params, a.mem, a.mem_lens, a.eps, a.start, a.seqs, a.attn_weights,
                                                  a.scratch, a.scratch_bytes, a.N, a.beam, a.T, a.S, a.E, a.H, a.A, a.V, None,
                                                  end, *con, *f.tail())


def ens_call(a, f, con=(1.0, 0, 0, None, 0)):
    return _lib.lib().acvae_ensemble_search_finishing(a.params, a.mem, a.lens, a.eps, a.S.ctypes.data, a.E.ctypes.data,
                                                      a.H.ctypes.data, a.A.ctypes.data, a.M, a.start, a.end, a.greedy, a.seqs,
                                                      a.logprobs, a.scratch, a.scratch_bytes, a.N, a.beam, a.T, a.V, None,
                                                      *con, *f.tail())


def refusals(make, call, need):
    """The refusals the two entries share.  A well-formed call would reach its first launch with these pointers, so the one
    positive control is the workspace code: every check in front of it has passed when it is returned."""
    a = make()
    a.scratch_bytes = need(a) - 1
    assert call(a, Fin(a.T)) == EWORKSPACE                                # all else in order
    for nbest in (0, -1, 4, 17):                                           # outside [1, beam = 3]
        a = make()
        assert call(a, Fin(a.T, nbest)) == EINVAL, nbest
    for field in ("nb_seqs", "nb_scores", "nb_logprobs", "nb_lengths", "norm_ptr"):      # a NULL output, a NULL table
        a, f = make(), Fin(make().T)
        setattr(f, field, None)
        assert call(a, f) == EINVAL, field
    for bad in (0.0, -1.0, float("inf"), float("nan")):                     # an entry that is not finite and positive
        for at in (0, -1):
            a = make()
            f = Fin(a.T)
            f.norm[at] = bad
            assert call(a, f) == EINVAL, (bad, at)
    a = make()
    assert call(a, Fin(a.T), con=(0.0, 0, 0, None, 0)) == EINVAL          # what the constrained entries refuse
    assert call(make(), Fin(make().T), con=(1.0, 0, make().T + 1, None, 0)) == EINVAL


def test_beam_search_finishing_refusal_codes():
    ge.build()
    lib = _lib.lib()
    need = lambda a: lib.acvae_beam_search_finishing_scratch_bytes(a.N, a.beam, a.T, a.S, a.E, a.H, a.A, a.V)
    refusals(BeamArgs, beam_call, need)
    for end in (-1, 50):                                                    # end_idx outside [0, V)
        assert beam_call(BeamArgs(), Fin(BeamArgs().T), end=end) == EINVAL
    for field in ("params", "mem", "mem_lens", "eps", "seqs", "attn_weights", "scratch"):
        a = BeamArgs()
        setattr(a, field, None)
        assert beam_call(a, Fin(a.T)) == EINVAL, field
    assert beam_call(BeamArgs(beam=17), Fin(BeamArgs().T, 17)) == EINVAL
    a = BeamArgs()                                                          # the constrained size is not enough
    a.scratch_bytes = lib.acvae_beam_search_constrained_scratch_bytes(a.N, a.beam, a.T, a.S, a.E, a.H, a.A, a.V)
    assert beam_call(a, Fin(a.T)) == EWORKSPACE


def test_ensemble_search_finishing_refusal_codes():
    ge.build()
    lib = _lib.lib()
    need = lambda a: lib.acvae_ensemble_search_finishing_scratch_bytes(a.M, a.N, a.beam, a.T, a.S.ctypes.data, a.E.ctypes.data,
                                                                       a.H.ctypes.data, a.A.ctypes.data, a.V)
    refusals(Args, ens_call, need)
    a = Args(beam=1)                                                        # greedy has nothing to finish
    a.greedy = 1
    assert ens_call(a, Fin(a.T, 1)) == EINVAL
    a = Args(beam=1)
    a.scratch_bytes = need(a) - 1
    assert ens_call(a, Fin(a.T, 1)) == EWORKSPACE                           # (beam 1 without greedy is in order)
    for field in ("seqs", "logprobs", "scratch"):
        a = Args()
        setattr(a, field, None)
        assert ens_call(a, Fin(a.T)) == EINVAL, field


def test_per_op_entry_refusal_codes():
    ge.build()
    lib = _lib.lib()
    p = 0x1000
    assert lib.acvae_beam_retire(None, p, p, 2, 0, 4, None) == EINVAL
    assert lib.acvae_beam_retire(p, None, p, 2, 0, 4, None) == EINVAL
    assert lib.acvae_beam_retire(p, p, None, 2, 0, 4, None) == EINVAL
    assert lib.acvae_beam_retire(p, p, p, 2, 0, 0, None) == EINVAL
    norm = np.ones(8, np.float32)

    def finish(parent=p, word=p, stride=6, f=p, table=norm.ctypes.data, dev=p, attw=p, attw_out=p, nb=(p, p, p, p), N=2,
               beam=3, T=8, S=4, nbest=3):
        return lib.acvae_beam_finish(parent, word, stride, f, table, dev, attw, p, p, attw_out, *nb, N, beam, T, S, nbest, 2, None)

    for kw in (dict(parent=None), dict(word=None), dict(f=None), dict(table=None), dict(dev=None), dict(stride=5),
               dict(attw=None), dict(attw_out=None), dict(nbest=0), dict(nbest=4), dict(beam=17, nbest=17, stride=40),
               dict(N=0), dict(T=0), dict(S=0), dict(nb=(None, p, p, p)), dict(nb=(p, None, p, p)), dict(nb=(p, p, None, p)),
               dict(nb=(p, p, p, None))):
        assert finish(**kw) == EINVAL, kw
    norm[3] = 0.0
    assert finish() == EINVAL


# ------------------------------------------------------------------------------------------------ the Python keywords
def test_every_value_error_of_the_keywords():
    """Raised in front of the encoder: the model lives on the CPU, where the first library call would raise RuntimeError."""
    from acvae_amd import evaluate as EV
    from acvae_amd.consensus import Consensus
    from acvae_amd.ensemble import Ensemble
    m = cpu_model(1).eval()
    feats, lens = torch.zeros(2, 64, 64), np.array([64, 64])
    ens = Ensemble([m, cpu_model(2).eval()])

    def runs(**kw):
        return [lambda: m(feats, lens.copy(), max_length=8, **kw),
                lambda: ens(feats, lens.copy(), max_length=8, **kw)]

    for method in ("greedy",):                                             # (the ensemble knows greedy and beam only)
        for run in runs(method=method, finish_on_end=True):
            with pytest.raises(ValueError, match="finish_on_end"):
                run()
    for method in ("sample", "gumbel", "dbs"):
        with pytest.raises(ValueError, match="finish_on_end"):
            m(feats, lens.copy(), max_length=8, method=method, finish_on_end=True)
    with pytest.raises(ValueError, match="finish_on_end"):                  # the default method is greedy
        m(feats, lens.copy(), max_length=8, finish_on_end=True)
    for kw in (dict(length_penalty=1.0), dict(nbest=1), dict(nbest=2, finish_on_end=False), dict(length_penalty=0.0)):
        for run in runs(method="beam", beam_size=3, **kw):
            with pytest.raises(ValueError, match="without finish_on_end"):
                run()
    for lp in (-0.5, float("inf"), float("nan"), "long", True):
        for run in runs(method="beam", beam_size=3, finish_on_end=True, length_penalty=lp):
            with pytest.raises(ValueError, match="length_penalty"):
                run()
    for run in runs(method="beam", beam_size=3, finish_on_end=True, length_penalty=60.0):
        with pytest.raises(ValueError, match="overflows"):                  # 8 ** 60 is no float32
            run()
    for nbest in (0, -1, 4, 2.0, True):
        for run in runs(method="beam", beam_size=3, finish_on_end=True, nbest=nbest):
            with pytest.raises(ValueError, match="nbest"):
                run()
    with pytest.raises(ValueError, match="finish_on_end"):
        m(feats, lens.copy(), max_length=8, method="beam", finish_on_end=1)
    voc = EV.Vocabulary()
    for w in ["<pad>", "<start>", "<end>", "<unk>"] + [f"w{i}" for i in range(46)]:
        voc.add_word(w)
    with pytest.raises(ValueError, match="rerank"):                         # stays refused with a search
        m.rollout_shared_encoder(feats, lens.copy(), 3, method="beam", beam_size=3, max_length=8, finish_on_end=True,
                                 rerank=Consensus(voc))
    items = [("a", torch.zeros(64, 64))]
    with pytest.raises(ValueError, match="nbest"):
        EV.evaluate(m, items, voc, method="beam", beam_size=3, max_length=8, finish_on_end=True, nbest=4)
    with pytest.raises(ValueError, match="rerank"):
        EV.evaluate(m, items, voc, method="beam", beam_size=3, max_length=8, finish_on_end=True, rerank=Consensus(voc))
    with pytest.raises(ValueError, match="without finish_on_end"):
        m.beam_search({}, 8, 3, nbest=2)
    with pytest.raises(TypeError, match="unexpected"):
        m.beam_search({}, 8, 3, finish=True)
