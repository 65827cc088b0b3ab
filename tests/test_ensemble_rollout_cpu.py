"""CPU: the ensemble rollouts without a GPU - the float64 yardstick of tests/ensemble_rollout_util.py against a plain loop
and against the five mistakes it has to catch, its host-loop twin against ensemble_util.ensemble_greedy, what
Ensemble.rollout and ensemble_evaluate refuse on CPU tensors, the refusal codes of the new C entries (host code: nothing is
launched), and the float64 reference alone on the kernel test's seeded inputs: how many decisions that test leaves out."""
import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import acvae_oracle as O
import ensemble_rollout_util as RU
import ensemble_util as EU
from acvae_amd import _lib
from acvae_amd.consensus import Consensus
from acvae_amd.diversity import Diversity
from acvae_amd.ensemble import Ensemble, ensemble_evaluate
from test_consensus_cpu import vocab_of
from test_ensemble_cpu import EINVAL, EUNSUPPORTED, EWORKSPACE, MAXLEN, Args, E, V, cpu_model, state_of
from test_ensemble_rollout_kernels_gpu import MAX_BOUND, MAX_LEFT_OUT, decision_bound, mixture_and_bound

END = 2


def small(seed, M=3, R=4, Vs=7, method="sample"):
    rng = np.random.default_rng(seed)
    rows = [(rng.standard_normal((R, Vs)) * 2 + m).astype(np.float32) for m in range(M)]
    noise = rng.gumbel(size=(R, Vs)) if method == "gumbel" else rng.exponential(size=(R, Vs))
    return rows, noise.astype(np.float32)


# ------------------------------------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("method", RU.METHODS)
def test_yardstick_is_the_plain_loop(method):
    for seed, M, R, Vs, temp in ((1, 1, 3, 1, 1.0), (2, 2, 4, 2, 0.5), (3, 3, 5, 7, 2.0), (4, 8, 3, 300, 1.0)):
        rows, noise = small(seed, M, R, Vs, method)
        if Vs > 2:
            for row in rows:                       # a word no member gives any mass, with the noise most in its favour
                row[0, 1] = -np.inf
            noise[0, 1] = 80.0 if method == "gumbel" else 1e-30
            rows[0][1, 2], rows[0][1, 4] = rows[0][1, 4], rows[0][1, 2]
        prev = np.array([END if r % 2 else 5 for r in range(R)])
        got = RU.pick(rows, noise, method, temp, prev, END)
        words, lps = RU.pick_brute(rows, noise, method, temp, prev, END)
        assert np.array_equal(got["word"], words)
        assert np.allclose(got["logprob"], lps, atol=1e-12, rtol=0)
        assert (got["word"][prev == END] == END).all()
        if Vs > 2:
            assert got["chosen"][0] != 1 and got["v"][0, 1] == -np.inf
        assert np.allclose(np.exp(got["v"]).sum(-1), 1.0, atol=1e-12)          # the mixture is a distribution


def test_yardstick_first_maximum_on_planted_ties():
    for method in RU.METHODS:
        rows, noise = small(5, 2, 3, 9, method)
        for row in rows:
            row[:, 6] = row[:, 2] = 9.0
        noise[:, 6] = noise[:, 2] = noise[:, 0]
        got = RU.pick(rows, noise, method, 1.0)
        assert (got["chosen"] == 2).all() and (got["gap"] == 0.0).all()
        assert np.array_equal(RU.pick_brute(rows, noise, method, 1.0)[0], got["chosen"])


def test_yardstick_by_hand():
    """Members p = (1/2, 1/4, 1/4) and (1/10, 3/5, 3/10): the mixture is (0.3, 0.425, 0.275).  With q = (1, 2, 1) "sample"
    scores 0.3, 0.2125, 0.275 at temp 1 (word 0) and 0.09, 0.0903, 0.0756 at temp 1/2 (word 1)."""
    rows = [np.log(np.array([[0.5, 0.25, 0.25]])) + 7.0, np.log(np.array([[0.1, 0.6, 0.3]])) - 2.0]
    q = np.array([[1.0, 2.0, 1.0]])
    one = RU.pick(rows, q, "sample", 1.0)
    assert np.allclose(np.exp(one["v"]), [[0.3, 0.425, 0.275]], atol=1e-12) and one["chosen"][0] == 0
    assert np.allclose(np.exp(one["score"]), [[0.3, 0.2125, 0.275]], atol=1e-12)
    half = RU.pick(rows, q, "sample", 0.5)
    assert half["chosen"][0] == 1 and np.allclose(np.exp(half["score"]), [[0.09, 0.0903125, 0.075625]], atol=1e-12)
    assert np.allclose(half["logprob"], np.log(0.425))                          # untempered
    g = np.array([[0.0, -0.4, 0.1]])
    assert RU.pick(rows, g, "gumbel", 3.0)["chosen"][0] == 2                    # log .3, log .425 - .4, log .275 + .1


@pytest.mark.parametrize("mutant", RU.MUTANTS)
def test_yardstick_catches_the_mutant(mutant):
    """Each planted mistake changes a word or a log-probability of at least one of a few seeded cases; most change many."""
    differs = 0
    for method in RU.METHODS:
        for seed in range(6):
            rows, noise = small(10 + seed, 3, 6, 40, method)
            if mutant == "last_max":               # exact ties that win: only they tell the first maximum from the last
                for row in rows:
                    row[:, 30] = row[:, 3] = 12.0
                noise[:, 30] = noise[:, 3]
            prev = np.array([END, 1, END, 4, 5, END])
            want = RU.pick(rows, noise, method, 0.5, prev, END)
            got = RU.pick(rows, noise, method, 0.5, prev, END, mutant=mutant)
            differs += int(not np.array_equal(want["word"], got["word"])
                           or not np.allclose(want["logprob"], got["logprob"], atol=1e-9, rtol=0))
    assert differs >= 6, (mutant, differs)


# ------------------------------------------------------------------------------------------------ the host-loop twin
@pytest.fixture(scope="module")
def case():
    states = [state_of(cpu_model(1)), state_of(cpu_model(2))]
    feats, _, fl, _ = O.synthetic_batch(2, 64, V, 7, seed=2, ragged=True)
    g = torch.Generator().manual_seed(3)
    eps = [torch.randn(2, MAXLEN, 3, E, generator=g) for _ in states]
    noise = torch.empty(MAXLEN, 6, V).exponential_(1, generator=g).numpy()
    return states, [EU.encode(s, feats, fl) for s in states], eps, noise


def test_twin_greedy_with_one_row_per_clip_is_ensemble_greedy(case):
    states, enc, eps, _ = case
    one = [e[:, :, :1] for e in eps]
    want, want_lp = EU.ensemble_greedy(states, enc, MAXLEN, one)
    got = RU.rollout_twin(states, enc, 1, MAXLEN, one, None, "greedy", 1.0)
    assert np.array_equal(got["seqs"], want.numpy())
    assert np.allclose(got["logprobs"], want_lp.numpy(), atol=1e-9)


def test_twin_rows_of_a_clip_share_its_memory_and_feeding_its_own_words_changes_nothing(case):
    states, enc, eps, noise = case
    own = RU.rollout_twin(states, enc, 3, MAXLEN, eps, noise, "sample", 1.0)
    assert own["seqs"].shape == (6, MAXLEN) and (own["gap"] >= 0).all()
    assert len({tuple(r) for r in own["seqs"].tolist()}) > 2                   # the rows differ: they are samples
    fed = RU.rollout_twin(states, enc, 3, MAXLEN, eps, noise, "sample", 1.0, feed=own["seqs"])
    assert np.array_equal(fed["seqs"], own["seqs"]) and np.array_equal(fed["logprobs"], own["logprobs"])
    other = own["seqs"].copy()
    other[:, 0] = (other[:, 0] + 1) % V
    assert not np.array_equal(RU.rollout_twin(states, enc, 3, MAXLEN, eps, noise, "sample", 1.0, feed=other)["logprobs"][:, 1:],
                              own["logprobs"][:, 1:])
    # clip-major rows: row n * 3 + j with rollout j's noise of clip n alone is row j of a one-clip rollout of that clip
    solo = RU.rollout_twin(states, [(m[1:2], l[1:2]) for m, l in enc], 3, MAXLEN, [e[1:2] for e in eps], noise[:, 3:],
                           "sample", 1.0)
    assert np.array_equal(solo["seqs"], own["seqs"][3:])
    for row in own["seqs"].tolist():                                           # a finished row keeps <end>
        if O.END_IDX in row:
            assert row[row.index(O.END_IDX):] == [O.END_IDX] * (MAXLEN - row.index(O.END_IDX))


# ------------------------------------------------------------------------------------------------ Python refusals
def test_rollout_refusals_come_in_front_of_the_encoders():
    """CPU tensors: a call that got past its refusals would raise the RuntimeError of _lib.require_cuda."""
    ens = Ensemble([cpu_model(1), cpu_model(2)])
    feats, lens = torch.zeros(1, 64, 64), np.array([64])
    for match, kw in (("method", dict(method="beam")), ("method", dict(method="dbs")), ("method", dict(method="multinomial")),
                      ("top_k", dict(method="greedy", top_k=3)), ("top_p", dict(method="greedy", top_p=0.5)),
                      ("top_k", dict(top_k=-1)), ("top_p", dict(top_p=0.0)), ("sample_n", dict(sample_n=0)),
                      ("sample_n", dict(sample_n=2.5)), ("temp", dict(temp=0.0)), ("temp", dict(temp=float("nan"))),
                      ("temp", dict(temp=float("inf"))), ("temp", dict(temp="x")), ("rng", dict(rng="philox")),
                      ("min_length", dict(min_length=21)), ("repetition_penalty", dict(repetition_penalty=0.0)),
                      ("suppress_tokens", dict(suppress_tokens=[ens.end_idx])),
                      ("rerank", dict(sample_n=1, rerank=Consensus(vocab_of(V)))), ("rerank", dict(sample_n=17, rerank=Consensus(vocab_of(V)))),
                      ("max_length", dict(sample_n=3, rerank=Consensus(vocab_of(V)), max_length=65)),
                      ("Consensus", dict(sample_n=3, rerank="best"))):
        with pytest.raises(ValueError, match=match):
            ens.rollout(feats, lens, **kw)
    ens.noise = {"eps": [torch.zeros(1, 20, 1, E)]}                             # one tensor for two members
    with pytest.raises(ValueError, match="noise"):
        ens.rollout(feats, lens)
    assert ens.noise is None
    for kw in (dict(), dict(method="greedy", sample_n=4), dict(method="gumbel", top_k=5, top_p=0.9, temp=0.7, rng="host"),
               dict(sample_n=16, rerank=Consensus(vocab_of(V)), max_length=64)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ens.rollout(feats, lens, **kw)
    with pytest.raises(ValueError, match="method"):                             # forward has not changed
        ens(feats, lens, method="sample")


def test_ensemble_evaluate_refusals():
    ens = Ensemble([cpu_model(1)])
    items = [("a", torch.zeros(64, 64))]
    for match, kw in (("sample_n", dict(rerank=Consensus(vocab_of(V)))), ("sample_n", dict(diversity=Diversity(vocab_of(V)))),
                      ("rerank", dict(sample_n=1, rerank=Consensus(vocab_of(V)))), ("diversity", dict(sample_n=1, diversity=Diversity(vocab_of(V)))),
                      ("diversity", dict(sample_n=17, diversity=Diversity(vocab_of(V)))), ("Diversity", dict(sample_n=3, diversity=3)),
                      ("max_length", dict(sample_n=3, diversity=Diversity(vocab_of(V)), max_length=999)),
                      ("Accuracy", dict(sample_n=3, accuracy=3)), ("method", dict(sample_n=3, method="beam"))):
        with pytest.raises(ValueError, match=match):
            ensemble_evaluate(ens, items, None, **kw)


# ------------------------------------------------------------------------------------------------ the C entry points
class RolloutArgs(Args):
    """A well-formed argument set of acvae_ensemble_rollout (fake non-null device pointers, as Args)."""

    def __init__(self, M=2, N=3, sample_n=3, T=MAXLEN, vocab=V):
        super().__init__(M, N, sample_n, T, vocab)
        self.method, self.temp, self.top_k, self.top_p, self.noise = 2, 1.0, 0, 1.0, 0x1000
        self.con = (1.0, 0, 0, None, 0)

    def nbytes(self):
        return _lib.lib().acvae_ensemble_rollout_scratch_bytes(self.M, self.N, self.beam, self.T, self.S.ctypes.data,
                                                               self.E.ctypes.data, self.H.ctypes.data, self.A.ctypes.data, self.V)

    def call(self):
        return _lib.lib().acvae_ensemble_rollout(self.params, self.mem, self.lens, self.eps, self.S.ctypes.data,
                                                 self.E.ctypes.data, self.H.ctypes.data, self.A.ctypes.data, self.M, self.start,
                                                 self.end, self.method, self.temp, self.top_k, self.top_p, self.noise,
                                                 self.seqs, self.logprobs, self.scratch, self.scratch_bytes, self.N,
                                                 self.beam, self.T, self.V, None, *self.con)


def test_ensemble_rollout_refusal_codes():
    """Every case is refused before anything is launched or read on the device: with these pointers a call that got as far
    as its first launch would not return a code at all."""
    ge.build()
    assert _lib.lib().acvae_abi_version() == 3
    for M in (0, -1, 9):
        a = RolloutArgs(); a.M = M
        assert a.call() == EINVAL and a.nbytes() == -1, M
    for field in ("params", "mem", "lens", "eps"):
        a = RolloutArgs()
        getattr(a, field)[1] = None
        assert a.call() == EINVAL, field
    for field in ("params", "mem", "lens", "eps", "seqs", "logprobs", "scratch"):
        a = RolloutArgs()
        setattr(a, field, None)
        assert a.call() == EINVAL, field
    for n in (0, -3):
        a = RolloutArgs(sample_n=n)
        assert a.call() == EINVAL and a.nbytes() == -1, n
    a = RolloutArgs(N=(1 << 20) // 4 + 1, sample_n=4)                  # R > 2^20
    assert a.call() == EUNSUPPORTED and a.nbytes() == -1
    assert RolloutArgs(N=(1 << 20) // 4, sample_n=4).nbytes() > 0
    for temp in (0.0, -1.0, float("nan"), float("inf")):
        a = RolloutArgs(); a.temp = temp
        assert a.call() == EINVAL, temp
    for method in (-1, 3):
        a = RolloutArgs(); a.method = method
        assert a.call() == EINVAL, method
    for method in (1, 2):                                              # a sampling method draws on the caller's noise
        a = RolloutArgs(); a.method, a.noise = method, None
        assert a.call() == EINVAL, method
    for top_k, top_p in ((-1, 1.0), (0, 0.0), (0, 1.5), (0, float("nan"))):
        a = RolloutArgs(); a.top_k, a.top_p = top_k, top_p
        assert a.call() == EINVAL, (top_k, top_p)
    for top_k, top_p in ((3, 1.0), (0, 0.5)):                          # greedy samples nothing to truncate
        a = RolloutArgs(); a.method, a.noise, a.top_k, a.top_p = 0, None, top_k, top_p
        assert a.call() == EINVAL, (top_k, top_p)
    for start, end in ((-1, 2), (V, 2), (1, -1), (1, V)):
        a = RolloutArgs(); a.start, a.end = start, end
        assert a.call() == EINVAL, (start, end)
    for con in ((0.0, 0, 0, None, 0), (1.0, -1, 0, None, 0), (1.0, 0, MAXLEN + 1, None, 0), (1.0, 0, 0, None, 2)):
        a = RolloutArgs(); a.con = con
        assert a.call() == EINVAL, con
    # what is left is well formed: greedy without noise, sampling with it, truncated or not, all get as far as the workspace
    for method, noise, top_k in ((0, None, 0), (1, 0x1000, 0), (2, 0x1000, 0), (2, 0x1000, 5)):
        a = RolloutArgs(); a.method, a.noise, a.top_k = method, noise, top_k
        need = a.nbytes()
        assert need > 0
        a.scratch_bytes = need - 1
        assert a.call() == EWORKSPACE, method
    # the scratch is the search's at beam = sample_n, and grows with the rows
    assert RolloutArgs(sample_n=3).nbytes() == Args(beam=3).nbytes()
    assert RolloutArgs(sample_n=5).nbytes() > RolloutArgs(sample_n=3).nbytes() > RolloutArgs(sample_n=1).nbytes()


# ------------------------------------------------------------------------------------------------ the reference alone
@pytest.mark.parametrize("method", RU.METHODS)
@pytest.mark.parametrize("V_", RU.VS[1:])
def test_reference_alone_leaves_the_decisions_decided(V_, method):
    """For the inputs test_ensemble_rollout_kernels_gpu.test_mix_sample_vs_fp64 draws: the decisions whose float64 top-1 minus
    top-2 score lies within twice the bound, per parameter set (V, M, method, temp) over R = 1, 3, 160.  The kernel test's
    cap applies to this count, and its ceiling to the bound."""
    for M in RU.MS:
        cases = [RU.kernel_inputs(V_, M, R, method) for R in RU.RS]
        cases = [c + mixture_and_bound(c[0]) for c in cases]
        for temp in RU.TEMPS:
            left_out = total = 0
            for rows, noise, v, mixb in cases:
                want, sb = decision_bound(rows, noise, method, temp, v, mixb)
                assert sb.max() <= MAX_BOUND
                left_out += int((want["gap"] <= 2 * sb).sum()); total += len(sb)
            assert left_out <= MAX_LEFT_OUT * total, (V_, M, method, temp, left_out, total)
