"""CPU: ensemble decoding without a GPU - the yardstick itself (tests/ensemble_util.py) against O.beam_search and against
numbers worked out by hand, what acvae_amd.ensemble.Ensemble refuses, and the refusal codes and scratch arithmetic of the
new C entry points (host code: nothing is launched)."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import acvae_oracle as O
import ensemble_util as EU
from acvae_amd import _lib
from acvae_amd.decoder import VAERNNBahdanauAttnDecoder
from acvae_amd.encoder import Cnn10
from acvae_amd.vae_model import Hybrid_VAEModel

V, E, T_FEAT, MAXLEN = 50, 64, 64, 8
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -3, -4


def cpu_model(seed=1, vocab=V, embed=E):
    torch.manual_seed(seed)
    dec = VAERNNBahdanauAttnDecoder(vocab_size=vocab, enc_mem_size=embed, embed_size=embed, hidden_size=embed, dropout=0.0,
                                    num_layers=1, rnn_type="GRU", attn_size=embed)
    return Hybrid_VAEModel(Cnn10(64, 512), dec, posterior_model="PosteriorRNN_hybrid",
                           posterior_args={"hidden_size": embed, "dropout": 0.0}, prior_model="PriorRNN",
                           prior_args={"hidden_size": embed, "dropout": 0.0})


def state_of(model):
    return {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}


@pytest.fixture(scope="module")
def case():
    state = state_of(cpu_model(1))
    feats, _, fl, _ = O.synthetic_batch(3, T_FEAT, V, 7, seed=2, ragged=True)
    eps = torch.randn(3, MAXLEN, 3, E, generator=torch.Generator().manual_seed(3))
    return state, feats, fl, eps, EU.encode(state, feats, fl)


# ------------------------------------------------------------------------------------------------ the yardstick
def test_helper_with_one_member_is_the_oracle_beam_search(case):
    state, feats, fl, eps, enc = case
    rec, orec = {}, {}
    with torch.no_grad():
        want = O.beam_search(state, feats, fl.copy(), 3, MAXLEN, eps, record=orec)
    got, score = EU.ensemble_beam([state], [enc], 3, MAXLEN, [eps], record=rec)
    assert torch.equal(got, want)
    assert min(min(m) for m in orec["margins"]) > 1e-4          # the comparison was not decided by rounding
    for a, b in zip(rec["margins"], orec["margins"]):
        assert len(a) == len(b) == MAXLEN + 1 and np.allclose(a, b, atol=1e-4)
    assert torch.isfinite(score).all() and (score < 0).all()


def test_helper_identical_members_give_the_one_member_tokens(case):
    state, feats, fl, eps, enc = case
    one_b, s1 = EU.ensemble_beam([state], [enc], 3, MAXLEN, [eps])
    three_b, s3 = EU.ensemble_beam([state] * 3, [enc] * 3, 3, MAXLEN, [eps] * 3)
    assert torch.equal(one_b, three_b) and torch.allclose(s1, s3, atol=1e-12)
    g = [eps[:, :, :1]]
    one_g, l1 = EU.ensemble_greedy([state], [enc], MAXLEN, g)
    three_g, l3 = EU.ensemble_greedy([state] * 3, [enc] * 3, MAXLEN, g * 3)
    assert torch.equal(one_g, three_g) and torch.allclose(l1, l3, atol=1e-12)


def test_helper_greedy_keeps_end_after_the_first_end(case):
    state, feats, fl, eps, enc = case
    bumped = dict(state)
    bumped["decoder.classifier.bias"] = state["decoder.classifier.bias"].clone()
    bumped["decoder.classifier.bias"][O.END_IDX] += 3.0
    rec = {}
    seqs, _ = EU.ensemble_greedy([bumped, state], [enc, enc], MAXLEN, [eps[:, :, :1], eps[:, :, 1:2]], record=rec)
    ended = 0
    for i, row in enumerate(seqs.tolist()):
        if O.END_IDX in row[:-1]:
            first = row.index(O.END_IDX)
            ended += 1
            assert row[first:] == [O.END_IDX] * (MAXLEN - first)
            assert len(rec["margins"][i]) == first + 1           # decisions up to and including the <end>
        else:
            assert len(rec["margins"][i]) == MAXLEN
    assert ended > 0


def test_mixing_rule_two_members_three_words_by_hand():
    """Member 0 holds p = (1/2, 1/4, 1/4), member 1 p = (1/10, 3/5, 3/10): the mean is (0.3, 0.425, 0.275), so the ensemble
    picks word 1 although member 0 alone picks word 0; an additive constant on a member's logits changes nothing."""
    l0 = torch.log(torch.tensor([[0.5, 0.25, 0.25]])) + 7.0
    l1 = torch.log(torch.tensor([[0.1, 0.6, 0.3]])) - 2.0
    lp = EU.mix_logprobs([l0, l1])
    want = np.log(np.array([[0.3, 0.425, 0.275]]))
    assert np.allclose(lp.numpy(), want, atol=1e-7)
    assert int(lp.argmax(-1)) == 1 and int(l0.argmax(-1)) == 0
    assert abs(float(torch.exp(lp).sum()) - 1.0) < 1e-7


# ------------------------------------------------------------------------------------------------ Ensemble(models)
def test_ensemble_refusals():
    from acvae_amd.ensemble import Ensemble
    from acvae_amd.seq_train_model import ScstWrapper
    m = cpu_model(1)
    with pytest.raises(ValueError, match="no members"):
        Ensemble([])
    with pytest.raises(ValueError, match="at most 8"):
        Ensemble([m] * 9)
    with pytest.raises(ValueError, match="Hybrid_VAEModel"):
        Ensemble([m, torch.nn.Linear(2, 2)])
    with pytest.raises(ValueError, match="vocab_size"):
        Ensemble([m, cpu_model(2, vocab=V + 1)])
    for what in ("start_idx", "end_idx"):
        other = cpu_model(2)
        setattr(other, what, getattr(other, what) + 5)
        with pytest.raises(ValueError, match=what):
            Ensemble([m, other])
    with pytest.raises(ValueError, match="different devices"):
        Ensemble([m, copy.deepcopy(m).to("meta")])
    ens = Ensemble([ScstWrapper(m), cpu_model(2, embed=128)])          # wrappers unwrapped; E may differ per member
    assert ens.models[0] is m and len(ens.models) == 2 and isinstance(ens.models, torch.nn.ModuleList)
    with pytest.raises(ValueError, match="method"):
        ens(torch.zeros(1, 64, 64), np.array([64]), method="sample")
    assert len(Ensemble([m] * 8).models) == 8


# ------------------------------------------------------------------------------------------------ the C entry points
class Args:
    """A well-formed argument set of acvae_ensemble_search over M members (fake non-null device pointers: every case
    below is refused before anything is launched or read on the device)."""

    def __init__(self, M=2, N=3, beam=3, T=MAXLEN, vocab=V):
        self.M, self.N, self.beam, self.T, self.V = M, N, beam, T, vocab
        self.greedy, self.start, self.end = 0, 1, 2
        n = max(M, 1)
        self.tables = [(ctypes.c_void_p * 35)(*([0x1000] * 35)) for _ in range(n)]
        self.params = (ctypes.c_void_p * n)(*[ctypes.cast(t, ctypes.c_void_p).value for t in self.tables])
        self.mem, self.lens, self.eps = ((ctypes.c_void_p * n)(*([0x1000] * n)) for _ in range(3))
        self.S, self.E, self.H, self.A = (np.full(n, v, np.int32) for v in (4, E, E, E))
        self.seqs = self.logprobs = self.scratch = 0x1000
        self.scratch_bytes = 1 << 40

    def nbytes(self):
        return _lib.lib().acvae_ensemble_search_scratch_bytes(self.M, self.N, self.beam, self.T, self.S.ctypes.data,
                                                              self.E.ctypes.data, self.H.ctypes.data, self.A.ctypes.data, self.V)

    def call(self):
        return _lib.lib().acvae_ensemble_search(self.params, self.mem, self.lens, self.eps, self.S.ctypes.data,
                                                self.E.ctypes.data, self.H.ctypes.data, self.A.ctypes.data, self.M, self.start,
                                                self.end, self.greedy, self.seqs, self.logprobs, self.scratch,
                                                self.scratch_bytes, self.N, self.beam, self.T, self.V, None)


def test_ensemble_search_refusal_codes():
    ge.build()
    for M in (0, -1, 9):
        a = Args(); a.M = M
        assert a.call() == EINVAL, M
    for field in ("params", "mem", "lens", "eps"):                   # a null entry, in any of the member arrays
        a = Args()
        getattr(a, field)[1] = None
        assert a.call() == EINVAL, field
    for field in ("params", "mem", "lens", "eps", "seqs", "logprobs", "scratch"):      # a null array / output
        a = Args()
        setattr(a, field, None)
        assert a.call() == EINVAL, field
    a = Args(); a.H[1] = E + 1                                      # H_m != E_m is a shape the search takes: with room for
    need = a.nbytes()                                               # equal widths only it asks for its workspace (nothing is
    assert need > Args().nbytes()                                   # launched), it does not answer EINVAL
    a.scratch_bytes = need - 1
    assert a.call() == EWORKSPACE
    a.scratch_bytes = Args().nbytes()
    assert a.call() == EWORKSPACE
    a = Args(beam=65)
    assert a.call() == EINVAL
    a = Args(beam=17)                                               # beyond acvae_topk_flat_batched's k <= 16
    assert a.call() == EUNSUPPORTED
    a = Args(beam=3); a.greedy = 1                                  # greedy is beam 1
    assert a.call() == EINVAL
    a = Args(N=(1 << 20) // 4 + 1, beam=4)                          # N * beam > 2^20
    assert a.call() == EUNSUPPORTED and a.nbytes() == -1
    for start, end in ((-1, 2), (V, 2), (1, -1), (1, V)):
        a = Args(); a.start, a.end = start, end
        assert a.call() == EINVAL, (start, end)
    a = Args()
    need = a.nbytes()
    assert need > 0
    a.scratch_bytes = need - 1
    assert a.call() == EWORKSPACE
    lib = _lib.lib()                                                # the mix kernel's launcher
    ptrs = (ctypes.c_void_p * 9)(*([0x1000] * 9)); ld = np.full(9, V, np.int64)
    assert lib.acvae_ensemble_mix(ptrs, ld.ctypes.data, 0, None, 0x1000, V, None, None, 0, 4, V, None) == EINVAL
    assert lib.acvae_ensemble_mix(ptrs, ld.ctypes.data, 9, None, 0x1000, V, None, None, 0, 4, V, None) == EINVAL
    assert lib.acvae_ensemble_mix(ptrs, ld.ctypes.data, 2, None, None, V, None, None, 0, 4, V, None) == EINVAL    # no output
    assert lib.acvae_ensemble_mix(ptrs, ld.ctypes.data, 2, None, 0x1000, V - 1, None, None, 0, 4, V, None) == EINVAL
    ld[1] = V - 1
    assert lib.acvae_ensemble_mix(ptrs, ld.ctypes.data, 2, None, 0x1000, V, None, None, 0, 4, V, None) == EINVAL
    ptrs[1] = None; ld[1] = V
    assert lib.acvae_ensemble_mix(ptrs, ld.ctypes.data, 2, None, 0x1000, V, None, None, 0, 4, V, None) == EINVAL


class BeamArgs:
    """A well-formed argument set of acvae_beam_search (fake non-null device pointers, as Args)."""

    def __init__(self, N=3, beam=3):
        self.table = (ctypes.c_void_p * 35)(*([0x1000] * 35))
        self.params = ctypes.cast(self.table, ctypes.c_void_p).value
        self.mem = self.mem_lens = self.eps = self.seqs = self.attn_weights = self.scratch = 0x1000
        self.start, self.scratch_bytes = 1, 1 << 40
        self.N, self.beam, self.T, self.S, self.E, self.H, self.A, self.V = N, beam, MAXLEN, 4, E, E, E, V

    def nbytes(self):
        return _lib.lib().acvae_beam_search_scratch_bytes(self.N, self.beam, self.T, self.S, self.E, self.H, self.A, self.V)

    def call(self):
        return _lib.lib().acvae_beam_search(self.params, self.mem, self.mem_lens, self.eps, self.start, self.seqs,
                                            self.attn_weights, self.scratch, self.scratch_bytes, self.N, self.beam, self.T,
                                            self.S, self.E, self.H, self.A, self.V, None)


def test_beam_search_refusal_codes():
    """Every case is refused before anything is launched or read on the device: with these pointers a call that got as far
    as its first launch would not return a code at all.  Beam 17 is the case that used to be refused only mid-call, by
    acvae_topk_flat_batched (k <= 16)."""
    ge.build()
    for field in ("params", "mem", "mem_lens", "eps", "seqs", "attn_weights", "scratch"):
        a = BeamArgs()
        setattr(a, field, None)
        assert a.call() == EINVAL, field
    for start in (-1, V):
        a = BeamArgs(); a.start = start
        assert a.call() == EINVAL, start
    a = BeamArgs(); a.H = E + 1                                     # H != E is a shape the search takes: with room for
    need = a.nbytes()                                               # equal widths only it asks for its workspace (nothing is
    assert need > BeamArgs().nbytes()                               # launched), it does not answer EINVAL
    a.scratch_bytes = need - 1
    assert a.call() == EWORKSPACE
    a.scratch_bytes = BeamArgs().nbytes()
    assert a.call() == EWORKSPACE
    for beam in (65, 17):
        assert BeamArgs(beam=beam).call() == EINVAL, beam
    a = BeamArgs(N=(1 << 20) // 4 + 1, beam=4)                      # N * beam > 2^20
    assert a.call() == EUNSUPPORTED and a.nbytes() == -1
    a = BeamArgs()
    need = a.nbytes()
    assert need > 0
    a.scratch_bytes = need - 1
    assert a.call() == EWORKSPACE


def test_ensemble_scratch_bytes_is_host_arithmetic_and_grows_with_members():
    ge.build()
    sizes = [Args(M=M).nbytes() for M in range(1, 9)]
    assert all(s > 0 for s in sizes) and all(b > a for a, b in zip(sizes, sizes[1:]))
    assert len({b - a for a, b in zip(sizes, sizes[1:])}) == 1       # equal members: equal increments
    assert Args(M=0).nbytes() == -1 and Args(M=9).nbytes() == -1
    big, small = Args(M=2), Args(M=2)
    big.E[1] = big.H[1] = big.A[1] = 2 * E                           # a wider member needs more
    assert big.nbytes() > small.nbytes()
    one = Args(M=1, beam=3)                                          # at M = 1: the single-model search's buffers less the
    single = _lib.lib().acvae_beam_search_scratch_bytes(one.N, 3, MAXLEN, 4, E, E, E, V)      # attention-weight history
    assert 0 < one.nbytes() < single + (1 << 16)
