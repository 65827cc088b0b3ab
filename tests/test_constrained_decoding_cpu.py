"""CPU: constrained decoding without a GPU - the numpy twin (tests/constrain_util.py) against a brute-force n-gram search,
the new entry points' declarations and refusals (nothing launches), the ValueErrors of the keywords, and the kernel's
resource use from the build's remarks."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import constrain_util as CU
from acvae_amd import _lib
from acvae_amd.decoder import VAERNNBahdanauAttnDecoder
from acvae_amd.encoder import Cnn10
from acvae_amd.search import CONSTRAINTS_OFF
from acvae_amd.vae_model import Hybrid_VAEModel

EINVAL = -1
NEG_INF = np.float32(-np.inf)


# ------------------------------------------------------------------------------------------------ the definition
def test_twin_against_brute_force_over_every_short_history():
    """All histories over a 4-word alphabet up to length 6 (5461 of them), n in 0..4, m in {0, 2}, with and without a
    suppress list: the twin's -inf set is the brute-force ban set (every n-gram of hist + [w] built, for every w) joined
    with end_idx below m and the list, and everything else is untouched bit for bit."""
    V, end_idx = 6, 5
    x = np.array([1.5, -2.0, 0.25, 3.0, -0.5, 0.75], np.float32)
    count = 0
    for L in range(0, 7):
        for hist in itertools.product(range(4), repeat=L):
            count += 1
            for n in range(0, 5):
                brute = CU.banned_set(hist, L, n, V)
                assert brute == CU.ngram_bans(hist, L, n, V), (hist, n)
                for m in (0, 2):
                    for sup in ((), (4, 1)):
                        want = set(brute) | set(sup) | ({end_idx} if L < m else set())
                        y = CU.constrain_row(x, hist, L, end_idx, 1.0, n, m, sup)
                        assert {int(i) for i in np.flatnonzero(np.isneginf(y))} == want, (hist, n, m, sup)
                        keep = [i for i in range(V) if i not in want]
                        assert np.array_equal(y[keep].view(np.int32), x[keep].view(np.int32))
    assert count == sum(4 ** L for L in range(7))


def test_n1_bans_every_word_of_the_history_and_short_histories_ban_nothing():
    assert CU.ngram_bans([3, 1, 3, 2], 4, 1) == {1, 2, 3}
    assert CU.ngram_bans([3, 1, 3, 2], 2, 1) == {1, 3}                    # only h[0..t)
    assert CU.ngram_bans([3, 1], 2, 4) == set()                            # t < n - 1
    assert CU.ngram_bans([7, 8, 7], 3, 2) == {8}                           # "7 8" exists: after 7, ban 8
    assert CU.ngram_bans([7, 8, 9, 7, 8], 5, 3) == {9}
    assert CU.ngram_bans([7, 8, 9, 7, 8], 5, 3, V=9) == set()              # a word outside the vocabulary is skipped


def test_the_penalty_touches_each_distinct_word_once():
    """A word that occurs three times is divided once; zero and negative logits are multiplied; -0.0 keeps its sign bit and
    an existing -inf stays; all in fp32."""
    th = np.float32(1.3)
    x = np.array([2.0, -2.0, 0.0, -0.0, 5.0, -np.inf, 7.0, 1e-3], np.float32)
    hist = [0, 1, 0, 2, 3, 0, 5, 1, 7, 99, -4]                              # 99 and -4: outside [0, V), skipped
    y = CU.constrain_row(x, hist, len(hist), 6, 1.3, 0, 0, ())
    want = x.copy()
    want[0] = x[0] / th
    want[1] = x[1] * th
    want[2] = x[2] * th
    want[3] = x[3] * th
    want[7] = x[7] / th
    assert np.array_equal(y.view(np.int32), want.view(np.int32))
    assert y[0] == np.float32(2.0) / th and y[0] != np.float32(2.0) / th / th
    assert np.signbit(y[3]) and not np.signbit(y[2]) and y[5] == NEG_INF and y[4] == 5.0 and y[6] == 7.0
    # only h[0..t) counts, and the fp32 value of theta is the one used
    y2 = CU.constrain_row(x, hist, 2, 6, 1.3, 0, 0, ())
    assert y2[0] == want[0] and y2[1] == want[1] and y2[7] == x[7]
    assert CU.constrain_row(x, hist, 2, 6, float(th), 0, 0, ())[0] == y2[0]
    # theta < 1 rewards a repeat: the same rule
    assert CU.constrain_row(x, [0, 1], 2, 6, 0.5, 0, 0, ())[0] == np.float32(4.0)
    assert CU.constrain_row(x, [0, 1], 2, 6, 0.5, 0, 0, ())[1] == np.float32(-1.0)


def test_a_ban_wins_over_the_penalty_and_min_length_bans_end_idx():
    x = np.array([2.0, 3.0, 4.0, 5.0], np.float32)
    y = CU.constrain_row(x, [1, 2, 1], 3, 3, 2.0, 2, 5, (0,))
    assert y[0] == NEG_INF                       # suppressed
    assert y[2] == NEG_INF                       # bigram "1 2" exists: banned, although it was penalised first
    assert y[1] == np.float32(1.5)               # penalised once, not banned
    assert y[3] == NEG_INF                       # t = 3 < m = 5
    assert CU.constrain_row(x, [1, 2, 1], 3, 3, 1.0, 0, 3, ())[3] == 5.0    # t = m: end_idx is free again
    assert CU.repeats_ngram([1, 2, 1, 2], 2) and not CU.repeats_ngram([1, 2, 1, 3], 2)


# ------------------------------------------------------------------------------------------------ the C ABI
CON = ["repetition_penalty", "no_repeat_ngram_size", "min_length", "suppress_host", "n_suppress"]


def test_new_symbols_are_declared_and_exported():
    protos, _ = _lib.parse_header()
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("acvae_constrain_logits", "acvae_beam_search_constrained_scratch_bytes",
                 "acvae_ensemble_search_constrained_scratch_bytes"):
        assert name in protos and hasattr(so, name), name
    assert [n for n, _ in protos["acvae_constrain_logits"][1]] == [
        "logits", "ld", "hist", "hist_ld", "t", "R", "V", "end_idx", *CON, "stream"]
    for name, base, added in (("acvae_decode_fwd_constrained", "acvae_decode_fwd_truncated", CON),
                              ("acvae_beam_search_constrained", "acvae_beam_search", ["end_idx"] + CON),
                              ("acvae_ensemble_search_constrained", "acvae_ensemble_search", CON),
                              ("acvae_beam_search_constrained_scratch_bytes", "acvae_beam_search_scratch_bytes", []),
                              ("acvae_ensemble_search_constrained_scratch_bytes", "acvae_ensemble_search_scratch_bytes", [])):
        assert name in protos and hasattr(so, name), name
        a, b = protos[name][1], protos[base][1]
        assert a[:len(b)] == b, name                                        # the base's parameters, in its order and types
        assert [n for n, _ in a[len(b):]] == added, name                    # additions only, behind them
    types = dict(protos["acvae_decode_fwd_constrained"][1])
    assert types["repetition_penalty"] is ctypes.c_float and types["suppress_host"] is ctypes.c_void_p
    assert dict(protos["acvae_beam_search_constrained"][1])["end_idx"] is ctypes.c_int64
    assert _lib.lib().acvae_abi_version() == 3
    assert int(_lib._defs["ACVAE_SUPPRESS_MAX"]) == 64


def test_the_kernel_uses_no_scratch():
    """From the build's resource remarks: the suppress list is indexed by lane inside the kernel arguments, which must not
    become a private copy."""
    import __graft_entry__ as ge
    from acvae_amd import build as b
    ge.build()
    hits = {n: u for n, u in b.resource_usage().items() if "constrain_logits_kernel" in n}
    assert len(hits) == 1, sorted(hits)
    for n, u in hits.items():
        assert u.get("scratch", -1) == 0, f"{n}: {u.get('scratch')} bytes per lane of scratch"


_KEEP = []                                       # host arrays the calls below point into


def _host_table(values, ctype):
    arr = (ctype * len(values))(*values)
    _KEEP.append(arr)
    return ctypes.addressof(arr)


def _call_by_name(name, **over):
    """Every pointer a host buffer, every size small and valid, then `over`: what is refused is refused for `over` alone.
    The ensemble entry reads HOST tables of M entries, which are real here (M = 1)."""
    buf = torch.zeros(1 << 16)
    _KEEP.append(buf)
    ints = dict(N=2, T=3, Tc=3, S=4, E=64, H=64, A=64, V=40, Eenc=64, start_idx=1, end_idx=2, sample_method=2, flags=0,
                top_k=0, ld_caps=0, ld=40, hist_ld=8, t=3, R=2, beam=2, max_length=5, M=1, greedy=0,
                no_repeat_ngram_size=0, min_length=0, n_suppress=0)
    ensemble = "ensemble" in name
    args = []
    for arg, ct in _lib.PROTOS[name][1]:
        if arg in over:
            v = over[arg]
        elif ensemble and arg in ("params", "mem", "mem_lens", "eps"):
            v = _host_table([buf.data_ptr()], ctypes.c_void_p)
        elif ensemble and arg in ("S", "E", "H", "A"):
            v = _host_table([ints[arg]], ctypes.c_int)
        elif ct is ctypes.c_void_p:
            v = None if arg in ("caps", "lens1", "q_z", "ss_flags_host", "dis_flags_host", "emb_keep", "stream",
                                "aux_stream", "suppress_host", "kept") else buf.data_ptr()
        elif ct is ctypes.c_float:
            v = {"temp": 1.0, "top_p": 1.0, "emb_drop_p": 0.0, "repetition_penalty": 1.0}[arg]
        elif arg in ("saved_bytes", "scratch_bytes"):
            v = buf.numel() * 4
        else:
            v = ints[arg]
        args.append(v)
    return getattr(_lib.lib(), name)(*args)


ENTRIES = ("acvae_constrain_logits", "acvae_decode_fwd_constrained", "acvae_beam_search_constrained",
           "acvae_ensemble_search_constrained")


def _ids(*ids):
    return _host_table(list(ids), ctypes.c_int)


@pytest.mark.parametrize("name", ENTRIES)
def test_abi_refusals_need_no_gpu(name):
    """Every refusal comes before any launch: the pointers are host memory and there may be no device at all."""
    for theta in (0.0, -1.5, float("nan"), float("inf"), float("-inf")):
        assert _call_by_name(name, repetition_penalty=theta) == EINVAL, theta
    assert _call_by_name(name, no_repeat_ngram_size=-1) == EINVAL
    assert _call_by_name(name, min_length=-1) == EINVAL
    assert _call_by_name(name, n_suppress=-1, suppress_host=_ids(3)) == EINVAL
    assert _call_by_name(name, n_suppress=65, suppress_host=_ids(*range(3, 68))) == EINVAL
    assert _call_by_name(name, n_suppress=2, suppress_host=None) == EINVAL               # a list is announced, none given
    assert _call_by_name(name, n_suppress=2, suppress_host=_ids(3, 40)) == EINVAL        # an id outside [0, V)
    assert _call_by_name(name, n_suppress=2, suppress_host=_ids(-1, 3)) == EINVAL
    if name != "acvae_constrain_logits":
        T = "Tc" if "decode" in name else "max_length"
        assert _call_by_name(name, min_length=6, **{T: 5}) == EINVAL                    # m > max_length
        # a row must keep a word: V <= n_suppress + max_length + beam
        beam = {} if "decode" in name else {"beam": 2}
        b = 1 if "decode" in name else 2
        for V, nsup in ((5 + b, 0), (5 + b + 3, 3)):
            sup = dict(n_suppress=nsup, suppress_host=_ids(*range(3, 3 + nsup))) if nsup else {}
            assert _call_by_name(name, V=V, no_repeat_ngram_size=2, **{T: 5}, **beam, **sup) == EINVAL, (V, nsup)


def test_the_kernel_entry_with_everything_off_launches_nothing():
    assert _call_by_name("acvae_constrain_logits") == 0                     # (host pointers: a launch would fault)
    assert _call_by_name("acvae_constrain_logits", logits=None, hist=None, n_suppress=0, suppress_host=None) == 0
    # with a control on, the remaining arguments are checked too
    on = dict(no_repeat_ngram_size=2)
    assert _call_by_name("acvae_constrain_logits", logits=None, **on) == EINVAL
    assert _call_by_name("acvae_constrain_logits", hist=None, **on) == EINVAL
    assert _call_by_name("acvae_constrain_logits", ld=39, **on) == EINVAL
    assert _call_by_name("acvae_constrain_logits", hist_ld=2, **on) == EINVAL           # t = 3 words do not fit
    assert _call_by_name("acvae_constrain_logits", end_idx=40, **on) == EINVAL
    assert _call_by_name("acvae_constrain_logits", t=-1, **on) == EINVAL
    assert _call_by_name("acvae_constrain_logits", R=0, **on) == EINVAL


def test_the_decode_forward_refuses_constraints_with_captions_or_a_recorded_rollout():
    d = "acvae_decode_fwd_constrained"
    buf = torch.zeros(64, dtype=torch.long)
    ones = _host_table([1, 1, 1], ctypes.c_int)
    train = dict(caps=buf.data_ptr(), ld_caps=4, lens1=buf.data_ptr(), q_z=buf.data_ptr(), ss_flags_host=ones,
                 dis_flags_host=ones)
    for on in (dict(repetition_penalty=1.2), dict(no_repeat_ngram_size=3), dict(min_length=2),
               dict(n_suppress=1, suppress_host=_ids(5))):
        assert _call_by_name(d, **train, **on) == EINVAL
        for method in (0, 1, 2):
            assert _call_by_name(d, sample_method=method, flags=_lib.FLAG_ROLLOUT_GRAD, **on) == EINVAL
    # the truncation refusals hold in the constrained entry as in its base
    assert _call_by_name(d, top_k=-1) == EINVAL
    assert _call_by_name(d, top_k=5, sample_method=0) == EINVAL


# ------------------------------------------------------------------------------------------------ the keywords
@pytest.fixture(scope="module")
def model():
    V, E = 40, 64
    dec = VAERNNBahdanauAttnDecoder(vocab_size=V, enc_mem_size=E, embed_size=E, hidden_size=E, dropout=0.0, num_layers=1,
                                    rnn_type="GRU", attn_size=E)
    return Hybrid_VAEModel(Cnn10(64, 512), dec, posterior_model="PosteriorRNN_hybrid",
                           posterior_args={"hidden_size": E, "dropout": 0.0}, prior_model="PriorRNN",
                           prior_args={"hidden_size": E, "dropout": 0.0})


ON = (dict(repetition_penalty=1.3), dict(no_repeat_ngram_size=2), dict(min_length=3), dict(suppress_tokens=[0, 3]))


def test_keyword_refusals_name_the_keyword(model):
    """Every refusal is raised in front of the encoder: host tensors never reach a kernel here."""
    feats, lens = torch.zeros(2, 64, 64), np.array([64, 64])
    caps, cap_lens = torch.ones(2, 5, dtype=torch.long), np.array([5, 5])
    model.eval()
    two = lambda **kw: model(feats, lens.copy(), max_length=10, **kw)
    end = int(model.end_idx)
    for bad in (0.0, -1.0, float("nan"), float("inf"), "x", True, 1e-60):
        with pytest.raises(ValueError, match="repetition_penalty"):
            two(repetition_penalty=bad)
    for key in ("no_repeat_ngram_size", "min_length"):
        for bad in (-1, 1.5, "3", True):
            with pytest.raises(ValueError, match=key):
                two(**{key: bad})
    with pytest.raises(ValueError, match="min_length"):
        two(min_length=11)                                                  # > max_length
    for bad in ([40], [-1], [1.5], ["a"], [True], 5, [end], list(range(3, 40)) + list(range(3, 33))):
        with pytest.raises(ValueError, match="suppress_tokens"):
            two(suppress_tokens=bad)
    for kw in ON:
        key = next(iter(kw))
        for method in ("greedy", "sample", "gumbel", "beam"):                # accepted: a value out of range still names itself
            assert model._constraints(dict(method=method, max_length=10, **kw), rollout=True) != CONSTRAINTS_OFF
        with pytest.raises(ValueError, match=key):
            two(method="dbs", **kw)
        with pytest.raises(ValueError, match=key):                           # the 4-input forward
            model(feats, lens.copy(), caps, cap_lens, ss_ratio=0.5, dis_ratio=0, **kw)
        with pytest.raises(ValueError, match=key):
            model.rollout_shared_encoder(feats, lens.copy(), 3, method="dbs", max_length=10, **kw)
        with pytest.raises(ValueError, match=key):                           # a row must keep a word: 40 <= 0..2 + 39 + 1
            two_kw = dict(kw, max_length=39)
            model(feats, lens.copy(), **two_kw)
        with pytest.raises(ValueError, match=key):                           # and beam rows count: 40 <= 2 + 30 + 8
            model(feats, lens.copy(), method="beam", beam_size=8, max_length=32 - len(kw.get("suppress_tokens", ())), **kw)
    model.train()                      # a forward that records a differentiable rollout: train(), gradients, two inputs
    try:
        for kw in ON:
            with pytest.raises(ValueError, match="differentiable rollout"):
                two(method="sample", **kw)
            with pytest.raises(ValueError, match=next(iter(kw))):
                model.rollout_shared_encoder(feats, lens.copy(), 3, method="sample", max_length=10, **kw)
            with torch.no_grad():      # no graph, no refusal
                assert model._constraints(dict(method="sample", max_length=10, **kw), rollout=True) != CONSTRAINTS_OFF
    finally:
        model.eval()


def test_all_off_values_normalise_to_off(model):
    model.eval()
    for kw in (dict(), dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, suppress_tokens=()),
               dict(repetition_penalty=None, no_repeat_ngram_size=None, min_length=None, suppress_tokens=None),
               dict(repetition_penalty=1, suppress_tokens=[]), dict(suppress_tokens=torch.zeros(0, dtype=torch.long)),
               dict(repetition_penalty=1.0 + 1e-12)):                      # float32(theta) is what the kernel would see
        for method, rollout in (("greedy", True), ("dbs", True), ("greedy", False)):     # off is never refused
            assert model._constraints(dict(method=method, **kw), rollout=rollout) == CONSTRAINTS_OFF
    th, n, m, ids = model._constraints(dict(method="beam", max_length=10, repetition_penalty=1.3, no_repeat_ngram_size=np.int64(3),
                                            min_length=2, suppress_tokens=np.array([3, 0])), rollout=True)
    assert (th, n, m, ids) == (float(np.float32(1.3)), 3, 2, (3, 0))
    assert all(type(v) is int for v in (n, m, *ids))
    assert model._constraints(dict(suppress_tokens=torch.tensor([4, 5]), max_length=10), rollout=True)[3] == (4, 5)


def test_ensemble_and_beam_search_validate_the_same_way(model):
    from acvae_amd.ensemble import Ensemble
    feats, lens = torch.zeros(2, 64, 64), np.array([64, 64])
    ens = Ensemble([model])
    for method in ("greedy", "beam"):
        with pytest.raises(ValueError, match="repetition_penalty"):
            ens(feats, lens.copy(), method=method, max_length=10, repetition_penalty=-2.0)
        with pytest.raises(ValueError, match="suppress_tokens"):
            ens(feats, lens.copy(), method=method, max_length=10, suppress_tokens=[int(model.end_idx)])
        with pytest.raises(ValueError, match="min_length"):
            ens(feats, lens.copy(), method=method, max_length=10, min_length=11)
    with pytest.raises(ValueError, match="no_repeat_ngram_size"):
        model.beam_search({}, 10, 3, no_repeat_ngram_size=-1)
    with pytest.raises(TypeError, match="top_k"):
        model.beam_search({}, 10, 3, top_k=3)


def test_ensemble_validates_its_keywords_without_consulting_a_member(model):
    """Ensemble.forward hands acvae_amd.search the ensemble's own vocabulary size and end_idx: the refusals carry the texts a
    single model gives, and no member's validator is called (here the first member's would fail the test)."""
    import copy
    import re
    from acvae_amd.ensemble import Ensemble

    def never(*a, **kw):
        raise AssertionError("Ensemble.forward consulted a member's validator")
    first = copy.copy(model)                                # shares the weights; the shadowing attributes are its own
    for name in ("_constraints", "_finishing", "_truncation", "_records_rollout"):
        object.__setattr__(first, name, never)
    ens = Ensemble([first, model])
    feats, lens = torch.zeros(2, 64, 64), np.array([64, 64])
    end, V = int(model.end_idx), int(model.vocab_size)
    for kw, text in (
            (dict(repetition_penalty=-2.0), "repetition_penalty must be a finite number > 0 (1.0 = off), got -2.0"),
            (dict(no_repeat_ngram_size=1.5), "no_repeat_ngram_size must be an integer >= 0 (0 = off), got 1.5"),
            (dict(min_length=11), "min_length=11 exceeds max_length=10"),
            (dict(suppress_tokens=[end]), f"suppress_tokens must not hold end_idx ({end}): no caption could end"),
            (dict(suppress_tokens=[V]), f"suppress_tokens: {V} is not a vocabulary id in [0, {V})"),
            (dict(method="dbs", beam_size=4, group_size=2, min_length=3),
             "min_length=3 with method='dbs': diverse beam search keeps its histories on the host and is not constrained; use "
             "'greedy', 'sample', 'gumbel' or 'beam'"),
            (dict(method="greedy", finish_on_end=True),
             "finish_on_end=True with method='greedy': finishing belongs to method='beam'"),
            (dict(method="beam", beam_size=3, nbest=2),
             "nbest=2 without finish_on_end=True: it ranks finished hypotheses only"),
            (dict(method="beam", beam_size=3, finish_on_end=True, nbest=4),
             "nbest must be an integer in [1, beam_size = 3], got 4"),
            (dict(method="beam", beam_size=3, finish_on_end=True, length_penalty=-1.0),
             "length_penalty must be a finite number >= 0, got -1.0")):
        with pytest.raises(ValueError, match=re.escape(text)):
            ens(feats, lens.copy(), **dict(dict(method="beam", max_length=10), **kw))
        single = dict(dict(method="beam", max_length=10), **kw)
        with pytest.raises(ValueError, match=re.escape(text)):            # the single model's text is the same one
            model._constraints(single, rollout=True)
            model._finishing(single)


def test_search_functions_and_the_models_delegates_agree(model):
    """acvae_amd.search's validators on the model's values return what the model's one-line delegates return, for the keyword
    sets of this file."""
    from acvae_amd import search
    model.eval()
    V, end, ml = model.vocab_size, model.end_idx, model.max_length
    sets = [dict(method=method, max_length=10, **kw) for kw in ON for method in ("greedy", "sample", "gumbel", "beam")]
    sets += [dict(method=m, **kw) for m in ("greedy", "dbs") for kw in (
        dict(), dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, suppress_tokens=()),
        dict(repetition_penalty=None, no_repeat_ngram_size=None, min_length=None, suppress_tokens=None),
        dict(repetition_penalty=1, suppress_tokens=[]), dict(repetition_penalty=1.0 + 1e-12))]
    sets.append(dict(method="beam", max_length=10, repetition_penalty=1.3, no_repeat_ngram_size=np.int64(3), min_length=2,
                     suppress_tokens=np.array([3, 0])))
    sets.append(dict(suppress_tokens=torch.tensor([4, 5]), max_length=10))
    for kw in sets:
        got = search.constraints(kw, V, end, ml, True, False)
        assert got == model._constraints(kw, rollout=True) and type(got) is tuple, kw
        assert search.truncation(kw, True, False) == model._truncation(kw, rollout=True) == (0, 1.0)
        assert search.finishing(kw, ml) is None and model._finishing(kw) is None
    for kw in (dict(method="beam", beam_size=4, finish_on_end=True),
               dict(method="beam", finish_on_end=True, nbest=3, length_penalty=0.5),
               dict(method="beam", beam_size=2, finish_on_end=np.bool_(True), nbest=np.int64(2), length_penalty=0)):
        assert search.finishing(kw, ml) == model._finishing(kw) and search.finishing(kw, ml) is not None
    for kw in (dict(method="sample", top_k=7, top_p=0.25), dict(method="gumbel", top_p=0.9)):
        assert search.truncation(kw, True, False) == model._truncation(kw, rollout=True) != (0, 1.0)


def test_scst_wrappers_drop_the_new_keywords():
    from acvae_amd import seq_train_model
    kw = seq_train_model._sample_kwargs(dict(max_length=5, temperature=1.0, repetition_penalty=1.3, no_repeat_ngram_size=2,
                                             min_length=2, suppress_tokens=[0]))
    assert not set(kw) & {"repetition_penalty", "no_repeat_ngram_size", "min_length", "suppress_tokens"}
