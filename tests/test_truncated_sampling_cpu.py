"""CPU: top-k / nucleus sampling without a GPU - the float64 definition (tests/truncate_util.py) against a brute-force loop
on rows whose masses are exact, the new entry points' declarations and refusals, and the ValueErrors of the keywords."""
import ctypes

import numpy as np
import pytest
import torch

import truncate_util as TU
from acvae_amd import _lib
from acvae_amd.decoder import VAERNNBahdanauAttnDecoder
from acvae_amd.encoder import Cnn10
from acvae_amd.vae_model import Hybrid_VAEModel

GUMBEL, MULTINOMIAL = TU.GUMBEL, TU.MULTINOMIAL
EINVAL = -1


# ------------------------------------------------------------------------------------------------ the definition
def four_equal(V, at=(3, 1, 7, 5)):
    x = np.full(V, -100.0, np.float32)
    x[list(at)] = 2.5
    return x


def test_four_equal_logits_and_p_06_keep_exactly_three():
    """pi = 1/4 on four words (the rest hold e^-100 each): the masses in front of ranks 0..4 are 0, 1/4, 1/2, 3/4, 1, so
    p = 0.6 keeps three words whatever the tolerance, and they are the three lowest indices."""
    for V in (8, 300):
        x = four_equal(V)
        for method, temp in ((GUMBEL, 1.0), (GUMBEL, 2.0), (MULTINOMIAL, 1.0), (MULTINOMIAL, 0.5), (MULTINOMIAL, 2.0)):
            lo, hi, order = TU.admissible(x, method, temp, 0, 0.6)
            assert (lo, hi) == (3, 3)
            assert list(order[:4]) == [1, 3, 5, 7]
            assert TU.brute_force_kept(x, method, temp, 0, 0.6) == [1, 3, 5]
            assert TU.admissible(x, method, temp, 2, 0.6)[:2] == (2, 2)         # both: the shorter prefix
            assert TU.admissible(x, method, temp, 5, 0.6)[:2] == (3, 3)
            assert TU.admissible(x, method, temp, 0, 1.0)[:2] == (V, V)         # exactly 1.0 is off
            assert TU.admissible(x, method, temp, 6, 1.0)[:2] == (6, 6)
            assert TU.admissible(x, method, temp, V + 9, 1.0)[:2] == (V, V)
            assert TU.admissible(x, method, temp, 0, 1e-6)[:2] == (1, 1)        # rank 0 is always kept
            # a cut exactly at a prefix mass: rank 2 has 1/2 in front of it, which is not < 1/2 - the definition keeps two,
            # and an fp32 kernel may see the mass a rounding below 1/2: [2, 3]
            assert TU.brute_force_kept(x, method, temp, 0, 0.5) == [1, 3]
            assert TU.admissible(x, method, temp, 0, 0.5)[:2] == (2, 3)
            assert TU.admissible(x, method, temp, 0, 0.5, tol=0.0)[:2] == (2, 2)


def test_util_against_the_brute_force_loop_on_dyadic_masses():
    """Logits that are multiples of log 2 at temp 1: masses 2^-j up to the rounding of log 2 in fp32 (1e-7 relative, far
    from every cut below): the interval collapses to the loop's count, for every (k, p), with duplicates and -inf."""
    rng = np.random.default_rng(0)
    ln2 = np.log(2.0)
    for V in (1, 2, 5, 37):
        for trial in range(6):
            j = rng.integers(0, 6, V)
            x = (-(j * ln2)).astype(np.float32)
            if trial % 3 == 2 and V > 2:
                x[rng.integers(0, V)] = -np.inf
            for method in (GUMBEL, MULTINOMIAL):
                order, before = TU.mass_before(x, method, 1.0)
                assert np.array_equal(order, sorted(range(V), key=lambda i: (-float(x[i]), i)))
                for k in (0, 1, 3, V, V + 2):
                    for cut in range(0, V + 1):
                        # p halfway between two prefix masses: no tolerance can move the count
                        pre = np.concatenate((before, [1.0]))
                        if cut + 1 < pre.size and pre[cut + 1] - pre[cut] > 1e-3:
                            p = 0.5 * (pre[cut] + pre[cut + 1])
                            want = TU.brute_force_kept(x, method, 1.0, k, p)
                            lo, hi, _ = TU.admissible(x, method, 1.0, k, p)
                            assert lo == hi == len(want), (V, trial, method, k, p, lo, hi, want)
                            assert list(order[:lo]) == want


def test_gumbel_ignores_temp_and_multinomial_does_not():
    x = (np.random.default_rng(1).standard_normal(500) * 2).astype(np.float32)
    g = [TU.admissible(x, GUMBEL, t, 0, 0.7)[:2] for t in (0.5, 1.0, 2.0)]
    assert g[0] == g[1] == g[2] == TU.admissible(x, MULTINOMIAL, 1.0, 0, 0.7)[:2]
    m = [TU.admissible(x, MULTINOMIAL, t, 0, 0.7)[0] for t in (0.5, 1.0, 2.0)]
    assert m[0] < m[1] < m[2]
    lo, hi, _ = TU.admissible(x, MULTINOMIAL, 2.0, 0, 0.7)
    assert 0 <= hi - lo <= 3                                           # a few words wide at most
    assert TU.mass_tol(5000) == pytest.approx(2 * (2 * (12 + 20 + 2 * np.log(5000)) + 1) * 2.0 ** -24)
    assert 7.6e-6 < TU.mass_tol(5000) < 1.3e-5


# ------------------------------------------------------------------------------------------------ the C ABI
def test_new_symbols_are_declared_and_exported():
    protos, _ = _lib.parse_header()
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name, base in (("acvae_sample_next_word_truncated", "acvae_sample_next_word"),
                       ("acvae_decode_fwd_truncated", "acvae_decode_fwd_sampled")):
        assert name in protos and hasattr(so, name), name
        a, b = [n for n, _ in protos[name][1]], [n for n, _ in protos[base][1]]
        extra = [n for n in a if n not in b]
        assert len(extra) == 3 and extra[:2] == ["top_k", "top_p"], (name, extra)      # additions only
        assert [n for n in a if n in b] == b
    assert _lib.lib().acvae_abi_version() == 3


def test_the_kernel_keeps_the_row_in_registers():
    """Key, mass and score of up to 32 words per lane live in registers: any scratch would be a global-memory round trip
    inside every probe.  From the build's resource remarks, as test_hot_kernels_keep_everything_in_registers reads them."""
    import __graft_entry__ as ge
    from acvae_amd import build as b
    ge.build()
    hits = {n: u for n, u in b.resource_usage().items() if "sample_trunc_rows_kernel" in n}
    assert len(hits) == 4, sorted(hits)                                 # 4, 20 and 32 words per lane, and the re-reading form
    for n, u in hits.items():
        assert u.get("scratch", -1) == 0, f"{n}: {u.get('scratch')} bytes per lane of scratch"
        assert u.get("vgprs", 999) <= 168, (n, u)                       # three workgroups of four wavefronts per CU at least


def _call_by_name(name, **over):
    """Every pointer a host buffer, every size small and valid, then `over`: what is refused is refused for `over` alone."""
    buf = torch.zeros(1 << 16)
    ints = dict(N=2, T=3, Tc=3, S=4, E=64, H=64, A=64, V=40, Eenc=64, start_idx=1, end_idx=2, method=2, sample_method=2,
                flags=0, top_k=0, ld_n=120, ld_t=40, nz_sn=120, nz_st=40, o_sn=3, o_st=1, ld_caps=0)
    args = []
    for arg, ct in _lib.PROTOS[name][1]:
        if arg in over:
            v = over[arg]
        elif ct is ctypes.c_void_p:
            v = None if arg in ("caps", "lens1", "q_z", "ss_flags_host", "dis_flags_host", "emb_keep", "stream",
                                "aux_stream") else buf.data_ptr()
        elif ct is ctypes.c_float:
            v = {"temp": 1.0, "top_p": 1.0, "emb_drop_p": 0.0}[arg]
        elif arg in ("saved_bytes", "scratch_bytes"):
            v = buf.numel() * 4
        else:
            v = ints[arg]
        args.append(v)
    return getattr(_lib.lib(), name)(*args)


def test_abi_refusals_need_no_gpu():
    for name in ("acvae_sample_next_word_truncated", "acvae_decode_fwd_truncated"):
        assert _call_by_name(name, top_k=-1) == EINVAL
        for p in (0.0, -0.5, 1.0000001, 2.0, float("nan"), float("inf")):
            assert _call_by_name(name, top_p=p) == EINVAL, (name, p)
        assert _call_by_name(name, top_k=-3, top_p=0.5) == EINVAL
    s = "acvae_sample_next_word_truncated"
    assert _call_by_name(s, top_k=5, method=0) == EINVAL                         # greedy draws nothing
    assert _call_by_name(s, top_k=5, temp=0.0) == EINVAL
    assert _call_by_name(s, top_k=5, V=0) == EINVAL
    assert _call_by_name(s, top_k=5, logits=None) == EINVAL
    d = "acvae_decode_fwd_truncated"
    for trunc in (dict(top_k=5), dict(top_p=0.9), dict(top_k=5, top_p=0.9)):
        assert _call_by_name(d, sample_method=0, **trunc) == EINVAL              # ACVAE_SAMPLE_GREEDY
        for method in (1, 2):
            assert _call_by_name(d, sample_method=method, flags=_lib.FLAG_ROLLOUT_GRAD, **trunc) == EINVAL


# ------------------------------------------------------------------------------------------------ the keywords
@pytest.fixture(scope="module")
def model():
    V, E = 40, 64
    dec = VAERNNBahdanauAttnDecoder(vocab_size=V, enc_mem_size=E, embed_size=E, hidden_size=E, dropout=0.0, num_layers=1,
                                    rnn_type="GRU", attn_size=E)
    return Hybrid_VAEModel(Cnn10(64, 512), dec, posterior_model="PosteriorRNN_hybrid",
                           posterior_args={"hidden_size": E, "dropout": 0.0}, prior_model="PriorRNN",
                           prior_args={"hidden_size": E, "dropout": 0.0})


def test_keyword_refusals_name_the_keyword(model):
    """Every refusal is raised in front of the encoder: host tensors never reach a kernel here."""
    feats, lens = torch.zeros(2, 64, 64), np.array([64, 64])
    caps, cap_lens = torch.ones(2, 5, dtype=torch.long), np.array([5, 5])
    model.eval()
    two = lambda **kw: model(feats, lens.copy(), **kw)
    for bad in (-1, 1.5, "3", True):
        with pytest.raises(ValueError, match="top_k"):
            two(method="sample", top_k=bad)
    for bad in (0.0, -0.1, 1.5, float("nan"), "x", 1e-60):
        with pytest.raises(ValueError, match="top_p"):
            two(method="sample", top_p=bad)
    for method in ("greedy", "beam", "dbs"):
        with pytest.raises(ValueError, match="top_k=3"):
            two(method=method, top_k=3)
        with pytest.raises(ValueError, match="top_p=0.9"):
            two(method=method, top_p=0.9)
    with pytest.raises(ValueError, match="top_p"):                          # the default method is greedy
        two(top_p=0.5)
    with pytest.raises(ValueError, match="top_k=5"):
        model(feats, lens.copy(), caps, cap_lens, ss_ratio=0.5, dis_ratio=0, top_k=5)
    with pytest.raises(ValueError, match="top_k"):
        model.rollout_shared_encoder(feats, lens.copy(), 3, method="greedy", top_k=2)
    # a forward that records a differentiable rollout: train() with gradients enabled and two inputs
    model.train()
    try:
        for kw in (dict(top_k=4), dict(top_p=0.9)):
            with pytest.raises(ValueError, match="differentiable rollout"):
                two(method="sample", **kw)
            with pytest.raises(ValueError, match="differentiable rollout"):
                model.rollout_shared_encoder(feats, lens.copy(), 3, method="sample", **kw)
    finally:
        model.eval()
    # off is off: the defaults, spelled out, are the untruncated call and return no truncation
    assert model._truncation(dict(method="greedy", top_k=0, top_p=1.0)) == (0, 1.0)
    assert model._truncation(dict(method="beam", top_k=None, top_p=None)) == (0, 1.0)
    assert model._truncation(dict(method="sample", top_k=7, top_p=0.25)) == (7, 0.25)
    assert model._truncation(dict(method="gumbel", top_p=0.9)) == (0, float(np.float32(0.9)))


def test_scst_wrappers_still_filter_their_keywords():
    from acvae_amd import seq_train_model
    kw = seq_train_model._sample_kwargs(dict(max_length=5, temperature=1.0, top_k=3, top_p=0.5))
    assert "top_k" not in kw and "top_p" not in kw
