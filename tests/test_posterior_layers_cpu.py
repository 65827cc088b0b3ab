"""CPU: the stacked posterior (PosteriorRNN_hybrid with num_layers > 1) on the host side - torch's parameter names and shapes
(a reference-layout state dict loads), the configurations that still raise, and the inter-layer dropout masks drawn in the
order torch's CPU nn.GRU draws them."""
import numpy as np
import pytest
import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

from acvae_amd import text_encoder as TE

E, HQ, V = 12, 8, 30


@pytest.mark.parametrize("L", [2, 3])
def test_state_dict_matches_torch_gru_and_a_reference_layout_loads(L):
    q = TE.PosteriorRNN_hybrid(E, E, V, hidden_size=HQ, num_layers=L, dropout=0.3)
    gru = torch.nn.GRU(E, HQ, num_layers=L, bidirectional=True, batch_first=True)
    ours = {k[len("network."):]: tuple(v.shape) for k, v in q.state_dict().items() if k.startswith("network.")}
    assert ours == {k: tuple(v.shape) for k, v in gru.state_dict().items()}
    assert tuple(q.network.weight_ih_l1.shape) == (3 * HQ, 2 * HQ)
    # the reference's PosteriorRNN_hybrid holds the same modules: a state dict in its layout loads, strictly
    ref = {"word_embedding.weight": torch.randn(V, E), "token_mean_log.weight": torch.randn(2 * E, 2 * HQ),
           "token_mean_log.bias": torch.randn(2 * E)}
    ref.update({"network." + k: torch.randn_like(v) for k, v in gru.state_dict().items()})
    q.load_state_dict(ref)
    for k, v in q.state_dict().items():
        assert torch.equal(v, ref[k]), k
    # the tensors the stacked entry points read for the upper layers: torch's order, forward four then _reverse four
    up = q._upper_table()
    assert len(up) == 8 * (L - 1)
    assert up[0] is q.network.weight_ih_l1 and up[4] is q.network.weight_ih_l1_reverse and up[-1] is getattr(
        q.network, f"bias_hh_l{L - 1}_reverse")
    assert len(q._weights()) == 11 + 8 * (L - 1)


def test_what_the_hip_path_still_refuses():
    with pytest.raises(NotImplementedError):
        TE.PriorRNN(E, E, E, V, hidden_size=E, num_layers=2)
    with pytest.raises(NotImplementedError):
        TE.PosteriorRNN_hybrid(E, E, V, hidden_size=HQ, num_layers=2, rnn_type="LSTM")
    with pytest.raises(ValueError):
        TE.PosteriorRNN_hybrid(E, E, V, hidden_size=HQ, num_layers=0)


def test_masks_are_drawn_only_in_training_between_layers():
    q = TE.PosteriorRNN_hybrid(E, E, V, hidden_size=HQ, num_layers=2, dropout=0.3)
    assert q.keep_p() == 0.3
    assert q.eval().keep_p() == 0.0
    assert TE.PosteriorRNN_hybrid(E, E, V, hidden_size=HQ, num_layers=1, dropout=0.3).keep_p() == 0.0
    assert TE.PosteriorRNN_hybrid(E, E, V, hidden_size=HQ, num_layers=3, dropout=0.0).keep_p() == 0.0
    assert TE.dropout_scale(0.3) == float(torch.ones(1).div_(0.7)[0])


def _stacked_restatement(grus, x, lens, masks, p):
    """fp64: one single-layer bidirectional nn.GRU per layer over the packed input, the product's masks (scaled as torch
    scales them) applied to every lower layer's padded output."""
    h = x
    for k, g in enumerate(grus):
        out, _ = g(pack_padded_sequence(h, lens, batch_first=True, enforce_sorted=False))
        h, _ = pad_packed_sequence(out, batch_first=True)
        if masks is not None and k + 1 < len(grus):
            h = h * (masks[k].double() / (1 - p))
    return h


@pytest.mark.parametrize("L", [2, 3])
@pytest.mark.parametrize("order", ["sorted", "unsorted"])
def test_mask_order_matches_torch_gru_dropout(L, order):
    """nn.GRU(num_layers=L, dropout=0.3) in training mode on a packed fp64 input equals the stacked single-layer GRUs with
    the masks posterior_keep_masks draws under the same torch.manual_seed: same generator, same order, same scale."""
    p = 0.3
    lens = np.array([7, 7, 5, 3, 1, 1]) if order == "sorted" else np.array([3, 7, 1, 5, 7, 1])
    N, Tc = len(lens), int(lens.max())
    torch.manual_seed(0)
    ref_gru = torch.nn.GRU(E, HQ, num_layers=L, bidirectional=True, batch_first=True, dropout=p).double().train()
    x = torch.randn(N, Tc, E, dtype=torch.float64)
    grus = []
    for k in range(L):
        g = torch.nn.GRU(E if k == 0 else 2 * HQ, HQ, bidirectional=True, batch_first=True).double()
        g.load_state_dict({n: getattr(ref_gru, n.replace("_l0", f"_l{k}")).detach() for n in g.state_dict()})
        grus.append(g)
    packed = pack_padded_sequence(x, torch.as_tensor(lens), batch_first=True, enforce_sorted=(order == "sorted"))
    for seed in (5, 6):
        torch.manual_seed(seed)
        with torch.no_grad():
            ref, _ = pad_packed_sequence(ref_gru(packed)[0], batch_first=True)
        after_ref = torch.rand(1)
        torch.manual_seed(seed)
        masks = TE.posterior_keep_masks(lens, Tc, HQ, L, p)
        after_ours = torch.rand(1)
        assert masks.shape == (L - 1, N, Tc, 2 * HQ) and masks.dtype == torch.uint8
        assert torch.equal(after_ref, after_ours), "the masks consume a different number of draws than nn.GRU"
        for n in range(N):
            assert not bool(masks[:, n, lens[n]:].any()), "padded positions must stay 0"
        with torch.no_grad():
            got = _stacked_restatement(grus, x, torch.as_tensor(lens), masks, p)
        torch.testing.assert_close(got, ref, atol=1e-10, rtol=0)
        # the dropout acts: without the masks the stacked result differs
        with torch.no_grad():
            plain = _stacked_restatement(grus, x, torch.as_tensor(lens), None, p)
        assert not torch.allclose(plain, ref, atol=1e-6)


def test_masks_fill_a_given_buffer():
    lens = np.array([4, 2, 2])
    torch.manual_seed(1)
    a = TE.posterior_keep_masks(lens, 4, HQ, 3, 0.5)
    buf = torch.full((2, 3, 4, 2 * HQ), 7, dtype=torch.uint8)
    torch.manual_seed(1)
    b = TE.posterior_keep_masks(lens, 4, HQ, 3, 0.5, out=buf)
    assert b is buf and torch.equal(a, buf)


def test_stacked_entry_points_refuse_bad_arguments_before_any_launch():
    """Host checks of acvae_posterior_stack_fwd / _bwd (no GPU needed: they return before any HIP call): a mask needs upper
    layers, upper layers need their tables, and the layer count is 1..16."""
    import ctypes
    import __graft_entry__ as ge
    from acvae_amd import _lib
    ge.build()
    lib = _lib.lib()
    p = 1 << 20                                        # never dereferenced: every call below is refused first
    tab = (ctypes.c_void_p * _lib.ENUMS_TEXT_N)(*([p] * _lib.ENUMS_TEXT_N))
    fwd = lambda up, L, keep: lib.acvae_posterior_stack_fwd(tab, up, L, keep, 1.0, p, 8, p, p, p, p, p, p, p, 1 << 40, p,
                                                            1 << 40, 2, 3, 32, 32, 5, None, 0)
    bwd = lambda up, ug, L, keep: lib.acvae_posterior_stack_bwd(tab, tab, up, ug, L, keep, 1.0, p, p, p, p, p, p, p, p,
                                                                1 << 40, p, 1 << 40, 2, 3, 32, 32, 5, None, 0)
    assert fwd(None, 2, None) == -1                   # no upper table
    assert fwd(None, 1, p) == -1                      # a mask with one layer
    assert fwd(tab, 17, None) == -1 and fwd(tab, 0, None) == -1
    assert bwd(tab, None, 2, None) == -1              # no upper gradient table
    assert bwd(None, None, 1, p) == -1
    sb = [lib.acvae_posterior_stack_saved_bytes(2, 3, 32, 32, 5, L) for L in (1, 2, 3)]
    assert sb[0] == lib.acvae_posterior_saved_bytes(2, 3, 32, 32, 5) and sb[0] < sb[1] < sb[2]
    assert lib.acvae_posterior_stack_scratch_bytes(2, 3, 32, 32, 5, 1) == lib.acvae_posterior_scratch_bytes(2, 3, 32, 32, 5)
    assert lib.acvae_posterior_stack_saved_bytes(2, 3, 32, 32, 5, 0) == -1
    assert lib.acvae_posterior_stack_saved_bytes(2, 3, 32, 32, 5, 17) == -1
