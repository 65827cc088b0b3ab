"""Mirror of ``models/text_encoder.py``: ``PosteriorRNN_hybrid`` (:156-216) and ``PriorRNN`` (:218-268)
with the reference's constructor keywords, parameter names and initialisation (``init`` :25-41)."""
import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .attn_model import Seq2SeqAttention
from .streams import scratch_buffer


def _init_weights(m):
    """models/text_encoder.py:29-41 (the Linear branch is the one that fires here)"""
    if isinstance(m, nn.Linear):
        nn.init.xavier_uniform_(m.weight)
        if m.bias is not None:
            nn.init.constant_(m.bias, 0)


class PosteriorBaseEncoder(nn.Module):
    def __init__(self, word_dim, embed_size, vocab_size):
        super().__init__()
        self.word_dim, self.embed_size, self.vocab_size = word_dim, embed_size, vocab_size
        self.word_embedding = nn.Embedding(vocab_size, word_dim)

    def init(self):
        for m in self.modules():
            m.apply(_init_weights)


class PriorBaseEncoder(nn.Module):
    def __init__(self, word_dim, audiofeats_size, embed_size, vocab_size):
        super().__init__()
        self.word_dim, self.embed_size, self.vocab_size = word_dim, embed_size, vocab_size
        self.audiofeats_size = audiofeats_size
        self.word_embedding = nn.Embedding(vocab_size, word_dim)

    def init(self):
        for m in self.modules():
            m.apply(_init_weights)


def _check_rnn_kwargs(kwargs, what, rnn_default, stacked=False):
    layers = kwargs.get("num_layers", 1)
    if stacked:
        if not isinstance(layers, int) or isinstance(layers, bool) or layers < 1:
            raise ValueError(f"{what}: num_layers must be a positive integer, got {layers!r}")
        if layers > 16:
            raise NotImplementedError(f"{what}: the HIP path implements up to 16 layers")
    elif layers != 1:
        raise NotImplementedError(f"{what}: the HIP path implements num_layers=1")
    if kwargs.get("rnn_type", rnn_default) != rnn_default:
        raise NotImplementedError(f"{what}: the HIP path implements rnn_type={rnn_default}")


def posterior_keep_masks(lens1, Tc, hidden_size, num_layers, p, out=None):
    """The inter-layer dropout masks of the posterior's nn.GRU(num_layers, dropout=p) in training mode, drawn on the CPU
    generator the way torch's CPU GRU draws them over a packed input: for each lower layer k in turn, one
    ``bernoulli_(1 - p)`` over that layer's packed output ``[sum(lens1), 2 * hidden_size]`` (time-major; the rows of a step
    in pack_padded_sequence order).  Returns (or fills ``out``) uint8 [num_layers-1, N, Tc, 2 * hidden_size] in the batch-major
    layout of acvae_posterior_stack_fwd; padded positions are 0.  Host only."""
    lens = torch.as_tensor(np.asarray(lens1), dtype=torch.long).reshape(-1)
    N, W = lens.numel(), 2 * hidden_size
    if out is None:
        out = torch.empty(num_layers - 1, N, Tc, W, dtype=torch.uint8)
    out.zero_()
    if bool((lens[:-1] >= lens[1:]).all()):       # enforce_sorted=True: the rows keep their order
        order = torch.arange(N)
    else:                                          # enforce_sorted=False sorts them by length
        order = torch.sort(lens, descending=True).indices
    sizes = [int((lens > t).sum()) for t in range(Tc)]
    rows = torch.cat([order[:b] for b in sizes])
    steps = torch.cat([torch.full((b,), t, dtype=torch.long) for t, b in enumerate(sizes)])
    for k in range(num_layers - 1):
        m = torch.empty(len(rows), W).bernoulli_(1 - p)
        out[k][rows, steps] = m.to(torch.uint8)
    return out


def dropout_scale(p):
    """1 / (1 - p) as torch's dropout forms it (``noise.div_(1 - p)`` on a float32 tensor)."""
    return float(torch.ones(()).div_(1 - p)) if p < 1 else 0.0


class _PosteriorFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mod, caps_d, lens1_d, eps_q, keep_d, Tc, *weights):
        N = caps_d.shape[0]
        E, Hq, V, NL = mod.embed_size, mod.hidden_size, mod.vocab_size, mod.num_layers
        dev = eps_q.device
        params = mod._text_table()
        upper = mod._upper_table()
        scale = dropout_scale(mod.dropout) if keep_d is not None else 0.0
        saved_b = _lib.call("acvae_posterior_stack_saved_bytes", N, Tc, E, Hq, V, NL)
        scratch_b = _lib.call("acvae_posterior_stack_scratch_bytes", N, Tc, E, Hq, V, NL)
        saved = torch.empty(saved_b, dtype=torch.uint8, device=dev)
        scratch = scratch_buffer(scratch_b, dev)
        qm, ql, qz = (torch.empty(N, Tc, E, device=dev) for _ in range(3))
        utt = torch.empty(N, 2 * Hq, device=dev)
        _lib.persist_status(dev)                 # the device's status words are registered before the first persistent launch
        # one layer: the one-layer entry point (the same code in the library; num_layers = 1 of the stacked call)
        name, extra = ("acvae_posterior_fwd", ()) if NL == 1 else \
            ("acvae_posterior_stack_fwd", (upper, NL, keep_d, scale))
        _lib.call(name, params, *extra, caps_d, caps_d.stride(0), lens1_d, eps_q, qm, ql, qz, utt, saved,
                  saved_b, scratch, scratch_b, N, Tc, E, Hq, V, _lib.current_stream(), _lib.call_flags())
        ctx.set_materialize_grads(False)         # unused outputs arrive as None in backward (no zero-fill launches)
        ctx.mod, ctx.saved, ctx.dims, ctx.scale = mod, saved, (N, Tc, E, Hq, V), scale
        # an OUTPUT kept as a plain ctx attribute forms a tensor -> grad_fn -> ctx -> tensor cycle that is never collected
        ctx.save_for_backward(lens1_d, eps_q, ql, keep_d)
        return qm, ql, qz, utt

    @staticmethod
    def backward(ctx, d_qm, d_ql, d_qz, d_utt):
        mod = ctx.mod
        lens1_d, eps_q, ql, keep_d = ctx.saved_tensors
        N, Tc, E, Hq, V = ctx.dims
        NL = mod.num_layers
        params = mod._text_table()
        grads = [None] * len(params)
        owner = mod._owner() if mod._owner is not None else None
        views = getattr(owner, "_grad_views", None)
        for i, p in enumerate(params):
            if p is not None and p.requires_grad and 10 <= i <= 20:
                grads[i] = _lib.grad_buffer(views, p)
        upper = mod._upper_table()
        # every upper-layer gradient is written (a frozen tensor's into a throwaway buffer)
        upper_g = [_lib.grad_buffer(views, p) if p.requires_grad else torch.empty_like(p) for p in upper]
        c = lambda t: None if t is None else t.contiguous().float()
        scratch_b = _lib.call("acvae_posterior_stack_scratch_bytes", N, Tc, E, Hq, V, NL)
        scratch = scratch_buffer(scratch_b, eps_q.device)
        name, extra = ("acvae_posterior_bwd", ()) if NL == 1 else \
            ("acvae_posterior_stack_bwd", (upper, upper_g, NL, keep_d, ctx.scale))
        _lib.call(name, params, grads, *extra, lens1_d, eps_q, ql, c(d_qm), c(d_ql), c(d_qz),
                  c(d_utt), ctx.saved, ctx.saved.numel(), scratch, scratch_b, N, Tc, E, Hq, V, _lib.current_stream(),
                  _lib.call_flags())
        ctx.saved = None
        if owner is not None and owner._grad_ready_cb is not None:
            owner._grad_ready_cb("text")            # decode backward always precedes this node (it consumes d_q_z)
        pairs = list(zip(params, grads)) + [(p, g if p.requires_grad else None) for p, g in zip(upper, upper_g)]
        outs = [next((g for p, g in pairs if p is w), None) for w in mod._weights()]
        return (None, None, None, None, None, None, *outs)


class PosteriorRNN_hybrid(PosteriorBaseEncoder):
    """q(z_t | caption): BiGRU over the packed caption -> token_mean_log -> (mean, logvar) -> reparam;
    utterance vector = mean_with_lens + max_with_lens of the BiGRU outputs."""

    def __init__(self, word_dim, embed_size, vocab_size, **kwargs):
        super().__init__(word_dim, embed_size, vocab_size)
        self.hidden_size = kwargs.get("hidden_size", 256)
        self.bidirectional = kwargs.get("bidirectional", True)
        self.num_layers = kwargs.get("num_layers", 1)
        self.dropout = kwargs.get("dropout", 0.3)
        self.rnn_type = kwargs.get("rnn_type", "GRU")
        _check_rnn_kwargs(kwargs, "PosteriorRNN_hybrid", "GRU", stacked=True)
        if not self.bidirectional:
            raise NotImplementedError("PosteriorRNN_hybrid: the HIP path implements the bidirectional GRU")
        if word_dim != embed_size:
            raise NotImplementedError("PosteriorRNN_hybrid: word_dim must equal embed_size")
        # dropout only acts between stacked layers; with num_layers=1 torch ignores it (and warns)
        self.network = nn.GRU(word_dim, self.hidden_size, num_layers=self.num_layers, bidirectional=True, batch_first=True,
                              dropout=self.dropout if self.num_layers > 1 else 0.0)
        self.token_mean_log = nn.Linear(2 * self.hidden_size, 2 * embed_size)
        self.init()
        self._owner = None          # Hybrid_VAEModel sets this so the parameter table covers the whole text side

    def _text_table(self):
        if self._owner is not None:
            return self._owner()._text_table()
        t = [None] * _lib.ENUMS_TEXT_N
        n = self.network
        t[10:21] = [self.word_embedding.weight, n.weight_ih_l0, n.weight_hh_l0, n.bias_ih_l0, n.bias_hh_l0,
                    n.weight_ih_l0_reverse, n.weight_hh_l0_reverse, n.bias_ih_l0_reverse, n.bias_hh_l0_reverse,
                    self.token_mean_log.weight, self.token_mean_log.bias]
        return t

    def _upper_table(self):
        """network.*_l{k} and *_l{k}_reverse for k >= 1, in the order of acvae_posterior_stack_fwd's upper table."""
        n = self.network
        return [getattr(n, f"{w}_l{k}{sfx}") for k in range(1, self.num_layers) for sfx in ("", "_reverse")
                for w in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]

    def _weights(self):
        return [p for p in self._text_table()[10:21]] + self._upper_table()

    def keep_p(self):
        """The inter-layer dropout probability the next forward applies (0 when it draws no masks)."""
        return float(self.dropout) if self.training and self.num_layers > 1 and self.dropout > 0 else 0.0

    def forward(self, x, lengths, eps=None, keep=None):
        """x: caption ids [N,L] (float or long, as the collate fn pads with float zeros); lengths: cap_lens.
        eps (optional): the N(0,1) draw to use; default torch.randn on the CPU generator (text_encoder.py:196).
        keep (optional, used when keep_p() > 0): the inter-layer dropout masks [num_layers-1, N, Tc, 2*hidden_size]; default
        posterior_keep_masks on the CPU generator, drawn before eps as nn.GRU draws them inside self.network(...)."""
        dev = self.token_mean_log.weight.device
        lengths = np.asarray(lengths) - 1
        Tc = int(lengths.max())
        N = x.shape[0]
        keep_d = None
        p = self.keep_p()
        if p > 0:
            if keep is None:
                keep = _lib.h2d_fill((self.num_layers - 1, N, Tc, 2 * self.hidden_size), torch.uint8, dev,
                                     lambda buf: posterior_keep_masks(lengths, Tc, self.hidden_size, self.num_layers, p,
                                                                      out=buf))
            keep_d = _lib.h2d(keep, dev, torch.uint8).contiguous()
        caps_d = _lib.h2d(x, dev, torch.long).contiguous()
        lens1_d = _lib.h2d(lengths, dev, torch.long)
        if eps is None:
            eps = torch.randn(N, Tc, self.embed_size)
        eps = _lib.h2d(eps, dev).contiguous()
        qm, ql, qz, utt = _PosteriorFn.apply(self, caps_d, lens1_d, eps, keep_d, Tc, *self._weights())
        return {"q_means": qm, "q_logs": ql, "q_z": qz, "q_means_utt": utt, "q_logs_utt": None, "q_z_utt": None}


class PriorRNN(PriorBaseEncoder):
    """p(z_t | w_<t, z_<t, audio): word-embedding attention over the audio memory + LSTM + mean_log_out +
    reparameterisation (text_encoder.py:218-268).  The per-step arithmetic runs inside acvae_decode_fwd."""

    def __init__(self, word_dim, audiofeats_size, embed_size, vocab_size, **kwargs):
        super().__init__(word_dim, audiofeats_size, embed_size, vocab_size)
        self.hidden_size = kwargs.get("hidden_size", 256)
        self.bidirectional = kwargs.get("bidirectional", False)
        self.num_layers = kwargs.get("num_layers", 1)
        self.dropout = kwargs.get("dropout", 0.3)
        self.rnn_type = kwargs.get("rnn_type", "LSTM")
        _check_rnn_kwargs(kwargs, "PriorRNN", "LSTM")
        if self.bidirectional:
            raise NotImplementedError("PriorRNN: the HIP path implements the unidirectional LSTM")
        if self.hidden_size != embed_size:
            # init_hidden sizes the LSTM state with embed_size (text_encoder.py:240-245)
            raise ValueError("PriorRNN needs hidden_size == embed_size (SURVEY §8)")
        self.word_attn = Seq2SeqAttention(audiofeats_size, word_dim, audiofeats_size)
        self.network = nn.LSTM(word_dim + audiofeats_size + embed_size, self.hidden_size, num_layers=1,
                               bidirectional=False, batch_first=True)
        self.mean_log_out = nn.Linear(self.hidden_size, 2 * embed_size)
        self.init()
        self._owner = None

    def init_hidden(self, bs, device):
        z = lambda: torch.zeros(self.num_layers, bs, self.embed_size, device=device)
        return (z(), z())

    def forward(self, word, enc_mem, hiddens_state, last_z, lens, eps=None):
        """One prior step (inference, no gradient): models/text_encoder.py:247-268.  word [N,1], enc_mem [N,S,E],
        hiddens_state (h, c) each [1,N,E], last_z [N,E], lens [N] -> {"mean","log","hiddens_state","z"}.
        eps: optional N(0,1) draw; default torch.randn on the CPU generator (:259)."""
        if self._owner is None:
            raise RuntimeError("PriorRNN.forward needs the parameters of its Hybrid_VAEModel")
        owner = self._owner()
        _lib.require_cuda(enc_mem)
        dev = enc_mem.device
        enc_mem = enc_mem.contiguous().float()
        N, S, E = enc_mem.shape
        V = self.vocab_size
        w = word.reshape(-1).to(device=dev, dtype=torch.long).contiguous()
        h_prev = hiddens_state[0].reshape(N, E).to(dev).contiguous().float()
        c_prev = hiddens_state[1].reshape(N, E).to(dev).contiguous().float()
        last_z = last_z.reshape(N, E).to(dev).contiguous().float()
        lens_d = torch.as_tensor(lens).to(device=dev, dtype=torch.long).contiguous()
        if eps is None:
            eps = torch.randn(N, E)
        eps = eps.to(dev).contiguous().float()
        with torch.no_grad():
            encproj = owner._encproj(1, enc_mem)
            mean, logv, z, h, c = (torch.empty(N, E, device=dev) for _ in range(5))
            attw = torch.empty(N, S, device=dev)
            H, A = owner.decoder.model.hidden_size, owner.decoder.attn.attn_size
            sb = _lib.call("acvae_step_scratch_bytes", N, S, E, H, A, V)
            scratch = scratch_buffer(sb, dev)
            _lib.call("acvae_prior_step_fwd", owner._text_table(), w, enc_mem, lens_d, encproj, h_prev,
                      c_prev, last_z, eps, mean, logv, z, h, c, attw, scratch, sb, N, S, E, V, _lib.current_stream())
        return {"mean": mean, "log": logv, "hiddens_state": (h.unsqueeze(0), c.unsqueeze(0)), "z": z}
