"""The decode composite (acvae_decode_fwd / acvae_decode_bwd, include/acvae_hip.h) restated in plain torch on the CPU, at any
dtype, and the yardstick its float64 run gives the HIP path.  Nothing from the HIP path enters this file.

decode()     the loop of oracle/acvae_oracle.py hybrid_forward (prior step, decoder step, utterance head) given the words it
             feeds; the steps are oracle.seq2seq_attention / lstm_cell / gru_cell, written out so that a MUTANT (below) can
             reach inside.  tests/test_decode_ref_cpu.py holds its float32 run equal to O.hybrid_forward's text side.
backward()   the gradients of sum_k <out_k, up_k> over a subset of the six upstreams, for every decoder / pnet /
             mean_log_out / ln parameter, mem and q_z (autograd; an output without an upstream contributes nothing, a
             tensor no given upstream reaches gets zeros).
yardstick()  both in float64 and float32 at a Case: per tensor the float64 value and r32 = ratio(float32 run, float64 run),
             ratio(x, ref) = max_i |x_i - ref_i| / max(|ref_i|, rms(ref)).
tolerance()  max(1e-5, 8 r32) max(|ref|, rms(ref)) per element: 1e-5 is the kernel tests' floor (chain_tol); 8 allows for
             what separates two correct fp32 evaluations - another summation order (MFMA accumulation, hoisted attention
             halves, split-K slices) and the attention's fast tanh, whose absolute error 2.5e-7 (csrc/common.h) is about
             four times the library's.
pool_margin() max_with_lens routes a gradient to the arg-max step: the smallest top-1 minus top-2 of the float64 outputs over
             t < len per (row, channel).  Every Case's seed below was chosen on the CPU so that it is >= POOL_MARGIN.

MUTANTS are deliberately wrong variants of the backward (one defect each); tests/test_decode_ref_cpu.py shows that the
tolerance flags every one of them, so the bound is not vacuous."""
import dataclasses
import functools
import math

import torch
import torch.nn.functional as F

import acvae_oracle as O

UPS = ("logits", "outputs", "p_means", "p_logs", "p_z", "p_means_utt")
FWD = ("logits", "outputs", "attn_w", "p_means", "p_logs", "p_z", "p_means_utt", "h", "hp", "cp", "lse")
FLOOR, FACTOR, POOL_MARGIN = 1e-5, 8.0, 1e-4
START, END = 1, 2
MUTANTS = ("no_max_pool", "mean_over_Tc", "embed_once", "mem_one_past", "no_last_dh", "no_last_z", "dis_z_to_q",
           "no_keep_scale", "no_ln_bias", "dqd_share0_only", "softmax_sum_per_share")
SPLIT_MUTANTS = MUTANTS[-2:]        # the two mistakes of an attention backward split into shares of SHARE frames
SHARE = 64                          # frames per attention workgroup of the persistent BPTT (csrc/persist_plan.h PB_RC_FRAMES)


# ---------------------------------------------------------------------------------------------------------- the loop
def _swap_grad(value, grad_from):
    """`value` forward, the gradient of `grad_from` backward."""
    return value.detach() + grad_from - grad_from.detach()


class _EmbedOnce(torch.autograd.Function):
    """MUTANT embed_once: a word that several rows feed at one step receives ONE row's gradient instead of their sum."""

    @staticmethod
    def forward(ctx, table, w):
        ctx.save_for_backward(w)
        ctx.shape = table.shape
        return table[w]

    @staticmethod
    def backward(ctx, d):
        (w,) = ctx.saved_tensors
        g = d.new_zeros(ctx.shape)
        g[w] = d
        return g, None


class _SoftmaxPerShare(torch.autograd.Function):
    """MUTANT softmax_sum_per_share: the softmax backward ds = w (dw - sum_s w dw) with the sum taken over the 64 frames of
    the element's own share instead of over the clip (the shares of a split attention backward do not talk to each other:
    the whole sum has to come from elsewhere)."""

    @staticmethod
    def forward(ctx, score):
        w = torch.softmax(score, dim=-1)
        ctx.save_for_backward(w)
        return w

    @staticmethod
    def backward(ctx, dw):
        (w,) = ctx.saved_tensors
        ds = torch.empty_like(w)
        for s0 in range(0, w.shape[-1], SHARE):
            ws, dws = w[..., s0:s0 + SHARE], dw[..., s0:s0 + SHARE]
            ds[..., s0:s0 + SHARE] = ws * (dws - (ws * dws).sum(-1, keepdim=True))
        return ds


def _split_attention(st, prefix, h, mem, mem_lens, mutant):
    """oracle.seq2seq_attention with its two halves taken apart (qd = h W_q^T, the memory half with the bias), so that a
    SPLIT_MUTANT can reach between them.  Equal to the oracle's up to the rounding of one more addition."""
    W, b, v = st[prefix + ".h2attn.weight"], st[prefix + ".h2attn.bias"], st[prefix + ".v"]
    Hq, S = h.shape[1], mem.shape[1]
    qd = F.linear(h, W[:, :Hq]).unsqueeze(1).expand(-1, S, -1)
    if mutant == "dqd_share0_only":        # MUTANT: the frames of the shares behind the first never reach d qd
        first = (torch.arange(S) < SHARE).view(1, S, 1)
        qd = torch.where(first, qd, qd.detach())
    score = torch.tanh(qd + F.linear(mem, W[:, Hq:], b)) @ v
    mask = torch.arange(S).unsqueeze(0) < torch.as_tensor(mem_lens).view(-1, 1)
    score = score.masked_fill(~mask, -1e10)
    weights = _SoftmaxPerShare.apply(score) if mutant == "softmax_sum_per_share" else torch.softmax(score, dim=-1)
    return (weights.unsqueeze(1) @ mem).squeeze(1), weights


def _dec_table(st):
    """The decoder's [V, E] embedding table (projected pretrained embeddings: Embedding . Linear^T + bias)."""
    if "decoder.word_embeddings.0.weight" in st:
        return F.linear(st["decoder.word_embeddings.0.weight"], st["decoder.word_embeddings.1.weight"],
                        st["decoder.word_embeddings.1.bias"])
    return st["decoder.word_embeddings.weight"]


def decode(state, mem, mem_lens, words, lens1, q_z, eps_p, dis_flags, emb_keep=None, p=0.0, dtype=torch.float64,
           rollout=False, mutant=None):
    """words [N, Tc] long: the word fed at every step.  Teacher-forced form: step t feeds q_z[:, t] to the decoder, or the
    prior's z where dis_flags[t]; rollout form (q_z, lens1, dis_flags unused): every step feeds the prior's z, no
    utterance head, H free.  emb_keep [Tc, N, E] / p: the decoder's embedding dropout.  -> dict of FWD."""
    assert mutant is None or mutant in MUTANTS, mutant
    st = {k: v.to(dtype) for k, v in state.items() if torch.is_tensor(v) and v.dtype.is_floating_point}
    mem = mem.to(dtype)
    if "ln.weight" in st:
        mem = F.linear(mem, st["ln.weight"], st["ln.bias"].detach() if mutant == "no_ln_bias" else st["ln.bias"])
    N, Tc = words.shape
    E = st["pnet.mean_log_out.weight"].shape[1]
    H = st["decoder.model.weight_hh_l0"].shape[1]
    mem_lens = torch.as_tensor(mem_lens)
    att_mem = mem
    if mutant == "mem_one_past":           # the frame behind each row's last one takes that frame's memory gradient too
        idx = torch.arange(N)
        last, nxt = mem_lens - 1, torch.clamp(mem_lens, max=mem.shape[1] - 1)
        leak = torch.zeros_like(mem)
        leak[idx, last] = (mem[idx, nxt] - mem[idx, nxt].detach()) * (nxt != last).to(dtype).unsqueeze(1)
        att_mem = mem + leak
    table = _dec_table(st)
    h, hp, cp, lz = mem.new_zeros(N, H), mem.new_zeros(N, E), mem.new_zeros(N, E), mem.new_zeros(N, E)
    out = {k: [] for k in ("logits", "outputs", "attn_w", "p_means", "p_logs", "p_z")}
    for t in range(Tc):
        w = words[:, t].long()
        x = F.embedding(w, st["pnet.word_embedding.weight"])
        ctx, _ = O.seq2seq_attention(st, "pnet.word_attn", x, att_mem, mem_lens)
        hp, cp = O.lstm_cell(torch.cat([x, ctx, lz], dim=-1), hp, cp, st["pnet.network.weight_ih_l0"],
                             st["pnet.network.weight_hh_l0"], st["pnet.network.bias_ih_l0"], st["pnet.network.bias_hh_l0"])
        ml = F.linear(hp, st["pnet.mean_log_out.weight"], st["pnet.mean_log_out.bias"])
        mean, log = ml[:, :E], ml[:, E:]
        pz = eps_p[t].to(dtype) * torch.exp(.5 * log) + mean
        if rollout or dis_flags[t]:
            z = pz if mutant != "dis_z_to_q" or rollout else _swap_grad(pz, q_z[:, t].to(dtype))
        else:
            z = q_z[:, t].to(dtype)
        emb = _EmbedOnce.apply(table, w) if mutant == "embed_once" else F.embedding(w, table)
        if emb_keep is not None and p > 0.0:
            kept = emb * emb_keep[t].to(dtype)
            emb = _swap_grad(kept * (1.0 / (1.0 - p)), kept) if mutant == "no_keep_scale" else kept * (1.0 / (1.0 - p))
        if mutant in SPLIT_MUTANTS:
            ctx, aw = _split_attention(st, "decoder.attn", h, att_mem, mem_lens, mutant)
        else:
            ctx, aw = O.seq2seq_attention(st, "decoder.attn", h, att_mem, mem_lens)
        h = O.gru_cell(torch.cat((emb, ctx, z), dim=-1), h, st["decoder.model.weight_ih_l0"], st["decoder.model.weight_hh_l0"],
                       st["decoder.model.bias_ih_l0"], st["decoder.model.bias_hh_l0"])
        out["logits"].append(F.linear(h, st["decoder.classifier.weight"], st["decoder.classifier.bias"]))
        # MUTANT no_last_dh: what the last step's output receives directly (d_outputs, the pooled head) never enters BPTT
        out["outputs"].append(h.detach() if mutant == "no_last_dh" and t == Tc - 1 else h)
        out["attn_w"].append(aw); out["p_means"].append(mean); out["p_logs"].append(log); out["p_z"].append(pz)
        lz = pz.detach() if mutant == "no_last_z" else pz
    out = {k: torch.stack(v, 1) for k, v in out.items()}
    out["h"], out["hp"], out["cp"] = h, hp, cp
    out["lse"] = torch.logsumexp(out["logits"], dim=-1)
    if not rollout:
        lens1 = torch.as_tensor(lens1)
        mask = (torch.arange(Tc).unsqueeze(0) < lens1.view(-1, 1)).unsqueeze(-1)
        mean_pool = (out["outputs"] * mask).sum(1) / lens1.unsqueeze(1)
        max_pool = out["outputs"].masked_fill(~mask, -math.inf).max(1).values
        if mutant == "mean_over_Tc":
            mean_pool = _swap_grad(mean_pool, (out["outputs"] * mask).sum(1) / Tc)
        if mutant == "no_max_pool":
            max_pool = max_pool.detach()
        out["p_means_utt"] = F.linear(mean_pool + max_pool, st["mean_log_out.weight"], st["mean_log_out.bias"])
    return out


def grad_keys(state, rollout=False):
    """The state entries acvae_decode_bwd owns, in table order."""
    keys = [k for k in state if k.startswith(("decoder.", "pnet.", "mean_log_out.", "ln."))]
    return [k for k in keys if not (rollout and k.startswith("mean_log_out."))]


def backward(state, mem, mem_lens, words, lens1, q_z, eps_p, dis_flags, ups, emb_keep=None, p=0.0, dtype=torch.float64,
             rollout=False, mutant=None):
    """ups: {name in UPS: tensor}, the given upstreams.  -> (forward dict, gradient dict: "g.<state key>", "d_mem", "d_q_z")."""
    keys = grad_keys(state, rollout)
    st = {k: (v.to(dtype).clone().requires_grad_(True) if k in keys else v) for k, v in state.items()}
    mem_l = mem.to(dtype).clone().requires_grad_(True)
    q_l = None if rollout else q_z.to(dtype).clone().requires_grad_(True)
    out = decode(st, mem_l, mem_lens, words, lens1, q_l, eps_p, dis_flags, emb_keep, p, dtype, rollout, mutant)
    total = sum((out[k] * ups[k].to(dtype)).sum() for k in UPS if k in ups)
    leaves = [st[k] for k in keys] + [mem_l] + ([] if rollout else [q_l])
    got = torch.autograd.grad(total, leaves, allow_unused=True)
    got = [torch.zeros_like(l) if g is None else g for l, g in zip(leaves, got)]
    grads = {"g." + k: g for k, g in zip(keys, got)}
    grads["d_mem"] = got[len(keys)]
    if not rollout:
        grads["d_q_z"] = got[len(keys) + 1]
    return {k: v.detach() for k, v in out.items()}, grads


# ---------------------------------------------------------------------------------------------------------- the measure
def ratio(x, ref):
    """max_i |x_i - ref_i| / max(|ref_i|, rms(ref)), the suite's element-wise measure; an all-zero ref admits only zeros."""
    x, ref = x.detach().double(), ref.detach().double()
    assert x.shape == ref.shape, (x.shape, ref.shape)
    if ref.numel() == 0:
        return 0.0
    err = (x - ref).abs()
    rms = float(ref.pow(2).mean().sqrt())
    if rms == 0.0:
        return 0.0 if float(err.max()) == 0.0 else math.inf
    return float((err / torch.clamp(ref.abs(), min=rms)).max())


def tolerance(ref, r32):
    """Per element: max(1e-5, 8 r32) max(|ref|, rms(ref))."""
    ref = ref.detach().double()
    rms = float(ref.pow(2).mean().sqrt()) if ref.numel() else 0.0
    return max(FLOOR, FACTOR * r32) * torch.clamp(ref.abs(), min=rms)


def excess(got, ref, r32):
    """max_i |got_i - ref_i| / tolerance_i: <= 1 passes.  (0 / 0 -> 0: an exact zero where only zero is admitted.)"""
    got, ref = got.detach().double().cpu(), ref.detach().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if ref.numel() == 0:
        return 0.0
    err, tol = (got - ref).abs(), tolerance(ref, r32)
    q = torch.where(err == 0, torch.zeros_like(err), err / tol)
    return float(torch.nan_to_num(q, nan=math.inf, posinf=math.inf).max())


# ---------------------------------------------------------------------------------------------------------- the cases
@dataclasses.dataclass(frozen=True)
class Case:
    """One shape / input set of the composite.  `path` and `assert_*` say which launches the GPU test means to take; they
    do not enter the reference."""
    name: str
    V: int = 44
    E: int = 64
    H: int = 64
    A: int = 32
    N: int = 3
    Tc: int = 7
    S: int = 5
    ln: bool = True                   # Eenc = 512 -> E through ln; False: Eenc = E, no ln
    proj: int = 0                     # D0 of projected embeddings (0: a plain table)
    p: float = 0.0                    # the decoder's embedding dropout (a keep mask is drawn when > 0)
    dis: str = "none"                 # none | all | alt
    ss: str = "all"                   # all | mixed (the HIP forward's own words are fed where the flag is clear)
    words: str = "random"             # random | same | few | last (every word V - 1)
    full: bool = False                # every row at full length
    ups: tuple = UPS
    rollout: bool = False
    seed: int = 1
    path: str = "persist"             # persist | per_step | no_split | defer | defer_per_step
    persist_ok: bool = True           # what widths_util.plans must say about both persistent launches at this shape
    mem_lens: tuple = ()              # the clips' frames, explicit (N of them, the first S); (): S, S - 2, S - 4, .., 1
    att: str = ""                     # S > 64, persistent: the forward attention the plan must choose (resident | streamed)

    @property
    def Eenc(self):
        return 512 if self.ln else self.E

    def ref_key(self):
        return dataclasses.replace(self, name="", path="", persist_ok=True, att="")

    def frames(self):
        """The clips' memory lengths."""
        if self.mem_lens:
            assert len(self.mem_lens) == self.N and max(self.mem_lens) == self.mem_lens[0] == self.S and min(self.mem_lens) >= 1
            return list(self.mem_lens)
        return ([self.S] + [max(1, self.S - 2 * n) for n in range(1, self.N - 1)] + ([1] if self.N > 1 else []))[:self.N]


def make_state(c):
    """The text side's closed-form state at the case's widths (no encoder, no posterior: the decode calls read neither)."""
    shapes = O.state_shapes(c.V, c.E, c.H, c.A, c.E, c.Eenc, proj_embed=c.proj or None)
    shapes = {k: s for k, s in shapes.items() if k.startswith(("decoder.", "pnet.", "mean_log_out.", "ln."))}
    return O.closed_form_state(shapes)


def dis_flags(c):
    return [{"none": 0, "all": 1, "alt": t % 2}[c.dis] for t in range(c.Tc)]


def ss_flags(c):
    return [1 if c.ss == "all" else (t + 1) % 2 for t in range(c.Tc)]


def inputs(c):
    """Everything a case feeds, float32 on the CPU.  caps [N, Tc + 1] holds the caption words (<start> first); the
    lengths hold both 1 and Tc (N > 1), the memory lengths both 1 and S."""
    g = torch.Generator().manual_seed(1000 * c.seed + 7 * c.N + c.Tc)
    N, Tc, S, E, H, V = c.N, c.Tc, c.S, c.E, c.H, c.V
    lens1 = [Tc] * N if c.full or N == 1 else [max(1, Tc - n) for n in range(N - 1)] + [1]
    pick = {"random": lambda n: torch.randint(3, V, (n,), generator=g), "same": lambda n: torch.full((n,), 5),
            "few": lambda n: torch.tensor([4, 5, V - 1])[torch.randint(0, 3, (n,), generator=g)],
            "last": lambda n: torch.full((n,), V - 1)}[c.words]
    caps = pick(N * (Tc + 1)).view(N, Tc + 1).long()
    if c.words == "random":
        caps[:, 0] = START
        caps[0, Tc - 1] = V - 1
    d = dict(caps=caps, lens1=torch.tensor(lens1), mem=torch.randn(N, S, c.Eenc, generator=g),
             mem_lens=torch.tensor(c.frames()), q_z=torch.randn(N, Tc, E, generator=g),
             eps_p=torch.randn(Tc, N, E, generator=g))
    d["emb_keep"] = (torch.rand(Tc, N, E, generator=g) >= c.p).to(torch.uint8) if c.p > 0 else None
    shapes = dict(logits=(N, Tc, V), outputs=(N, Tc, H), p_means=(N, Tc, E), p_logs=(N, Tc, E), p_z=(N, Tc, E),
                  p_means_utt=(N, 2 * E))
    ups = {k: torch.randn(shapes[k], generator=g) for k in UPS}            # all six drawn, so a subset keeps its values
    d["ups"] = {k: ups[k] for k in c.ups}
    d["noise"] = torch.empty(Tc, N, V).exponential_(1, generator=g) if c.rollout else None
    return d


def fed_words(c, caps, seqs=None):
    """The word fed at every step [N, Tc]: the caption's where the step is teacher-forced, else <start> at step 0 and
    `seqs[:, t - 1]` (another implementation's own words, constants) afterwards."""
    if c.ss == "all" and not c.rollout:
        return caps[:, :c.Tc].clone()
    ss = [0] * c.Tc if c.rollout else ss_flags(c)
    w = torch.empty(c.N, c.Tc, dtype=torch.long)
    for t in range(c.Tc):
        w[:, t] = caps[:, t] if ss[t] else (torch.full((c.N,), START) if t == 0 else seqs[:, t - 1])
    return w


def _run(c, d, words, dtype, mutant=None):
    fwd, grads = backward(make_state(c), d["mem"], d["mem_lens"], words, d["lens1"], d["q_z"], d["eps_p"], dis_flags(c),
                          d["ups"], d["emb_keep"], c.p, dtype, c.rollout, mutant)
    res = {"fwd." + k: v for k, v in fwd.items()}
    res.update(grads)
    return res


def yardstick_for(c, words):
    """{tensor: (float64 value, r32)} at the case's inputs with `words` fed."""
    d = inputs(c)
    r64, r32 = _run(c, d, words, torch.float64), _run(c, d, words, torch.float32)
    return {k: (v, ratio(r32[k], v)) for k, v in r64.items()}


def surrogate_words(c):
    """Words for a case whose fed words are the HIP forward's own (mixed scheduled sampling, rollouts) where no GPU is at
    hand: random ones.  The GPU test replays the real ones."""
    g = torch.Generator().manual_seed(c.seed)
    return torch.randint(3, c.V, (c.N, c.Tc), generator=g)


@functools.lru_cache(maxsize=None)
def _yardstick(key):
    d = inputs(key)
    seqs = None if key.ss == "all" and not key.rollout else surrogate_words(key)
    return yardstick_for(key, fed_words(key, d["caps"], seqs))


def yardstick(c):
    """The case's yardstick with its own caption words (a case that feeds model words: surrogate_words)."""
    return _yardstick(c.ref_key())


def margin_of(outputs, lens1):
    o = outputs.detach().double()
    if o.shape[1] < 2:
        return math.inf
    mask = (torch.arange(o.shape[1]).unsqueeze(0) < torch.as_tensor(lens1).view(-1, 1)).unsqueeze(-1)
    top = o.masked_fill(~mask, -math.inf).topk(2, dim=1).values
    gap = top[:, 0] - top[:, 1]
    return float(gap.min())


def pool_margin(c):
    """The smallest top-1 minus top-2 of the float64 outputs over t < len, per (row, channel); inf without a pool."""
    if c.rollout:
        return math.inf
    return margin_of(yardstick(c)["fwd.outputs"][0], inputs(c)["lens1"])


# The cases of tests/test_decode_composite_gpu.py: the smallest shapes at which each branch can still go wrong.
ALL, ONE = UPS, lambda k: (k,)
_L = dict(A=160, V=51, att="resident")          # E = 64, A = 160: the forward attention keeps S <= 187 frames on the CU
_P = dict(E=512, H=512, N=2, Tc=3, ln=False, V=300, seed=2, att="streamed")      # production E: more than 64 frames are streamed
S_LONG = [
    Case("S66", S=66, **_L),                                               # two shares, the last of 2 frames
    Case("S66-defer", S=66, path="defer", **_L),
    Case("S65", S=65, N=4, mem_lens=(65, 64, 63, 1), seed=2, **_L),              # last share of ONE frame; a clip ends at the share
    Case("S128", S=128, mem_lens=(128, 65, 1), **_L),                      #   boundary, one just inside share 0; two full shares
    Case("S129", S=129, **_L),                                             # three shares, the last of 1 frame
    Case("S130", S=130, **_L),                                             # ... of 2 frames
    Case("S130-per_step", S=130, path="per_step", **_L),
    Case("S187", S=187, N=4, mem_lens=(187, 130, 64, 1), **_L),            # ... of 59; every clip but the first leaves a share
    Case("S187-per_step", S=187, N=4, mem_lens=(187, 130, 64, 1), path="per_step", **_L),           # (or two) fully masked
    Case("S66-Tc1", S=66, Tc=1, **_L),                                     # the launch writes NO row of dqd
    Case("S66-Tc2", S=66, Tc=2, **_L),
    Case("S66-N1", S=66, N=1, seed=2, **_L),
    Case("S66-N32", S=66, N=32, Tc=2, **_L),                               # 64 attention workgroups
    Case("S66-ss_mixed", S=66, ss="mixed", **_L),                          # the context a PER-STEP forward saved in rnn_d
    Case("S66-only_outputs", S=66, ups=ONE("outputs"), **_L),              # NULL d_logits upstream
    Case("S66-emb_dropout", S=66, p=0.3, **_L),                            # the ctx slot between the embedding and z columns
    Case("E512_A512_S66", S=66, A=512, **_P),                              # the batched pb_gemm1_shares (A = 512), ks_rb 3, ks_pa 2
    Case("E512_A256_S130", S=130, A=256, **dict(_P, seed=3)),                            # its one-group-at-a-time form with three shares
    Case("S130_A320", S=130, A=320, V=51, seed=2, att="streamed"),                 # E = 64 streamed: [S][A] does not fit the LDS
]
CASES = [
    # widths (widths_util.TRAIN_SETS) and paths
    Case("E64_A32"),
    Case("E64_A32-per_step", path="per_step"),
    Case("E64_A160", A=160, N=5, Tc=7, S=5),
    Case("E64_A160-per_step", A=160, N=5, Tc=7, S=5, path="per_step"),
    Case("E64_A160-defer", A=160, N=5, Tc=7, S=5, path="defer"),
    Case("E64_A160-defer_per_step", A=160, N=5, Tc=7, S=5, path="defer_per_step"),
    Case("E128_A96", E=128, H=128, A=96, N=5, seed=2),
    Case("E128_A96-per_step", E=128, H=128, A=96, N=5, seed=2, path="per_step"),
    Case("E64_A72", A=72, path="per_step", persist_ok=False),
    Case("E64_A50", A=50, N=4, V=51, path="per_step", persist_ok=False),
    Case("E512_A256", E=512, H=512, A=256, N=2, V=300, Tc=2, ln=False, seed=2),
    Case("E512_A256-per_step", E=512, H=512, A=256, N=2, V=300, Tc=2, ln=False, seed=2, path="per_step"),
    # N
    Case("N1", N=1),
    Case("N32", N=32, Tc=2, A=160),
    Case("N33", N=33, Tc=2, A=160, V=51, path="per_step", persist_ok=False),
    # Tc
    Case("Tc1", Tc=1),
    Case("Tc1-per_step", Tc=1, path="per_step"),
    Case("Tc2-full", Tc=2, full=True),
    # S
    Case("S1", S=1),
    Case("S64", S=64, A=160),
    Case("S64-per_step", S=64, A=160, path="per_step"),
    Case("S64-no_split", S=64, A=160, path="no_split"),
    # S > 64: the persistent BPTT's attention role runs as 2 or 3 workgroups per clip (shares of 64 frames) that hand d qd over
    # as parts and take the softmax backward's sum from <dctx, ctx>; each has a per-step partner on the same reference
    Case("S66-per_step", S=66, A=160, V=51, path="per_step"),
    *S_LONG,
    # words: one owner of all N Tc rows; N Tc across embed_scatter_kernel's bitmap words
    Case("same_word", words="same"),
    Case("rows31", N=31, Tc=1, words="last"),
    Case("rows32", N=16, Tc=2, words="same"),
    Case("rows33", N=11, Tc=3, words="few", V=51),
    Case("rows65", N=13, Tc=5, words="same", path="per_step"),
    # dis flags: any set flag forces the non-persistent, non-deferred backward
    Case("dis_all", dis="all", path="defer"),
    Case("dis_alt", dis="alt", A=160, N=5),
    # scheduled sampling: the HIP forward's own words are replayed
    Case("ss_mixed", ss="mixed", A=160),
    # upstreams: each alone, the rest NULL
    *[Case("only_" + k, ups=ONE(k)) for k in UPS],
    Case("only_p_means+p_logs", ups=("p_means", "p_logs")),
    Case("only_p_means+p_logs-per_step", ups=("p_means", "p_logs"), path="per_step"),
    Case("only_outputs-per_step", ups=ONE("outputs"), path="per_step"),
    Case("only_p_z-dis_alt", ups=ONE("p_z"), dis="alt"),
    # embedding dropout, projected embeddings
    Case("emb_dropout", p=0.3),
    Case("emb_dropout-per_step", p=0.3, path="per_step"),
    Case("proj_embed", proj=24),
    # differentiable rollouts: (E, H, A) of widths_util.INFER_SETS
    Case("rollout_H96_A160", H=96, A=160, rollout=True, ups=ONE("logits"), path="per_step", persist_ok=False),
    Case("rollout_H40_A50", H=40, A=50, rollout=True, ups=ONE("logits"), path="per_step", persist_ok=False),
]
CASE_IDS = [c.name for c in CASES]
assert len(set(CASE_IDS)) == len(CASES)
