"""GPU: the workspace contract of the composite entries of the C ABI (include/acvae_hip.h, DESIGN.md "Workspace contract").

Every entry below is called THROUGH THE C ABI (_lib.call) with each workspace argument a guarded view (tests/ws_guard.py)
of EXACTLY the bytes its `*_bytes` function returns, three times on the same inputs, seeds and dropout masks:
once per fill of FILLS (0x00; 0xFF = NaN / -1 / full counters), and once more in a buffer that holds what the same entry
left behind at a DIFFERENT shape (the stale case production meets through the caching allocator).  Asserted:

  (a) every guard is intact (the autouse fixture checks them again when the test is through);
  (b) every output and every gradient is bit-identical across the three runs (torch.equal, no tolerance) and holds no NaN;
  (c) with the declared size of a workspace reduced by 64 bytes the call returns ACVAE_EWORKSPACE, and the NaN-prefilled
      outputs, the running statistics, the workspace and all guards are untouched.  (The two step entries share ONE
      acvae_step_scratch_bytes and acvae_prior_step_fwd is not told H and A: the entry whose layout sets the size must
      refuse, the other one must run inside the guards when its own, smaller layout still fits - StepFam.refuses.)
  (d) one `close` check per entry against the existing Python path at the same inputs: the direct call is wired correctly
      (correctness against the oracle is tested elsewhere).

Words a kernel waits on or counts arrivals in, and where the call itself zeroes them
---------------------------------------------------------------------------------------------------------------------
Two kinds exist.  LAST-ARRIVER TICKETS (column sums, BatchNorm finalize, skinny split-K, fused / grouped TN products, the
split-over-frames attention): a workgroup adds 1 and only compares the old value with the expected count; nobody waits, so
a wrong start value gives a wrong or unwritten result, never a hang.  ARRIVAL COUNTERS of the persistent launches
(decode_persist.hip): workgroups poll them; every poll loop is bounded (pd_wait, spin_limit) and a launch that gives up
writes NaN and sets the registered status words, which every run here checks.  All of both kinds are zeroed INSIDE the
call, in front of its first kernel, so every entry below gets the 0xFF fill; no entry is left with guards only.

entry                               words                                            zeroed by the call at
----------------------------------  -----------------------------------------------  ---------------------------------------
acvae_encoder_fwd (Cnn10 / Cnn14)   column-sum / bn_finalize tickets at scratch +    csrc/encoder.hip:640 colsum_tickets_reset
                                    s_dpart (conv.hip CS_TICKETS = 128 words)
acvae_encoder_bwd / _bwd_hooked     the same tickets                                 csrc/encoder.hip:782 colsum_tickets_reset
acvae_encoder_fwd (ResNet38)        the same tickets                                 csrc/encoder.hip:397 (r38_fwd)
acvae_encoder_bwd* (ResNet38)       the same tickets                                 csrc/encoder.hip:486 (r38_bwd)
acvae_posterior_stack_fwd           skinny split-K tickets; persistent BiGRU         csrc/decoder.hip:327-334 ZeroBatch
                                    counters pq_cnt and its hand-over buffer         (zb_skinny :328, pq_cnt :330, pq_hbuf :331)
                                    pq_hbuf, one set per layer
acvae_posterior_stack_bwd           skinny, column-sum and TN tickets; pq_cnt; the   csrc/decoder.hip:424-428 ZeroBatch
                                    embedding-table gradient (an accumulator)        (:425 tickets, :426 pq_cnt, :427 table)
acvae_decode_fwd / _sampled /       skinny tickets of both chains; the split         csrc/decoder.hip:660-666 ZeroBatch
_truncated / _constrained           attention's counters attfws_d / attfws_p;        (:661 skinny, :662 attention, :663 pd_cnt,
                                    persistent decode counters pd_cnt; h_{-1}         :665 h0)
acvae_decode_bwd                    skinny / column-sum / TN tickets of both         csrc/decoder.hip:1018-1031 ZeroBatch
                                    chains; persistent BPTT counters pd_cnt_b and    (:1019 tickets, :1021 pd_cnt_b, :1022
                                    the accumulator dmem_p; with clips of more       dmem_p, :1025 dqd, :1030 tables)
                                    than 64 frames dqd, whose step-0 rows that
                                    launch never writes; both embedding-table
                                    gradients
   a persistent launcher zeroes its own counters when its caller has not (no ACVAE_FLAG_INT_CNT_ZEROED):
                                                                                     csrc/decode_persist.hip:1405
acvae_attn_precompute               none (one GEMM, no workspace)                    -
acvae_prior_step_fwd /              skinny tickets; the split attention's 256        csrc/search.hip:122-123 and :144-145
acvae_decoder_step_fwd              counters at scratch + attws                      (acvae_skinny_ws_reset, step_attws_reset)
acvae_beam_search* /                per member the same two sets inside its step     csrc/search.hip:417-418; the states h / hp /
acvae_ensemble_search*              scratch; the running scores topk                 cp / lz :423-426 and topk :435 are zeroed too

Where the header makes zeroing the caller's job (the first 1024 bytes of acvae_attn_fwd's workspace, reset_tickets = 0 of
the reducers' test entries) the per-op tests zero exactly that region and poison the rest: tests/test_text_kernels_gpu.py,
tests/test_ops_gpu.py, tests/test_handoff_gpu.py, tests/test_gemm_group_gpu.py.  No composite entry has such a region.

Shapes: the smallest at which the layouts' terms still differ.  The decode forward / backward in TRAINING needs H == E
(include/acvae_hip.h: ACVAE_EUNSUPPORTED otherwise), so the training pair runs at two width sets of
widths_util.TRAIN_SETS (A > E and A < E), with the persistent launches and, through ACVAE_FLAG_NO_PERSIST, without them;
the width sets with 3H > 4E and with H < E, A <= E (widths_util.INFER_SETS) run the inference forwards and the
differentiable rollout's forward / backward, where H is free.  The step API, the searches and the ensemble members use
the same two sets.  The whole encoder group runs a second time in a child process with ACVAE_CONV_WINO=0: the layout's
BatchNorm-partials term depends on that switch, which is read once per process.

Guards sit around a workspace, not between the regions inside it: the unequal-width and oracle tests remain the check for
one region running into the next."""
import copy
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import widths_util as W
from acvae_amd import _lib
from acvae_amd import text_encoder as TE
from acvae_amd.ensemble import Ensemble
from acvae_amd.search import _constraint_args, length_norm
from acvae_amd.vae_model import _DecodeFn
from test_dropout_philox_gpu import make_encoder
from ws_guard import FILLS, guarded, ws_guards  # noqa: F401  (autouse fixture: every guard intact after each test)

pytestmark = pytest.mark.gpu
NAN = float("nan")
INT_FILL = -77
V = 37
SHORT = 64
CONSTRAIN = (1.2, 2, 2, (5,))           # repetition_penalty, no_repeat_ngram_size, min_length, suppress_tokens
TRUNCATE = (5, 0.9)                     # top_k, top_p
FINISH = (0.7, 2)                       # length_penalty, nbest


def S():
    return _lib.current_stream()


def nans(*shape):
    return torch.full(shape, NAN, device="cuda")


def ints(*shape, dtype=torch.long):
    return torch.full(shape, INT_FILL, dtype=dtype, device="cuda")


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and \
        torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def close(got, want, what, rtol=1e-5, atol=1e-6):
    """The direct call against the Python path on the same inputs: the same library code, so a loose fp32 bound on the
    scale of the tensor is ample; integers and -inf must match exactly."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not got.dtype.is_floating_point:
        assert torch.equal(got, want), what
        return
    g, w = got.detach().double().cpu(), want.detach().double().cpu()
    fin = torch.isfinite(w)
    assert torch.equal(torch.isfinite(g), fin) and torch.equal(g[~fin], w[~fin]), what
    scale = float(w[fin].abs().max()) if bool(fin.any()) else 0.0
    err = (g[fin] - w[fin]).abs()
    ok = err <= atol * max(scale, 1.0) + rtol * w[fin].abs()
    assert bool(ok.all()), f"{what}: max |err| {float(err.max()):.3e} at scale {scale:.3e}"


class Family:
    """One group of entries at one shape: `sizes()` the declared bytes of its workspaces by name, `fresh()` new prefilled
    outputs in self.O (and the mutable inputs restored), `steps()` the calls in order as (entry, workspace names, fn) with
    fn(ws, nbytes): ws[name] a guarded handle, nbytes[name] the size the call is told."""
    dev = torch.device("cuda")

    def sizes(self):
        raise NotImplementedError

    def fresh(self):
        raise NotImplementedError

    def steps(self):
        raise NotImplementedError

    def refuses(self, step, name):
        """Whether step `step` must refuse workspace `name` told 64 bytes fewer: True for every entry that has a `*_bytes`
        function of its own.  (False: it must accept it; None: either.  Only the step API, whose two entries share one
        function, answers otherwise.)"""
        return True


def run(fam, ws, what):
    nbytes = fam.sizes()
    fam.fresh()
    _lib.persist_status(fam.dev)
    for _entry, _uses, fn in fam.steps():
        fn(ws, nbytes)
    torch.cuda.synchronize()
    _lib.check_persist_status(fam.dev)          # a persistent launch that gave up on a counter would say so here
    for h in ws.values():
        h.check()
    out = {k: v.clone() for k, v in fam.O.items()}
    nan = [k for k, v in out.items() if v.dtype.is_floating_point and bool(torch.isnan(v).any())]
    assert not nan, f"{what}: NaN in {nan}"
    untouched = [k for k, v in out.items() if not v.dtype.is_floating_point and v.numel() and bool((v == INT_FILL).all())]
    assert not untouched, f"{what}: never written: {untouched}"
    return out


def stale_from(src, nbytes):
    """A guarded buffer of `nbytes` whose contents are what `src` (a buffer the entry just used at another shape) holds."""
    h = guarded(nbytes, 0x00, what="stale")
    old = src.view
    assert old.numel() > 0
    h.view.copy_(old.repeat(-(-nbytes // old.numel()))[:nbytes])
    return h


def refusals(fam, what):
    """(c): every workspace of every entry, told 64 bytes fewer: ACVAE_EWORKSPACE, and nothing is touched."""
    nbytes = fam.sizes()
    ws = {k: guarded(n, 0xFF, what=f"{what} {k}") for k, n in nbytes.items()}
    fam.fresh()
    n_refused = 0
    for j, (entry, uses, fn) in enumerate(fam.steps()):
        torch.cuda.synchronize()
        before = {k: v.clone() for k, v in fam.O.items()}
        held = {k: ws[k].view.clone() for k in uses}
        accepted = False
        for k in uses:
            short = dict(nbytes)
            short[k] = nbytes[k] - SHORT
            must = fam.refuses(j, k)
            try:
                fn(ws, short)
            except RuntimeError as exc:
                assert f"{entry} failed: ACVAE_EWORKSPACE" in str(exc), exc
                assert must is not False, f"{what}: {entry} refused {k} - 64 bytes, which its own layout fits into"
                n_refused += 1
            else:
                assert not must, f"{what}: {entry} accepted {k} with 64 bytes fewer than declared"
                accepted = True
        torch.cuda.synchronize()
        if not accepted:
            bad = [k for k in before if not same_bits(before[k], fam.O[k])]
            assert not bad, f"{what}: {entry} refused a short workspace but wrote {bad}"
            assert all(torch.equal(held[k], ws[k].view) for k in uses), f"{what}: {entry} refused but wrote into a workspace"
        for h in ws.values():
            h.check()
        fn(ws, nbytes)                          # for real: the next entry reads what this one leaves
    torch.cuda.synchronize()
    _lib.check_persist_status(fam.dev)
    for h in ws.values():
        h.check()
    return n_refused


def contract(fam, other, what):
    """(a), (b), (c) for `fam`; `other` is the same entries at a different shape, the source of the stale contents.
    Returns the outputs (for the check against the Python path)."""
    nbytes = fam.sizes()
    assert nbytes and all(n > SHORT for n in nbytes.values()), nbytes
    assert nbytes != other.sizes(), "the stale run needs a shape with another layout"
    runs = []
    for fill in FILLS:
        ws = {k: guarded(n, fill, what=f"{what} {k} fill {fill:#04x}") for k, n in nbytes.items()}
        runs.append(run(fam, ws, f"{what} fill {fill:#04x}"))
    ows = {k: guarded(n, 0xFF, what=f"{what} {k} other shape") for k, n in other.sizes().items()}
    run(other, ows, f"{what} other shape")
    ws = {k: stale_from(ows[k], n) for k, n in nbytes.items()}
    runs.append(run(fam, ws, f"{what} stale"))
    for name, r in zip(("fill 0xff", "stale contents"), runs[1:]):
        bad = [k for k in runs[0] if not torch.equal(runs[0][k], r[k])]
        assert not bad, f"{what}: {name} changes {bad} against fill 0x00"
    n = refusals(fam, what)
    assert n >= 1 and (n == sum(len(u) for _, u, _ in fam.steps()) or type(fam).refuses is not Family.refuses)
    return runs[0]


def ptr(h):
    return h.data_ptr()


# ================================================================================================ encoder
ENC_SHAPES = {"Cnn10": ((1, 16), (3, 47)), "Cnn14_16k": ((1, 32), (3, 95)), "ResNet38": ((1, 32), (3, 95))}
ENC_CASES = [(n, d) for n, d in (("Cnn10", "f32"), ("Cnn10", "bf16"), ("Cnn14_16k", "f32"), ("Cnn14_16k", "bf16"),
                                 ("ResNet38", "f32"))]


@functools.lru_cache(maxsize=1)
def encoder(name, dtype):
    """The encoder and a pristine copy of its state (the forward updates the running statistics in place)."""
    enc = make_encoder(name, dtype)
    return enc, {k: v.detach().clone() for k, v in enc.state_dict().items()}


def enc_site_shapes(enc, name, N, T):
    if name == "ResNet38":
        return enc.site_shapes(N, T)[1]
    chans, out, h, w = [64, 128, 256, 512, 1024, 2048], [], T, 64
    for b in range(enc.N_BLOCKS):
        if b < enc.N_BLOCKS - 1 or name == "Cnn10":
            h, w = h // 2, w // 2
        out.append((N, chans[b], h, w))
    return out + [(N, enc.OUT_CHANNELS)] * 2


class EncoderFam(Family):
    """acvae_encoder_fwd in training mode with explicit masks, acvae_encoder_bwd on its `saved`, the forward again (the
    backward may work inside `saved`), acvae_encoder_bwd_hooked."""

    def __init__(self, name, dtype, N, T):
        self.name, self.dtype, self.N, self.T = name, dtype, N, T
        self.enc, self.state0 = encoder(name, dtype)
        self.arch = self.enc._arch()
        g = torch.Generator().manual_seed(100 * N + T)
        self.feats = torch.randn(N, T, 64, generator=g).cuda()
        probs = [0.2] * (len(enc_site_shapes(self.enc, name, N, T)) - 2) + [0.5, 0.5]
        self.masks = [(torch.rand(s, generator=g) >= p).to(torch.uint8).cuda().contiguous()
                      for s, p in zip(enc_site_shapes(self.enc, name, N, T), probs)]
        assert len(self.masks) == self.enc._n_dropout_sites()
        self.S_, self.C = T // self.enc.TIME_DIV, self.enc.OUT_CHANNELS
        self.d_ae = torch.randn(N, self.S_, self.C, generator=g).cuda()
        self.seed = 1234567

    def sizes(self):
        return {"saved": _lib.call("acvae_encoder_saved_bytes", self.arch, self.N, self.T, 64),
                "scratch": _lib.call("acvae_encoder_scratch_bytes", self.arch, self.N, self.T, 64)}

    def table(self):
        return self.enc._param_table()

    def grad_slots(self):
        t = self.table()
        return [i for i, p in enumerate(t) if p.dtype.is_floating_point and p.requires_grad and i < len(t) - 2]

    def fresh(self):
        with torch.no_grad():
            for k, v in self.enc.state_dict().items():
                v.copy_(self.state0[k])
        t = self.table()
        self.O = {"audio_embeds": nans(self.N, self.S_, self.C), "pooled": nans(self.N, self.C)}
        for tag in ("bwd", "hooked"):
            for i in self.grad_slots():
                self.O[f"{tag}.grad{i}"] = torch.full_like(t[i], NAN)
        for i, p in enumerate(t):
            if not p.requires_grad:                    # running_mean / running_var / num_batches_tracked: updated in place
                self.O[f"buffer{i}"] = p

    def steps(self):
        N, T, t = self.N, self.T, self.table()

        def fwd(ws, nb):
            _lib.call("acvae_encoder_fwd", t, self.feats, self.O["audio_embeds"], self.O["pooled"], ptr(ws["saved"]),
                      nb["saved"], ptr(ws["scratch"]), nb["scratch"], self.arch, N, T, 64, 1, 0.2, 0.5, self.seed, self.masks,
                      S())

        def grads(tag):
            slots = set(self.grad_slots())
            return [self.O[f"{tag}.grad{i}"] if i in slots else None for i in range(len(t))]

        def bwd(ws, nb):
            _lib.call("acvae_encoder_bwd", t, grads("bwd"), self.feats, self.d_ae, ptr(ws["saved"]), nb["saved"],
                      ptr(ws["scratch"]), nb["scratch"], self.arch, N, T, 64, 1, 0.2, self.seed, self.masks, S())

        def hooked(ws, nb):
            _lib.call("acvae_encoder_bwd_hooked", t, grads("hooked"), self.feats, self.d_ae, ptr(ws["saved"]), nb["saved"],
                      ptr(ws["scratch"]), nb["scratch"], self.arch, N, T, 64, 1, 0.2, self.seed, self.masks, S(), None, None)

        both = ("saved", "scratch")
        return [("acvae_encoder_fwd", both, fwd), ("acvae_encoder_bwd", both, bwd), ("acvae_encoder_fwd", both, fwd),
                ("acvae_encoder_bwd_hooked", both, hooked)]

    def python_path(self):
        enc = copy.deepcopy(self.enc)
        enc.load_state_dict(self.state0)
        enc.train()
        enc.dropout_masks = [m.clone() for m in self.masks]
        for p in enc.parameters():
            p.grad = None
        out = enc(self.feats, [self.T] * self.N)
        (out["audio_embeds"] * self.d_ae).sum().backward()
        torch.cuda.synchronize()
        want = {"audio_embeds": out["audio_embeds"].detach(), "pooled": out["audio_embeds_pooled"].detach()}
        t = enc._param_table()
        for i in self.grad_slots():
            want[f"bwd.grad{i}"] = t[i].grad
        return want


@pytest.mark.parametrize("shape", [0, 1], ids=["smallest_clip", "odd_heights"])
@pytest.mark.parametrize("name,dtype", ENC_CASES, ids=[f"{n}-{d}" for n, d in ENC_CASES])
def test_encoder_contract(name, dtype, shape):
    (N, T), (No, To) = ENC_SHAPES[name][shape], ENC_SHAPES[name][1 - shape]
    fam, other = EncoderFam(name, dtype, N, T), EncoderFam(name, dtype, No, To)
    got = contract(fam, other, f"{name} {dtype} N={N} T={T}")
    for i in fam.grad_slots():                       # the hooked entry without a hook is the plain one
        assert torch.equal(got[f"bwd.grad{i}"], got[f"hooked.grad{i}"]), i
    for k, want in fam.python_path().items():
        close(got[k], want, f"{name} {dtype} N={N} T={T} {k}")


def test_encoder_contract_without_winograd():
    """ACVAE_CONV_WINO=0 (read once per process, hence the child): every layer takes the implicit GEMM, and the layout's
    BatchNorm-partials term max_bnpart (csrc/encoder.hip make_layout) loses the Winograd data gradient's rows."""
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-p", "no:cacheprovider",
                        "-k", "test_encoder_contract and not without_winograd"], env=dict(os.environ, ACVAE_CONV_WINO="0"),
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert f"{2 * len(ENC_CASES)} passed" in r.stdout, r.stdout[-500:]


# ================================================================================================ posterior
class PosteriorFam(Family):
    """acvae_posterior_stack_fwd / _bwd at NL = 2 with the inter-layer dropout mask, E != Hq."""

    def __init__(self, N, Tc, E, Hq, persist):
        self.N, self.Tc, self.E, self.Hq, self.NL = N, Tc, E, Hq, 2
        self.flags = 0 if persist else _lib.FLAG_NO_PERSIST
        torch.manual_seed(11)
        q = TE.PosteriorRNN_hybrid(E, E, V, hidden_size=Hq, num_layers=2, dropout=0.3)
        with torch.no_grad():
            for prm in q.parameters():
                prm.uniform_(-0.3, 0.3)
        self.q = q.cuda().train()
        g = torch.Generator().manual_seed(7 * N + Tc)
        lens1 = np.array([max(1, Tc - 3 * n) for n in range(N)])
        lens1[-1] = 1
        self.cap_lens = lens1 + 1
        self.caps = torch.randint(1, V, (N, Tc + 1), generator=g)
        self.caps_d, self.lens1 = self.caps.cuda().contiguous(), torch.as_tensor(lens1).cuda()
        self.eps = torch.randn(N, Tc, E, generator=g).cuda()
        torch.manual_seed(5)
        self.keep = TE.posterior_keep_masks(lens1, Tc, Hq, 2, 0.3).cuda().contiguous()
        self.scale = TE.dropout_scale(0.3)
        self.ups = [torch.randn(N, Tc, E, generator=g).cuda() for _ in range(3)] + [torch.randn(N, 2 * Hq, generator=g).cuda()]
        self.dims = (N, Tc, E, Hq, V)

    def sizes(self):
        return {"saved": _lib.call("acvae_posterior_stack_saved_bytes", *self.dims, 2),
                "scratch": _lib.call("acvae_posterior_stack_scratch_bytes", *self.dims, 2)}

    def fresh(self):
        N, Tc, E, Hq = self.N, self.Tc, self.E, self.Hq
        self.params, self.upper = self.q._text_table(), self.q._upper_table()
        self.O = {"q_means": nans(N, Tc, E), "q_logs": nans(N, Tc, E), "q_z": nans(N, Tc, E), "q_means_utt": nans(N, 2 * Hq)}
        for i in range(10, 21):
            self.O[f"grad{i}"] = torch.full_like(self.params[i], NAN)
        for i, p in enumerate(self.upper):
            self.O[f"upper_grad{i}"] = torch.full_like(p, NAN)

    def steps(self):
        O = self.O

        def fwd(ws, nb):
            _lib.call("acvae_posterior_stack_fwd", self.params, self.upper, 2, self.keep, self.scale, self.caps_d,
                      self.caps_d.stride(0), self.lens1, self.eps, O["q_means"], O["q_logs"], O["q_z"], O["q_means_utt"],
                      ptr(ws["saved"]), nb["saved"], ptr(ws["scratch"]), nb["scratch"], *self.dims, S(), self.flags)

        def bwd(ws, nb):
            grads = [O.get(f"grad{i}") for i in range(len(self.params))]
            ug = [O[f"upper_grad{i}"] for i in range(len(self.upper))]
            _lib.call("acvae_posterior_stack_bwd", self.params, grads, self.upper, ug, 2, self.keep, self.scale, self.lens1,
                      self.eps, O["q_logs"], *self.ups, ptr(ws["saved"]), nb["saved"], ptr(ws["scratch"]), nb["scratch"],
                      *self.dims, S(), self.flags)

        both = ("saved", "scratch")
        return [("acvae_posterior_stack_fwd", both, fwd), ("acvae_posterior_stack_bwd", both, bwd)]

    def python_path(self):
        for p in self.q.parameters():
            p.grad = None
        with _lib.override(persist=not self.flags):
            out = self.q(self.caps.float().cuda(), self.cap_lens, eps=self.eps, keep=self.keep)
            outs = [out[k] for k in ("q_means", "q_logs", "q_z", "q_means_utt")]
            torch.autograd.backward(outs, self.ups)
        torch.cuda.synchronize()
        want = dict(zip(("q_means", "q_logs", "q_z", "q_means_utt"), [o.detach() for o in outs]))
        for i in range(10, 21):
            want[f"grad{i}"] = self.params[i].grad
        for i, p in enumerate(self.upper):
            want[f"upper_grad{i}"] = p.grad
        return want


@pytest.mark.parametrize("persist", [True, False], ids=["persistent", "per_step"])
def test_posterior_stack_contract(persist):
    fam, other = PosteriorFam(3, 7, 64, 96, persist), PosteriorFam(5, 9, 64, 96, persist)
    plan = W.plans(3, 7, 5, 64, 64, 64, 96)
    assert plan["post_ok"] == 1                      # Hq % 32 == 0, N <= 32: the persistent recurrence is eligible
    got = contract(fam, other, f"posterior NL=2 E=64 Hq=96 persist={persist}")
    for k, want in fam.python_path().items():
        close(got[k], want, f"posterior {k}")


# ================================================================================================ text models
@functools.lru_cache(maxsize=None)
def text_model(E, H, A):
    m = W.build_model(V, E, H, A, E, state=W.make_state(V, E, H, A, E)).eval()
    m.use_side_stream = False                        # one stream: the direct calls pass aux_stream = NULL
    m.defer_param_grads = False
    assert hasattr(m, "ln") and int(m.start_idx) == 1 and int(m.end_idx) == 2
    return m


DEC_MINE = sorted(set(range(0, 10)) | set(range(21, 35)))


def dec_outputs(O, tag, N, Tc, S_, E, H, train, kept=False):
    O.update({f"{tag}.logits": nans(N, Tc, V), f"{tag}.outputs": nans(N, Tc, H), f"{tag}.seqs": ints(N, Tc),
              f"{tag}.slp": nans(N, Tc), f"{tag}.attw": nans(N, Tc, S_), f"{tag}.pm": nans(N, Tc, E), f"{tag}.pl": nans(N, Tc, E),
              f"{tag}.pz": nans(N, Tc, E), f"{tag}.hfin": nans(N, H), f"{tag}.hp": nans(N, E), f"{tag}.cp": nans(N, E)})
    if train:
        O[f"{tag}.putt"] = nans(N, 2 * E)
    if kept:
        O[f"{tag}.kept"] = ints(N, Tc, dtype=torch.int32)


def dec_out_args(O, tag):
    return [O.get(f"{tag}.{k}") for k in ("logits", "outputs", "seqs", "slp", "attw", "pm", "pl", "pz", "putt", "hfin", "hp", "cp")]


PY_KEYS = ("logits", "outputs", "seqs", "slp", "attw", "pm", "pl", "pz", "putt", "hfin", "hp", "cp", "kept")


class DecodeTrainFam(Family):
    """acvae_decode_fwd (teacher-forced, training) and acvae_decode_bwd: H == E, A free."""

    def __init__(self, name, N, Tc, S_, persist):
        p = W.TRAIN_SETS[name]
        self.E = self.H = E = p["E"]
        self.A = p["A"]
        self.N, self.Tc, self.S_ = N, Tc, S_
        self.flags = 0 if persist else _lib.FLAG_NO_PERSIST
        self.model = text_model(E, E, self.A)
        self.Eenc = self.model.ln.weight.shape[1]
        g = torch.Generator().manual_seed(31 * N + Tc)
        caps, cap_lens = W.ragged_caps(N, Tc + 1, V, g)
        self.caps_d = caps.long().cuda().contiguous()
        self.lens1 = torch.as_tensor(cap_lens - 1).cuda()
        assert int(self.lens1.max()) == Tc and len(set(cap_lens.tolist())) == N
        self.mem = torch.randn(N, S_, self.Eenc, generator=g).cuda()
        self.mem_lens = torch.tensor([max(1, S_ - 2 * n) for n in range(N)]).cuda()
        self.q_z = torch.randn(N, Tc, E, generator=g).cuda()
        self.eps_p = torch.randn(Tc, N, E, generator=g).cuda()
        self.ss, self.dis = (ctypes.c_int * Tc)(*([1] * Tc)), (ctypes.c_int * Tc)(*([0] * Tc))
        self.ups = [torch.randn(s, generator=g).cuda() for s in ((N, Tc, V), (N, Tc, E), (N, Tc, E), (N, Tc, E), (N, Tc, E),
                                                                 (N, 2 * E))]
        self.dims = (N, Tc, S_, E, E, self.A, V, self.Eenc)

    def sizes(self):
        return {"saved": _lib.call("acvae_decode_saved_bytes", *self.dims),
                "scratch": _lib.call("acvae_decode_scratch_bytes", *self.dims)}

    def fresh(self):
        self.params = self.model._text_table()
        self.O = {}
        dec_outputs(self.O, "fwd", self.N, self.Tc, self.S_, self.E, self.H, True)
        self.O["d_mem"], self.O["d_q_z"] = nans(self.N, self.S_, self.Eenc), nans(self.N, self.Tc, self.E)
        for i in DEC_MINE:
            if self.params[i] is not None:
                self.O[f"grad{i}"] = torch.full_like(self.params[i], NAN)

    def steps(self):
        O, m = self.O, self.model

        def fwd(ws, nb):
            _lib.call("acvae_decode_fwd", self.params, self.mem, self.mem_lens, self.caps_d, self.caps_d.stride(0), self.lens1,
                      self.q_z, self.eps_p, self.ss, self.dis, *dec_out_args(O, "fwd"), ptr(ws["saved"]), nb["saved"],
                      ptr(ws["scratch"]), nb["scratch"], *self.dims, int(m.start_idx), int(m.end_idx), S(), None, self.flags)

        def bwd(ws, nb):
            grads = [O.get(f"grad{i}") for i in range(len(self.params))]
            _lib.call("acvae_decode_bwd", self.params, grads, self.mem, self.mem_lens, self.lens1, self.eps_p, self.dis,
                      O["fwd.outputs"], O["fwd.attw"], O["fwd.pl"], *self.ups, O["d_mem"], O["d_q_z"], ptr(ws["saved"]),
                      nb["saved"], ptr(ws["scratch"]), nb["scratch"], *self.dims, S(), None, None, 0.0, self.flags)

        both = ("saved", "scratch")
        return [("acvae_decode_fwd", both, fwd), ("acvae_decode_bwd", both, bwd)]

    def python_path(self):
        m = self.model
        for p in m.parameters():
            p.grad = None
        mem, q_z = self.mem.clone().requires_grad_(True), self.q_z.clone().requires_grad_(True)
        with _lib.override(persist=not self.flags):
            out = _DecodeFn.apply(m, mem, self.mem_lens, self.caps_d, self.lens1, q_z, self.eps_p, [1] * self.Tc,
                                  [0] * self.Tc, self.Tc, None, *m._decode_weights())
            o = dict(zip(PY_KEYS, out))
            torch.autograd.backward([o[k] for k in ("logits", "outputs", "pm", "pl", "pz", "putt")], self.ups)
        torch.cuda.synchronize()
        want = {f"fwd.{k}": v.detach() for k, v in o.items()}
        want["d_mem"], want["d_q_z"] = mem.grad, q_z.grad
        for i in DEC_MINE:
            if self.params[i] is not None:
                want[f"grad{i}"] = self.params[i].grad
        return want


@pytest.mark.parametrize("persist", [True, False], ids=["persistent", "per_step"])
@pytest.mark.parametrize("name", ["E64_A160", "E64_A32"])
def test_decode_training_contract(name, persist):
    fam, other = DecodeTrainFam(name, 3, 7, 5, persist), DecodeTrainFam(name, 4, 9, 6, persist)
    plan = W.plans(3, 7, 5, fam.E, fam.H, fam.A, fam.E)
    assert plan["fwd_ok"] == 1 and plan["bwd_ok"] == 1     # both persistent launches are eligible at this set
    got = contract(fam, other, f"decode training {name} persist={persist}")
    for k, want in fam.python_path().items():
        close(got[k], want, f"decode training {name} {k}")


@pytest.mark.parametrize("persist", [True, False], ids=["persistent", "per_step"])
def test_decode_training_contract_long_clips(persist):
    """Clips of more than 64 frames: the scratch layout holds a non-empty region for the d qd shares of the persistent BPTT's
    split attention role (two shares at S = 66; three at S = 130, the shape whose leftovers the stale run starts from), and
    acvae_decode_bwd zeroes the rows of dqd that launch never writes."""
    name = "E64_A160"
    fam, other = DecodeTrainFam(name, 3, 7, 66, persist), DecodeTrainFam(name, 4, 9, 130, persist)
    plan, oplan = W.plans(3, 7, 66, fam.E, fam.H, fam.A, fam.E), W.plans(4, 9, 130, fam.E, fam.H, fam.A, fam.E)
    for p, n, tc, shares in ((plan, 3, 7, 2), (oplan, 4, 9, 3)):
        assert p["fwd_ok"] == 1 and p["bwd_ok"] == 1 and p["rc_splits"] == shares, p
        assert p["dqd_part_floats"] == shares * n * tc * fam.A and p["dv_rows"] == shares * n, p
    got = contract(fam, other, f"decode training {name} S=66 persist={persist}")
    for k, want in fam.python_path().items():
        close(got[k], want, f"decode training {name} S=66 {k}")


class DecodeInferFam(Family):
    """Where H is free: acvae_decode_fwd in inference, the differentiable rollout (acvae_decode_fwd_sampled with
    ACVAE_FLAG_ROLLOUT_GRAD, then acvae_decode_bwd), acvae_decode_fwd_truncated and acvae_decode_fwd_constrained."""

    def __init__(self, E, H, A, N, Tc, S_):
        self.E, self.H, self.A, self.N, self.Tc, self.S_ = E, H, A, N, Tc, S_
        self.model = text_model(E, H, A)
        self.Eenc = self.model.ln.weight.shape[1]
        g = torch.Generator().manual_seed(17 * N + Tc + H)
        self.mem = torch.randn(N, S_, self.Eenc, generator=g).cuda()
        self.mem_lens = torch.tensor([max(1, S_ - 2 * n) for n in range(N)]).cuda()
        self.eps_p = torch.randn(Tc, N, E, generator=g).cuda()
        self.noise = torch.empty(Tc, N, V).exponential_(1, generator=g).cuda()          # ACVAE_SAMPLE_MULTINOMIAL's draws
        self.dis = (ctypes.c_int * Tc)(*([1] * Tc))
        self.ups = [torch.randn(s, generator=g).cuda() for s in ((N, Tc, V), (N, Tc, H), (N, Tc, E), (N, Tc, E), (N, Tc, E))]
        self.dims = (N, Tc, S_, E, H, A, V, self.Eenc)
        self.mine = [i for i in DEC_MINE if i not in (31, 32)]
        arr = np.ascontiguousarray(CONSTRAIN[3], dtype=np.int32)
        self._suppress = arr
        self.con_args = (CONSTRAIN[0], CONSTRAIN[1], CONSTRAIN[2], arr.ctypes.data_as(ctypes.c_void_p), len(arr))

    def sizes(self):
        return {"saved": _lib.call("acvae_decode_saved_bytes", *self.dims),
                "scratch": _lib.call("acvae_decode_scratch_bytes", *self.dims)}

    def fresh(self):
        self.params = self.model._text_table()
        self.O = {}
        for tag in ("greedy", "rollout", "truncated", "constrained"):
            dec_outputs(self.O, tag, self.N, self.Tc, self.S_, self.E, self.H, False, kept=tag in ("truncated", "constrained"))
        self.O["d_mem"] = nans(self.N, self.S_, self.Eenc)
        for i in self.mine:
            if self.params[i] is not None:
                self.O[f"grad{i}"] = torch.full_like(self.params[i], NAN)

    def steps(self):
        O, m = self.O, self.model
        idx = (int(m.start_idx), int(m.end_idx))

        def head(tag, ws, nb):
            return (self.params, self.mem, self.mem_lens, None, 0, None, None, self.eps_p, None, self.dis, *dec_out_args(O, tag),
                    ptr(ws["saved"]), nb["saved"], ptr(ws["scratch"]), nb["scratch"], *self.dims, *idx, S(), None)

        def greedy(ws, nb):
            _lib.call("acvae_decode_fwd", *head("greedy", ws, nb), 0)

        def rollout(ws, nb):
            _lib.call("acvae_decode_fwd_sampled", *head("rollout", ws, nb), 2, 0.8, self.noise, None, 0.0, _lib.FLAG_ROLLOUT_GRAD)

        def bwd(ws, nb):
            grads = [O.get(f"grad{i}") for i in range(len(self.params))]
            _lib.call("acvae_decode_bwd", self.params, grads, self.mem, self.mem_lens, None, self.eps_p, None,
                      O["rollout.outputs"], O["rollout.attw"], O["rollout.pl"], *self.ups, None, O["d_mem"], None, ptr(ws["saved"]),
                      nb["saved"], ptr(ws["scratch"]), nb["scratch"], *self.dims, S(), None, None, 0.0, _lib.FLAG_ROLLOUT_GRAD)

        def truncated(ws, nb):
            _lib.call("acvae_decode_fwd_truncated", *head("truncated", ws, nb), 2, 0.8, self.noise, None, 0.0, 0, TRUNCATE[0],
                      TRUNCATE[1], O["truncated.kept"])

        def constrained(ws, nb):
            _lib.call("acvae_decode_fwd_constrained", *head("constrained", ws, nb), 2, 0.8, self.noise, None, 0.0, 0, TRUNCATE[0],
                      TRUNCATE[1], O["constrained.kept"], *self.con_args)

        both = ("saved", "scratch")
        return [("acvae_decode_fwd", both, greedy), ("acvae_decode_fwd_sampled", both, rollout), ("acvae_decode_bwd", both, bwd),
                ("acvae_decode_fwd_truncated", both, truncated), ("acvae_decode_fwd_constrained", both, constrained)]

    def python_path(self):
        m = self.model
        want = {}
        sample = (2, 0.8, self.noise)
        for tag, sampling in (("greedy", None), ("rollout", dict(sample=sample, rollout_grad=True)),
                              ("truncated", dict(sample=sample, truncate=TRUNCATE)),
                              ("constrained", dict(sample=sample, truncate=TRUNCATE, constrain=CONSTRAIN))):
            for p in m.parameters():
                p.grad = None
            mem = self.mem.clone().requires_grad_(True)
            out = _DecodeFn.apply(m, mem, self.mem_lens, None, None, None, self.eps_p, None, None, self.Tc, sampling,
                                  *m._decode_weights())
            o = dict(zip(PY_KEYS, out))
            o.pop("putt")
            want.update({f"{tag}.{k}": v.detach() for k, v in o.items()})
            if tag == "rollout":
                torch.autograd.backward([o[k] for k in ("logits", "outputs", "pm", "pl", "pz")], self.ups)
                torch.cuda.synchronize()
                want["d_mem"] = mem.grad
                for i in self.mine:
                    if self.params[i] is not None:
                        want[f"grad{i}"] = self.params[i].grad.clone()
        torch.cuda.synchronize()
        return want


INFER = [W.INFER_SETS[0], W.INFER_SETS[2]]
assert 3 * INFER[0][1] > 4 * INFER[0][0]                                          # 3H > 4E
assert INFER[1][1] < INFER[1][0] and INFER[1][2] <= INFER[1][0]                   # H < E and A <= E
INFER_IDS = [f"E{e}_H{h}_A{a}" for e, h, a in INFER]


@pytest.mark.parametrize("E,H,A", INFER, ids=INFER_IDS)
def test_decode_inference_and_rollout_contract(E, H, A):
    fam, other = DecodeInferFam(E, H, A, 3, 7, 5), DecodeInferFam(E, H, A, 4, 9, 6)
    got = contract(fam, other, f"decode inference E={E} H={H} A={A}")
    assert bool((got["truncated.kept"] >= 1).all()) and bool((got["truncated.kept"] <= TRUNCATE[0]).all())
    for k, want in fam.python_path().items():
        close(got[k], want, f"decode inference E={E} H={H} A={A} {k}")


# ================================================================================================ step API
class StepFam(Family):
    """acvae_attn_precompute (no workspace), then acvae_prior_step_fwd and acvae_decoder_step_fwd on ONE buffer of
    acvae_step_scratch_bytes, with the hoisted projections and with NULL (computed into the scratch)."""

    def __init__(self, E, H, A, N, S_):
        self.E, self.H, self.A, self.N, self.S_ = E, H, A, N, S_
        self.model = text_model(E, H, A)
        g = torch.Generator().manual_seed(13 * N + S_ + A)
        self.mem = torch.randn(N, S_, E, generator=g).cuda()
        self.mem_lens = torch.tensor([max(1, S_ - 4 * n) for n in range(N)]).cuda()
        self.word = torch.randint(3, V, (N,), generator=g).cuda()
        self.h, self.hp, self.cp, self.lz, self.eps = (torch.randn(N, w, generator=g).cuda() * 0.5 for w in (H, E, E, E, E))

    def sizes(self):
        return {"scratch": _lib.call("acvae_step_scratch_bytes", self.N, self.S_, self.E, self.H, self.A, V)}

    def fresh(self):
        N, S_, E, H, A = self.N, self.S_, self.E, self.H, self.A
        self.params = self.model._text_table()
        self.O = {"encproj_d": nans(N, S_, A), "encproj_p": nans(N, S_, E)}
        for tag in ("hoisted", "inside"):
            self.O.update({f"{tag}.mean": nans(N, E), f"{tag}.logv": nans(N, E), f"{tag}.z": nans(N, E), f"{tag}.hp": nans(N, E),
                           f"{tag}.cp": nans(N, E), f"{tag}.attw_p": nans(N, S_), f"{tag}.logits": nans(N, V),
                           f"{tag}.h": nans(N, H), f"{tag}.attw_d": nans(N, S_), f"{tag}.rnn_input": nans(N, 3 * E)})

    def steps(self):
        O, N, S_, E, H, A = self.O, self.N, self.S_, self.E, self.H, self.A

        def pre(which):
            def fn(ws, nb):
                _lib.call("acvae_attn_precompute", self.params, which, self.mem, O["encproj_p" if which else "encproj_d"], N, S_,
                          E, H, A, S())
            return fn

        def prior(tag):
            def fn(ws, nb):
                _lib.call("acvae_prior_step_fwd", self.params, self.word, self.mem, self.mem_lens,
                          O["encproj_p"] if tag == "hoisted" else None, self.hp, self.cp, self.lz, self.eps, O[f"{tag}.mean"],
                          O[f"{tag}.logv"], O[f"{tag}.z"], O[f"{tag}.hp"], O[f"{tag}.cp"], O[f"{tag}.attw_p"], ptr(ws["scratch"]),
                          nb["scratch"], N, S_, E, V, S())
            return fn

        def decoder(tag):
            def fn(ws, nb):
                _lib.call("acvae_decoder_step_fwd", self.params, self.word, self.h, self.mem, self.mem_lens,
                          O["encproj_d"] if tag == "hoisted" else None, O[f"{tag}.z"], O[f"{tag}.logits"], O[f"{tag}.h"],
                          O[f"{tag}.attw_d"], O[f"{tag}.rnn_input"], ptr(ws["scratch"]), nb["scratch"], N, S_, E, H, A, V, S())
            return fn

        one = ("scratch",)
        return [("acvae_attn_precompute", (), pre(0)), ("acvae_attn_precompute", (), pre(1)),
                ("acvae_prior_step_fwd", one, prior("hoisted")), ("acvae_decoder_step_fwd", one, decoder("hoisted")),
                ("acvae_prior_step_fwd", one, prior("inside")), ("acvae_decoder_step_fwd", one, decoder("inside"))]

    def refuses(self, step, name):
        """acvae_step_scratch_bytes sizes ONE buffer for both entries: the larger of the decoder step's layout by (E, H, A)
        and the prior step's, which is not told H and A, by (E, E, E).  Only the entry whose layout sets the size can
        tell that 64 bytes are missing; the other one's own need may still fit, and then it runs (inside the guards)."""
        declared = self.sizes()["scratch"]
        prior_own = _lib.call("acvae_step_scratch_bytes", self.N, self.S_, self.E, self.E, self.E, V)
        if step in (2, 4):
            return declared - SHORT < prior_own
        return True if declared > prior_own else None

    def python_path(self):
        m, N = self.model, self.N
        m._encproj_cache.clear()
        pr = m.pnet(self.word.view(N, 1), self.mem, (self.hp.unsqueeze(0), self.cp.unsqueeze(0)), self.lz, self.mem_lens,
                    eps=self.eps)
        de = m.decoder(word=self.word.view(N, 1), state=self.h.unsqueeze(0), enc_mem=self.mem, enc_mem_lens=self.mem_lens,
                       z=pr["z"])
        want = {"encproj_d": m._encproj(0, self.mem), "encproj_p": m._encproj(1, self.mem)}
        m._encproj_cache.clear()
        for tag in ("hoisted", "inside"):
            want.update({f"{tag}.mean": pr["mean"], f"{tag}.logv": pr["log"], f"{tag}.z": pr["z"],
                         f"{tag}.hp": pr["hiddens_state"][0][0], f"{tag}.cp": pr["hiddens_state"][1][0],
                         f"{tag}.logits": de["logits"][:, 0], f"{tag}.h": de["state"][0], f"{tag}.attw_d": de["weights"],
                         f"{tag}.rnn_input": de["rnn_input"][:, 0]})
        torch.cuda.synchronize()
        return want


@pytest.mark.parametrize("S_", [5, 21], ids=["S5_one_workgroup_attention", "S21_split_attention"])
@pytest.mark.parametrize("E,H,A", INFER, ids=INFER_IDS)
def test_step_api_contract(E, H, A, S_):
    fam, other = StepFam(E, H, A, 3, S_), StepFam(E, H, A, 5, S_ + 12)
    split = _lib.call("acvae_attn_fwd_workspace_bytes", 3, 1, S_, A, E) > 0
    assert split == (S_ == 21)                       # the split form's counters live in the scratch at S = 21 only
    got = contract(fam, other, f"step API E={E} H={H} A={A} S={S_}")
    for k, want in fam.python_path().items():
        close(got[k], want, f"step API E={E} H={H} A={A} S={S_} {k}")


# ================================================================================================ searches
N_S, BEAM, T_S, S_S = 2, 3, 6, 21


class FinishOut:
    """The n-best outputs and trailing arguments of an acvae_*_finishing entry, prefilled."""

    def __init__(self, O, tag, N, T, nbest):
        O.update({f"{tag}.nbest_seqs": ints(N, nbest, T), f"{tag}.nbest_scores": nans(N, nbest),
                  f"{tag}.nbest_logprobs": nans(N, nbest), f"{tag}.nbest_lengths": ints(N, nbest, dtype=torch.int32)})
        self.norm = length_norm(T, FINISH[0])         # a HOST table the entry reads before it returns
        self.args = (self.norm.ctypes.data_as(ctypes.c_void_p), nbest, O[f"{tag}.nbest_seqs"], O[f"{tag}.nbest_scores"],
                     O[f"{tag}.nbest_logprobs"], O[f"{tag}.nbest_lengths"])


class BeamFam(Family):
    """acvae_beam_search, _constrained and _finishing of one model, each on the scratch of its own *_scratch_bytes."""

    def __init__(self, E, H, A, N, beam, T, S_):
        self.E, self.H, self.A, self.N, self.beam, self.T, self.S_ = E, H, A, N, beam, T, S_
        self.model = text_model(E, H, A)
        g = torch.Generator().manual_seed(19 * N + S_ + H)
        self.audio = torch.randn(N, S_, self.model.ln.weight.shape[1], generator=g).cuda()
        self.lens = torch.tensor([max(1, S_ - 9 * n) for n in range(N)]).cuda()
        self.encoded = {"audio_embeds": self.audio, "audio_embeds_lens": self.lens.cpu()}
        with torch.no_grad():
            self.mem = self.model._projected_memory(self.encoded)
        self.eps = torch.randn(T, N, beam, E, generator=g).cuda()                   # step-major, as the library reads it
        self.dims = (N, beam, T, S_, E, H, A, V)
        self.con_args = _constraint_args(CONSTRAIN)
        self._keep = self.con_args[3]

    def sizes(self):
        return {"plain": _lib.call("acvae_beam_search_scratch_bytes", *self.dims),
                "constrained": _lib.call("acvae_beam_search_constrained_scratch_bytes", *self.dims),
                "finishing": _lib.call("acvae_beam_search_finishing_scratch_bytes", *self.dims)}

    def fresh(self):
        self.params = self.model._text_table()
        self.O = {}
        for tag in ("plain", "constrained", "finishing"):
            self.O[f"{tag}.seqs"], self.O[f"{tag}.attw"] = ints(self.N, self.T), nans(self.N, self.S_, self.T)
        self.fin = FinishOut(self.O, "finishing", self.N, self.T, FINISH[1])

    def steps(self):
        O, m = self.O, self.model

        def head(tag, ws, nb):
            return (self.params, self.mem, self.lens, self.eps, int(m.start_idx), O[f"{tag}.seqs"], O[f"{tag}.attw"], ptr(ws[tag]),
                    nb[tag], *self.dims, S())

        def plain(ws, nb):
            _lib.call("acvae_beam_search", *head("plain", ws, nb))

        def constrained(ws, nb):
            _lib.call("acvae_beam_search_constrained", *head("constrained", ws, nb), int(m.end_idx), *self.con_args)

        def finishing(ws, nb):
            _lib.call("acvae_beam_search_finishing", *head("finishing", ws, nb), int(m.end_idx), *self.con_args, *self.fin.args)

        return [("acvae_beam_search", ("plain",), plain), ("acvae_beam_search_constrained", ("constrained",), constrained),
                ("acvae_beam_search_finishing", ("finishing",), finishing)]

    def python_path(self):
        m, want = self.model, {}
        replay = self.eps.transpose(0, 1).contiguous().cpu()                       # [N, T, beam, E]
        con = dict(repetition_penalty=CONSTRAIN[0], no_repeat_ngram_size=CONSTRAIN[1], min_length=CONSTRAIN[2],
                   suppress_tokens=list(CONSTRAIN[3]))
        for tag, kw in (("plain", {}), ("constrained", con),
                        ("finishing", dict(con, finish_on_end=True, length_penalty=FINISH[0], nbest=FINISH[1]))):
            m.noise = dict(eps_beam=replay)
            out = m.beam_search(dict(self.encoded), self.T, self.beam, **kw)
            want[f"{tag}.seqs"], want[f"{tag}.attw"] = out["seqs"], out["attn_weights"]
            if tag == "finishing":
                want.update({f"{tag}.{k}": out[k] for k in ("nbest_seqs", "nbest_scores", "nbest_logprobs", "nbest_lengths")})
        torch.cuda.synchronize()
        return want


@pytest.mark.parametrize("E,H,A", INFER, ids=INFER_IDS)
def test_beam_search_contract(E, H, A):
    fam, other = BeamFam(E, H, A, N_S, BEAM, T_S, S_S), BeamFam(E, H, A, 3, 2, 8, S_S + 8)
    sz = fam.sizes()
    assert sz["plain"] < sz["constrained"] < sz["finishing"]        # the histories and the records need their own room
    got = contract(fam, other, f"beam search E={E} H={H} A={A}")
    for k, want in fam.python_path().items():
        close(got[k], want, f"beam search E={E} H={H} A={A} {k}")


ENS_T_FEAT = 336                                     # Cnn10: S = 21 memory frames


class EnsembleFam(Family):
    """acvae_ensemble_search (beam and greedy), _constrained and _finishing over two members of unequal widths."""

    def __init__(self, N, beam, T, t_feat):
        self.N, self.beam, self.T = N, beam, T
        self.models = [text_model(*w) for w in W.ENSEMBLE_MEMBERS]
        g = torch.Generator().manual_seed(23 * N + t_feat)
        self.feats = torch.randn(N, t_feat, 64, generator=g).cuda()
        self.feat_lens = np.array([max(16, t_feat - 136 * n) for n in range(N)])
        self.mems, self.lens, self.eps, self.eps1, dims = [], [], [], [], []
        with torch.no_grad():
            for m in self.models:
                enc = m.encoder(self.feats, self.feat_lens.copy())
                mem = m._projected_memory(enc)
                self.mems.append(mem)
                self.lens.append(torch.as_tensor(enc["audio_embeds_lens"]).to(device="cuda", dtype=torch.long).contiguous())
                E = mem.shape[2]
                self.eps.append(torch.randn(T, N, beam, E, generator=g).cuda())
                self.eps1.append(torch.randn(T, N, 1, E, generator=g).cuda())
                dims.append((mem.shape[1], E, m.decoder.model.hidden_size, m.decoder.attn.attn_size))
        assert dims[0] != dims[1]
        self.host = [np.ascontiguousarray([d[j] for d in dims], dtype=np.int32) for j in range(4)]
        self.host_ptrs = [a.ctypes.data for a in self.host]
        self.con_args = _constraint_args(CONSTRAIN)
        self.idx = (int(self.models[0].start_idx), int(self.models[0].end_idx))

    def sizes(self):
        a = (2, self.N, self.beam, self.T, *self.host_ptrs, V)
        return {"beam": _lib.call("acvae_ensemble_search_scratch_bytes", *a),
                "greedy": _lib.call("acvae_ensemble_search_scratch_bytes", 2, self.N, 1, self.T, *self.host_ptrs, V),
                "constrained": _lib.call("acvae_ensemble_search_constrained_scratch_bytes", *a),
                "finishing": _lib.call("acvae_ensemble_search_finishing_scratch_bytes", *a)}

    def fresh(self):
        self.tables = [_lib.ptr_table(m._text_table()) for m in self.models]
        self.params = (ctypes.c_void_p * 2)(*[ctypes.cast(t, ctypes.c_void_p).value for t in self.tables])
        self.O = {}
        for tag in ("beam", "constrained", "finishing"):
            self.O[f"{tag}.seqs"], self.O[f"{tag}.logprobs"] = ints(self.N, self.T), nans(self.N)
        self.O["greedy.seqs"], self.O["greedy.logprobs"] = ints(self.N, self.T), nans(self.N, self.T)
        self.fin = FinishOut(self.O, "finishing", self.N, self.T, FINISH[1])

    def steps(self):
        O = self.O

        def head(tag, ws, nb, greedy=0):
            beam = 1 if greedy else self.beam
            return (self.params, self.mems, self.lens, self.eps1 if greedy else self.eps, *self.host_ptrs, 2, *self.idx, greedy,
                    O[f"{tag}.seqs"], O[f"{tag}.logprobs"], ptr(ws[tag]), nb[tag], self.N, beam, self.T, V, S())

        def beam(ws, nb):
            _lib.call("acvae_ensemble_search", *head("beam", ws, nb))

        def greedy(ws, nb):
            _lib.call("acvae_ensemble_search", *head("greedy", ws, nb, 1))

        def constrained(ws, nb):
            _lib.call("acvae_ensemble_search_constrained", *head("constrained", ws, nb), *self.con_args)

        def finishing(ws, nb):
            _lib.call("acvae_ensemble_search_finishing", *head("finishing", ws, nb), *self.con_args, *self.fin.args)

        return [("acvae_ensemble_search", ("beam",), beam), ("acvae_ensemble_search", ("greedy",), greedy),
                ("acvae_ensemble_search_constrained", ("constrained",), constrained),
                ("acvae_ensemble_search_finishing", ("finishing",), finishing)]

    def python_path(self):
        ens, want = Ensemble(self.models), {}
        con = dict(repetition_penalty=CONSTRAIN[0], no_repeat_ngram_size=CONSTRAIN[1], min_length=CONSTRAIN[2],
                   suppress_tokens=list(CONSTRAIN[3]))
        for tag, kw in (("beam", dict(method="beam")), ("greedy", dict(method="greedy")), ("constrained", dict(con, method="beam")),
                        ("finishing", dict(con, method="beam", finish_on_end=True, length_penalty=FINISH[0], nbest=FINISH[1]))):
            eps = self.eps1 if tag == "greedy" else self.eps
            ens.noise = {"eps": [e.transpose(0, 1).contiguous().cpu() for e in eps]}
            out = ens(self.feats, self.feat_lens.copy(), beam_size=self.beam, max_length=self.T, **kw)
            want[f"{tag}.seqs"], want[f"{tag}.logprobs"] = out["seqs"], out["logprobs"]
            if tag == "finishing":
                want.update({f"{tag}.{k}": out[k] for k in ("nbest_seqs", "nbest_scores", "nbest_logprobs", "nbest_lengths")})
        torch.cuda.synchronize()
        return want


def test_ensemble_search_contract():
    fam, other = EnsembleFam(N_S, BEAM, T_S, ENS_T_FEAT), EnsembleFam(3, 2, 8, ENS_T_FEAT + 128)
    sz = fam.sizes()
    assert sz["greedy"] < sz["beam"] < sz["constrained"] < sz["finishing"]
    got = contract(fam, other, "ensemble search, two members")
    for k, want in fam.python_path().items():
        close(got[k], want, f"ensemble search {k}")
