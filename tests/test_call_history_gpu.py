"""State that outlives a call: one model object, many calls.

A call on a model with a past must give, bit for bit, what the same call gives on a model without one.  The ``veteran`` is
one ``Hybrid_VAEModel`` under a ``TrainStep`` that lives through a whole history of calls at changing batch sizes, frame
counts and caption lengths (grown and then shrunk, so that every grow-only scratch is reused at a smaller shape); before each
compared call ``fresh()`` builds a new model under a new ``TrainStep`` with the veteran's ``state_dict()`` (parameters and
buffers), so both sides hold their parameters in 16-byte-aligned views of a flat buffer and pick kernels alike.  Both sides
are seeded alike (``torch.manual_seed`` / ``random.seed``) and the encoder's dropout is off (``p_block = p_fc = 0``: its
device-drawn masks are numbered by a per-model call counter, which is history by design).  Compared with ``torch.equal``:
every tensor of the output dict, every parameter gradient after ``backward()``, every BatchNorm buffer after a training
forward.  The fresh route is what the oracle and golden tests validate; one step is anchored to the oracle here as well, so
the pair cannot agree on a common error.

The second half holds the step API (``model.decoder(word=..)`` / ``model.pnet(..)``) with ONE held encoder memory to account
across changes of the attention weights: the hoisted projection it caches per memory tensor must not outlive them."""
import random

import numpy as np
import pytest
import torch

import acvae_oracle as O
from acvae_amd import _lib
from acvae_amd.trainer import TrainStep
from parity_util import close
from test_model_gpu import build_model, hip_loss

pytestmark = pytest.mark.gpu

V = 40
HISTORIES = {"cnn10": dict(E=64, proj=0), "projemb": dict(E=64, proj=24), "no_ln": dict(E=512, proj=0)}


def initial_state(E, proj, scale=1.0):
    st = O.closed_form_state(O.state_shapes(V, E, E, None, E, 512, proj_embed=proj or None))
    if scale != 1.0:       # another set of text-side weights (the encoder and its BatchNorm statistics stay)
        st = {k: (v * scale if v.is_floating_point() and not k.startswith("encoder.") else v) for k, v in st.items()}
    return st


def under_train_step(E, proj, state):
    m = build_model(V, E, {k: v.detach().cpu() for k, v in state.items()}, proj_embed=proj)
    m.encoder.p_block = m.encoder.p_fc = 0.0
    return m, TrainStep(m, V)


class History:
    def __init__(self, name):
        cfg = HISTORIES[name]
        self.name, self.E, self.proj = name, cfg["E"], cfg["proj"]
        self.veteran, self.ts = under_train_step(self.E, self.proj, initial_state(self.E, self.proj))
        assert hasattr(self.veteran, "ln") == (self.E != 512)
        self.done = 0
        self.held = None                 # an encoder output obtained before the optimiser steps and held across them

    def fresh(self):
        m, _ts = under_train_step(self.E, self.proj, self.veteran.state_dict())
        m.train(self.veteran.training)
        m._keep_ts = _ts                 # (the flat buffers live as long as the model)
        return m


_histories = {}


def history(name, upto):
    """The history ``name`` advanced to just before step ``upto``: earlier steps that have not run yet (a test selected on
    its own) run as history only."""
    h = _histories.get(name)
    if h is None:
        h = _histories[name] = History(name)
    assert h.done <= upto, "the steps of a history run in file order"
    while h.done < upto:
        STEPS[h.done](h, compare=False)
        h.done += 1
    h.done = upto + 1
    return h


# ------------------------------------------------------------------------------------------------ calls and comparisons
def batch(B, T, L, seed, ragged=True):
    feats, caps, fl, cl = O.synthetic_batch(B, T, V, L, seed=seed, ragged=ragged)
    return feats.cuda(), caps, fl, cl


def tensors_of(out, prefix=""):
    got = {}
    for k, v in out.items():
        if isinstance(v, torch.Tensor):
            got[prefix + k] = v
        elif isinstance(v, (tuple, list)):
            got.update(tensors_of({f"{k}[{i}]": x for i, x in enumerate(v)}, prefix))
        elif isinstance(v, dict):
            got.update(tensors_of(v, prefix + k + "."))
    return got


def same(a, b, what):
    assert a.keys() == b.keys(), (what, sorted(a.keys() ^ b.keys()))
    assert a, what
    for k in a:
        x, y = a[k], b[k]
        assert x.dtype == y.dtype and x.shape == y.shape, (what, k, x.dtype, y.dtype, x.shape, y.shape)
        if x.is_floating_point():
            assert not bool(torch.isnan(x).any()), (what, k, "NaN")
        assert torch.equal(x, y), f"{what}: {k} differs between the reused model and a fresh one " \
                                  f"({int((x != y).sum())}/{x.numel()} elements)"


def train_call(m, b, seed, noise=None, **kw):
    """Training forward + loss + backward -> (outputs, gradients, BatchNorm buffers)."""
    feats_d, caps, fl, cl = b
    m.train()
    for p in m.parameters():
        p.grad = None
    if noise is not None:
        m.noise = dict(noise)
    torch.manual_seed(seed); random.seed(seed)
    out = m(feats_d, fl.copy(), caps, cl, **dict(dict(ss_ratio=1.0, dis_ratio=0), **kw))
    hip_loss(out, caps, cl, V)[0].backward()
    torch.cuda.synchronize()
    grads = {n: p.grad for n, p in m.named_parameters() if p.grad is not None}
    assert len(grads) > 30
    bufs = {n: t for n, t in m.named_buffers()}
    return tensors_of(out), grads, bufs


def compare_train(h, compare, b, seed, what, **kw):
    fresh = h.fresh() if compare else None          # (before the veteran's call: a training forward moves its BatchNorm buffers)
    got = train_call(h.veteran, b, seed, **kw)
    if compare:
        got = tuple({k: v.detach().clone() for k, v in part.items()} for part in got)
        want = train_call(fresh, b, seed, **kw)
        for a, w, part in zip(got, want, ("outputs", "gradients", "buffers")):
            same(a, w, f"{h.name} {what} {part}")


def infer_call(m, fn, seed):
    m.eval()
    torch.manual_seed(seed); random.seed(seed)
    with torch.no_grad():
        out = fn(m)
    torch.cuda.synchronize()
    return tensors_of(out)


def compare_infer(h, compare, fn, seed, what):
    fresh = h.fresh() if compare else None
    got = infer_call(h.veteran, fn, seed)
    if compare:
        got = {k: v.clone() for k, v in got.items()}
        same(got, infer_call(fresh, fn, seed), f"{h.name} {what}")
    h.veteran.train()


B1 = (3, 96, 7, 11)                      # step 1's batch (B, T, L, seed), called again at the end of step 7


def step_train_ragged(h, compare):
    compare_train(h, compare, batch(*B1), 21, "training step, ragged")


def step_greedy_larger(h, compare):
    f, _, fl, _ = batch(5, 250, 9, 12)
    compare_infer(h, compare, lambda m: m(f, fl.copy(), method="greedy", max_length=9), 22, "greedy at a larger B and T")
    h.veteran.eval()
    with torch.no_grad():                # held across the optimiser steps that follow (step 5 searches over it)
        f2, _, fl2, _ = batch(2, 130, 5, 13)
        h.held = h.veteran.encoder(f2, fl2.copy())
    h.veteran.train()


def step_two_optimizer_steps(h, compare):
    """History only: two fused updates (raw-pointer writes into the flat parameter buffer)."""
    for i in range(2):
        f, caps, fl, cl = batch(4, 64, 9, 14 + i)
        torch.manual_seed(23 + i); random.seed(23 + i)
        h.veteran.train()
        h.ts.step(f, fl.copy(), caps, cl, 1.0, 0, 0.5)
    torch.cuda.synchronize()


def step_train_batch_of_one(h, compare):
    compare_train(h, compare, batch(1, 90, 5, 16, ragged=False), 25, "training step at B = 1")


def step_beam(h, compare):
    f, _, fl, _ = batch(2, 130, 5, 13)
    compare_infer(h, compare, lambda m: m(f, fl.copy(), method="beam", beam_size=3, max_length=8), 26, "beam search")
    held = h.held
    compare_infer(h, compare, lambda m: m.beam_search(dict(held), 8, 3), 27,
                  "beam_search over an encoder output held across two optimiser steps")


def step_sampled_dbs_rollout(h, compare):
    f, _, fl, _ = batch(4, 200, 5, 17)
    compare_infer(h, compare, lambda m: m(f, fl.copy(), method="sample", temp=0.9, top_k=7, top_p=0.9, max_length=7), 28,
                  "sampled decoding with top_k / top_p")
    compare_infer(h, compare, lambda m: m(f[:3], fl[:3].copy(), method="dbs", beam_size=4, group_size=2, max_length=6,
                                          dbs_impl="device"), 29, "diverse beam search on the device")
    compare_infer(h, compare, lambda m: m.rollout_shared_encoder(f[:2], fl[:2].copy(), 3, method="sample", max_length=6), 30,
                  "rollout_shared_encoder(sample_n=3)")


def step_ss_dis_modes_and_step1_again(h, compare):
    compare_train(h, compare, batch(3, 160, 8, 18), 31, "scheduled-sampling step", ss_ratio=0.6)
    compare_train(h, compare, batch(2, 64, 6, 19), 32, "dis_ratio step", dis_ratio=0.5)
    h.veteran.eval()
    h.veteran.train()
    compare_train(h, compare, batch(*B1), 21, "step 1's call again")


def step_refused_call_keeps_replay(h, compare):
    """``model.noise`` set, then a call that is refused for its arguments before anything is drawn (a ``clip_index`` that
    names one clip three times): the replay stays pending (``Hybrid_VAEModel.noise``), the next valid call consumes it, the
    one after that draws afresh."""
    b = batch(3, 64, 6, 20)
    g = torch.Generator().manual_seed(5)
    noise = dict(eps_q=torch.randn(3, 5, h.E, generator=g), eps_p=torch.randn(5, 3, h.E, generator=g))
    h.veteran.noise = dict(noise)
    h.veteran.train()
    with pytest.raises(ValueError):
        h.veteran(b[0], b[2].copy(), b[1], b[3], ss_ratio=1.0, dis_ratio=0, clip_index=[0, 0, 0])
    assert h.veteran.noise is not None and torch.equal(h.veteran.noise["eps_q"], noise["eps_q"])
    fresh, fresh2 = (h.fresh(), h.fresh()) if compare else (None, None)
    got = train_call(h.veteran, b, 33)                      # the pending replay is consumed here ...
    assert h.veteran.noise is None
    if compare:
        got = tuple({k: v.detach().clone() for k, v in part.items()} for part in got)
        want = train_call(fresh, b, 33, noise=noise)        # ... and equals a fresh model given that replay
        for a, w, part in zip(got, want, ("outputs", "gradients", "buffers")):
            same(a, w, f"{h.name} call after a refused one {part}")
        undrawn = train_call(fresh2, b, 33)
        assert not torch.equal(undrawn[0]["p_z"], want[0]["p_z"])       # (the replay mattered)
    compare_train(h, compare, b, 34, "second call after a refused one: draws its own noise")


STEPS = [step_train_ragged, step_greedy_larger, step_two_optimizer_steps, step_train_batch_of_one, step_beam,
         step_sampled_dbs_rollout, step_ss_dis_modes_and_step1_again, step_refused_call_keeps_replay]
NAMES = sorted(HISTORIES)


@pytest.mark.parametrize("name", NAMES)
def test_step1_training_forward_and_backward_ragged(name):
    STEPS[0](history(name, 0), True)


@pytest.mark.parametrize("name", NAMES)
def test_step2_greedy_inference_at_a_larger_batch_and_length(name):
    STEPS[1](history(name, 1), True)


@pytest.mark.parametrize("name", NAMES)
def test_step3_two_optimizer_steps_as_history(name):
    STEPS[2](history(name, 2), True)
    assert _histories[name].ts.step_count == 2


@pytest.mark.parametrize("name", NAMES)
def test_step4_training_forward_and_backward_at_batch_of_one(name):
    STEPS[3](history(name, 3), True)


@pytest.mark.parametrize("name", NAMES)
def test_step5_beam_search_and_a_held_encoder_output(name):
    STEPS[4](history(name, 4), True)


@pytest.mark.parametrize("name", NAMES)
def test_step6_sampled_decoding_dbs_and_shared_encoder_rollout(name):
    STEPS[5](history(name, 5), True)


@pytest.mark.parametrize("name", NAMES)
def test_step7_scheduled_sampling_dis_ratio_mode_flip_then_step1_again(name):
    STEPS[6](history(name, 6), True)


@pytest.mark.parametrize("name", NAMES)
def test_step8_a_refused_call_leaves_the_replay_pending(name):
    STEPS[7](history(name, 7), True)


def test_step9_the_veterans_last_training_forward_against_the_oracle():
    """The oracle anchor: after the whole history, the veteran's training forward under recorded noise against the oracle's
    own step on the veteran's weights (loss terms <= 1e-4 relative, ``seqs`` exact, as tests/test_model_gpu.py), and bit for
    bit against a fresh model."""
    h = history("cnn10", len(STEPS))
    feats, caps, fl, cl = O.synthetic_batch(3, 96, V, 7, seed=11, ragged=True)
    ostate = {k: v.detach().cpu().clone() for k, v in h.veteran.state_dict().items()}
    rec = {}
    torch.manual_seed(41); random.seed(41)
    ores = O.OracleTrainer(ostate, V).step(feats, fl.copy(), caps, cl, 1.0, 0, record=rec, apply_update=False)
    results = []
    for m in (h.veteran, h.fresh()):
        m.train()
        m.encoder.p_block, m.encoder.p_fc = 0.2, 0.5         # the oracle's masks are replayed, at the reference's rates
        m.encoder.dropout_masks = rec["dropout"]
        got = train_call(m, (feats.cuda(), caps, fl, cl), 41, noise=dict(eps_q=rec["eps_q"], eps_p=rec["eps_p"]))
        m.encoder.dropout_masks = None
        m.encoder.p_block = m.encoder.p_fc = 0.0
        results.append(tuple({k: v.detach().clone() for k, v in part.items()} for part in got))
    for a, w, part in zip(results[0], results[1], ("outputs", "gradients", "buffers")):
        same(a, w, f"oracle-anchored step {part}")
    out = {k: v for k, v in results[0][0].items()}
    out["p_logs_utt"] = None
    _, ce, kl, mse = hip_loss(out, caps, cl, V)
    loss = ce + 0.5 * kl + mse
    for k, v in (("loss", loss), ("ce", ce), ("kl", kl), ("mse", mse)):
        ref = float(ores[k])
        print(k, float(v), ref)
        assert abs(float(v) - ref) <= 1e-4 * max(1.0, abs(ref)), (k, float(v), ref)
    assert np.array_equal(out["seqs"].cpu().numpy(), ores["out"]["seqs"].numpy())


# ------------------------------------------------------------------------------------------------ the step API and its cache
N_, S_ = 5, 9


class StepCase:
    """A model under a TrainStep, ONE held encoder memory and one step's inputs."""

    def __init__(self, E=64, proj=0):
        self.E, self.proj = E, proj
        self.model, self.ts = under_train_step(E, proj, initial_state(E, proj))
        self.model.eval()
        g = torch.Generator().manual_seed(2)
        self.mem = torch.randn(N_, S_, E, generator=g)
        self.mem_d = self.mem.cuda()
        self.lens = torch.tensor([9, 7, 4, 2, 1])
        self.word = torch.randint(0, V, (N_, 1), generator=g)
        self.h, self.hp, self.cp = (torch.randn(1, N_, E, generator=g) for _ in range(3))
        self.lz, self.eps = torch.randn(N_, E, generator=g), torch.randn(N_, E, generator=g)

    def call(self, m, mem_d=None):
        mem_d = self.mem_d if mem_d is None else mem_d
        with torch.no_grad():
            p = m.pnet(self.word, mem_d, (self.hp.cuda(), self.cp.cuda()), self.lz.cuda(), self.lens, eps=self.eps)
            d = m.decoder(word=self.word, state=self.h.cuda(), enc_mem=mem_d, enc_mem_lens=self.lens, z=p["z"])
        torch.cuda.synchronize()
        return {k: v.clone() for k, v in {**tensors_of(p, "prior."), **tensors_of(d, "decoder.")}.items()}

    def fresh(self):
        m, ts = under_train_step(self.E, self.proj, self.model.state_dict())
        m._keep_ts = ts
        return m.eval()

    def check_against_fresh(self, what):
        got = self.call(self.model)
        same(got, self.call(self.fresh()), what)
        return got


def test_step_api_after_load_state_dict_uses_the_new_attention_weights():
    c = StepCase()
    before = c.call(c.model)                                # fills the cache for the held memory
    state2 = initial_state(c.E, c.proj, scale=0.8)
    c.model.load_state_dict({k: v.clone() for k, v in state2.items()})
    got = c.check_against_fresh("step API after load_state_dict")
    assert not torch.equal(got["decoder.weights"], before["decoder.weights"])
    with torch.no_grad():                                   # and against the oracle, as test_single_step_modules_vs_oracle
        op = O.prior_step(state2, c.word, c.mem, (c.hp[0], c.cp[0]), c.lz, c.lens, c.eps)
        od = O.decoder_step(state2, c.word, c.h[0], c.mem, c.lens, op["z"])
    close(got["prior.mean"], op["mean"], what="prior mean"); close(got["prior.z"], op["z"], what="prior z")
    close(got["prior.hiddens_state[0]"][0], op["hiddens_state"][0], what="prior h")
    close(got["prior.hiddens_state[1]"][0], op["hiddens_state"][1], what="prior c")
    close(got["decoder.logits"][:, 0], od["logits"], 1e-4, 2e-5, what="dec logits")
    close(got["decoder.state"][0], od["state"], what="dec h")
    close(got["decoder.weights"], od["weights"], what="dec attn")
    close(got["decoder.rnn_input"][:, 0], od["rnn_input"], what="rnn_input")


@pytest.mark.parametrize("which", ["decoder.attn", "pnet.word_attn"])
def test_step_api_after_an_in_place_edit_of_the_attention_weights(which):
    c = StepCase()
    before = c.call(c.model)
    attn = c.model.decoder.attn if which == "decoder.attn" else c.model.pnet.word_attn
    with torch.no_grad():
        attn.h2attn.weight.mul_(1.5)
    got = c.check_against_fresh(f"step API after {which}.h2attn.weight.mul_(1.5)")
    assert any(not torch.equal(got[k], before[k]) for k in got)
    with torch.no_grad():
        attn.h2attn.bias.add_(0.25)
    c.check_against_fresh(f"step API after {which}.h2attn.bias.add_(0.25)")


@pytest.mark.parametrize("proj", [0, 24], ids=["plain", "projemb"])
def test_step_api_after_a_train_step(proj):
    """The fused update writes the parameters through raw pointers: no ``_version`` moves.  (With projected embeddings the
    decoder's table cache is under the same rule.)"""
    c = StepCase(proj=proj)
    before = c.call(c.model)
    f, caps, fl, cl = batch(3, 64, 7, 3)
    c.model.train()
    torch.manual_seed(1); random.seed(1)
    c.ts.step(f, fl.copy(), caps, cl, 1.0, 0, 0.5)
    c.model.eval()
    got = c.check_against_fresh("step API after TrainStep.step")
    assert any(not torch.equal(got[k], before[k]) for k in got)


def test_step_api_and_a_memory_rewritten_behind_torchs_back():
    """The held memory's contents change: an in-place edit torch sees (``_version`` moves) is noticed; a library call that
    writes into it is invisible, and the contract (``Hybrid_VAEModel._encproj``) is that such a caller calls
    ``drop_step_caches()`` - with it the result is a fresh model's, without it the projection is the stale one."""
    c = StepCase()
    c.call(c.model)
    c.mem_d.mul_(0.5)
    same(c.call(c.model), c.call(c.fresh()), "step API after mem_d.mul_(0.5)")
    src = torch.randn(c.E, N_ * S_, generator=torch.Generator().manual_seed(8)).cuda()
    stale = c.model._encproj(0, c.mem_d).clone()
    _lib.call("acvae_transpose", src, N_ * S_, c.mem_d, c.E, c.E, N_ * S_, _lib.current_stream())   # mem_d = src^T, unseen
    torch.cuda.synchronize()
    assert torch.equal(c.mem_d.reshape(N_ * S_, c.E), src.t())
    assert torch.equal(c.model._encproj(0, c.mem_d), stale)                     # the documented limit
    c.model.drop_step_caches()
    same(c.call(c.model), c.call(c.fresh()), "step API after a raw write into mem_d and drop_step_caches()")


def test_the_projection_is_computed_once_per_memory_tensor_in_a_search_loop(monkeypatch):
    c = StepCase()
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    mem2 = (c.mem_d * 2).contiguous()
    for mem_d in (c.mem_d, mem2):
        state, hid, lz, w = c.h.cuda(), (c.hp.cuda(), c.cp.cuda()), c.lz.cuda(), c.word
        for t in range(4):                                   # a beam-search-style loop over an unchanged model
            with torch.no_grad():
                p = c.model.pnet(w, mem_d, hid, lz, c.lens, eps=c.eps)
                d = c.model.decoder(word=w, state=state, enc_mem=mem_d, enc_mem_lens=c.lens, z=p["z"])
            state, hid, lz, w = d["state"], p["hiddens_state"], p["z"], d["logits"][:, 0].argmax(-1, keepdim=True)
    assert calls.count("acvae_attn_precompute") == 4         # two attentions x two memory tensors, not x four steps
    assert calls.count("acvae_decoder_step_fwd") == 8 and calls.count("acvae_prior_step_fwd") == 8
