"""GPU: the text side at UNEQUAL embed (E), decoder-GRU (H), attention (A) and posterior-GRU (Hq) widths.  Every other test,
golden and tool builds the text side with one number for all four, so a stride, offset, loop bound or scratch size written
with the wrong one of them passes the rest of the suite: dec_layout's max(A, E) regions (dencproj, dvpart, attws), the
[A, E + H] h2attn weight split into its state and memory columns and transposed for the backward, the persistent plans'
role counts (n_d1 = A/32 + 3H/32), the A-wide d qd shares of a split attention role, the beam gather of [H] and [E] rows.

Training (H = Hq = E is forced by the utterance head and the MSE; A is free): the sets of widths_util.TRAIN_SETS, each on the
default path and under the _lib.override variants of test_fullsize_grads_gpu.VARIANTS that select another path at that shape,
against one oracle step per set (the oracle draws and records the noise, the HIP model replays it): loss to 1e-4, teacher-forced
words equal, the forward tensors to parity_util.close(1e-4, 2e-5), every parameter gradient to grads_match_oracle's bounds.
The sets meant for the persistent decode launches are asserted to be taken by the plans (widths_util.plans) and to have run
them (their decoder gradients differ bit-wise from the per-step variant's).  One case feeds the prior's z to the decoder
(dis_ratio = 0.5: fixed coins) and one runs under scheduled sampling (ss_ratio = 0.5: the oracle is fed the HIP run's words and
the words are compared decision by decision, parity_util.words_match_by_margin), both at E = 64, A = 160.

Inference and rollouts (H and A free): the step modules, every decoding route against the CPU reference that route has, the
g19 goldens, and the refusal of a training forward with H != E.

Seeds, chosen with the references alone on the CPU so that no decision is within 2e-4 of a tie: see SS_SEED and NOISE_SEEDS."""
import random

import numpy as np
import pytest
import torch

import acvae_oracle as O
import widths_util as W
from acvae_amd import _lib
from conftest import load_golden
from parity_util import close, grads_match_oracle, words_match_by_margin
from test_fullsize_grads_gpu import VARIANTS
from test_model_gpu import hip_loss

pytestmark = pytest.mark.gpu

L = 7
SEED = 3
# scheduled sampling at E = 64, A = 160: with this seed the coins are TfTffT and the oracle alone (CPU) leaves out 0 of its 18
# decisions at a threshold of 2e-4 (smallest margin 7.0e-3); every word fed at a false-coin step differs from the caption's
# (seeds 4 and 5 draw six equal coins and were passed over)
SS_SEED = 3
DIS_FLAGS = [t % 3 == 1 for t in range(L - 1)]

CASES = {name: dict(set=name) for name in W.TRAIN_SETS}
CASES["E64_A160_dis"] = dict(set="E64_A160", dis=0.5, variants=("default",))          # per-step chains, never deferred
CASES["E64_A160_ss"] = dict(set="E64_A160", ss=0.5, variants=("default", "no_persist"))  # per-step forward, persistent BPTT


def _variants(case):
    """The variants that select another launch path at the case's shape.  The split-over-frames attention of the per-step path
    needs S > 16 frames and A % 4 == 0 (attention.hip, attn_split_shape): at S = 4 attn_split=False is the persist=False path.
    Where A is no multiple of 32 the decode goes per step whatever `persist` says, so persist=False is the default path (it
    would only take the posterior, at Hq = E, off its persistent launch, which tests/test_posterior_layers_gpu.py compares)."""
    p = CASES[case]
    if "variants" in p:
        return p["variants"]
    S = W.train_dims(p["set"], L)[5]
    same_path = {"no_persist_no_split"} if S <= 16 else set()
    if p["set"] not in W.TRAIN_PERSISTENT:
        same_path.add("no_persist")
    return [v for v in VARIANTS if v not in same_path]


PARAMS = [(c, v) for c in CASES for v in _variants(c)]
_CACHE = {}
RATIOS = {}


def _ratio(group, a, b, rtol, atol):
    a = torch.as_tensor(a).detach().cpu().double(); b = torch.as_tensor(b).detach().cpu().double()
    r = float(((a - b).abs() / (atol + rtol * b.abs())).max())
    RATIOS[group] = max(RATIOS.get(group, 0.0), r)
    return r


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    _CACHE.clear()
    _dec.clear()
    for k in sorted(RATIOS):
        print(f"\nWIDTHS worst error / tolerance, {k}: {RATIOS[k]:.3f}", end="")


def _patched(flags, run):
    if flags is None:
        return run()
    orig, it = torch.rand, iter(flags)
    torch.rand = lambda *a, **k: torch.tensor([0.0 if next(it) else 2.0])
    try:
        return run()
    finally:
        torch.rand = orig


def _case(name):
    """The oracle's natural step of one case (it draws and records the noise and, under scheduled sampling, the coins), once."""
    c = _CACHE.get(name)
    if c is not None:
        return c
    p = CASES[name]
    B, T, V, E, A, S, Tc = W.train_dims(p["set"], L)
    dis, ss = p.get("dis", 0), p.get("ss", 1.0)
    seed = SS_SEED if ss < 1.0 else SEED
    state = W.make_state(V, E, E, A, E)
    assert state["decoder.attn.h2attn.weight"].shape == (A, 2 * E) and state["decoder.attn.v"].shape == (A,)
    feats, _, fl, _ = O.synthetic_batch(B, T, V, L, seed=seed, ragged=True)
    caps, cl = W.ragged_caps(B, L, V, torch.Generator().manual_seed(seed))
    assert int(cl.max()) == L and int(cl.min()) == 2 and int(fl.max()) == T
    flags = DIS_FLAGS if dis else None
    c = dict(name=name, dims=(B, T, V, E, A, S, Tc), state=state, feats=feats, caps=caps, fl=fl, cl=cl, dis=dis, ss=ss,
             flags=flags, seed=seed, dec={}, under=None, fed=None)
    rec = {}
    ores = _oracle_step(c, None, rec)
    c.update(rec=rec, ores=ores)
    if ss < 1.0:
        coins = rec["ss_flags"]
        false_t = [t for t, f in enumerate(coins) if not f]
        assert False in coins and True in coins and max(false_t) >= 1, coins
        differ = float((rec["fed_words"][:, false_t] != caps[:, false_t].long()).double().mean())
        left = float((rec["margins"] <= 2e-4).double().mean())
        print(f"{name}: coins {''.join('T' if f else 'f' for f in coins)}; {differ:.0%} of the words fed at false-coin steps differ "
              f"from the caption word; the oracle alone leaves out {left:.1%} of its decisions at 2e-4 "
              f"(smallest margin {float(rec['margins'].min()):.2e})")
        assert differ >= 1 / 3 and left <= 0.10, (differ, left)
    _CACHE[name] = c
    return c


def _oracle_step(c, noise, record):
    st = {k: v.clone() for k, v in c["state"].items()}
    torch.manual_seed(c["seed"]); random.seed(c["seed"])
    return _patched(c["flags"], lambda: O.OracleTrainer(st, c["dims"][2]).step(
        c["feats"], c["fl"].copy(), c["caps"], c["cl"], c["ss"], c["dis"], noise=noise, record=record, apply_update=False))


def _oracle_under(c, force, fed=None):
    rec = c["rec"]
    noise = dict(dropout=[m.clone() for m in rec["dropout"]], eps_q=rec["eps_q"], eps_p=rec["eps_p"], relu_force=force,
                 fed_words=fed)
    r2 = {}
    res = _oracle_step(c, noise, r2)
    return dict(grads=res["grads"], loss=float(res["loss"]), out=res["out"], margins=r2["margins"])


def _hip(c, variant):
    B, T, V, E, A, S, Tc = c["dims"]
    model = W.build_model(V, E, E, A, E, c["state"]).train()
    rec = c["rec"]
    model.encoder.dropout_masks = rec["dropout"]
    model.encoder.keep_saved = True
    model.noise = dict(eps_q=rec["eps_q"], eps_p=rec["eps_p"])
    tags = []
    model._grad_ready_cb = lambda tag, *a: tags.append(tag)
    with _lib.override(**VARIANTS[variant]):
        torch.manual_seed(c["seed"]); random.seed(c["seed"])
        out = _patched(c["flags"], lambda: model(c["feats"].cuda(), c["fl"].copy(), c["caps"], c["cl"], ss_ratio=c["ss"],
                                                 dis_ratio=c["dis"]))
        loss = hip_loss(out, c["caps"], c["cl"], V)[0]
        loss.backward()
    torch.cuda.synchronize()
    model.check_persistent_launches()
    c["dec"][variant] = {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters()
                         if k.startswith("decoder.") and p.grad is not None}
    return model, out, float(loss.detach()), [t for t in tags if t.startswith("decode")]


FORWARD_KEYS = ("logits", "outputs", "attn_weights", "p_means", "p_logs", "p_z", "q_means", "q_means_utt", "p_means_utt",
                "sampled_logprobs")


@pytest.mark.parametrize("case,variant", PARAMS, ids=[f"{c}-{v}" for c, v in PARAMS])
def test_training_step_vs_oracle_at_unequal_widths(case, variant):
    c = _case(case)
    B, T, V, E, A, S, Tc = c["dims"]
    persistent = CASES[case]["set"] in W.TRAIN_PERSISTENT
    if persistent:             # the shape is taken by the plans: the case cannot go per step for its shape
        p = W.plans(B, Tc, S, E, E, A, E)
        assert p["fwd_ok"] and p["bwd_ok"] and p["post_ok"], p
    model, out, loss, tags = _hip(c, variant)
    named = dict(model.named_parameters())
    assert named["decoder.attn.h2attn.weight"].shape == (A, 2 * E)
    assert out["attn_weights"].shape == (B, S, Tc), out["attn_weights"].shape       # the memory really has S frames (66 at T = 1056)
    if c["ss"] < 1.0:          # against the oracle fed this run's words under this run's ReLU decisions
        seqs = out["seqs"].cpu()
        if c["fed"] is None or not torch.equal(seqs, c["fed"][0]):
            force = {i: m.cpu() for i, m in enumerate(model.encoder.relu_masks())}
            c["fed"] = (seqs, _oracle_under(c, force, seqs))
        ref = c["fed"][1]
        words_match_by_margin(f"{case}-{variant}", seqs, out["logits"], ref["out"], ref["margins"])
        want, oout = ref["loss"], ref["out"]
    else:
        want, oout = float(c["ores"]["loss"]), c["ores"]["out"]
        assert np.array_equal(out["seqs"].cpu().numpy(), oout["seqs"].numpy())
    print(f"{case}-{variant}: loss hip {loss:.6f} oracle {want:.6f}")
    RATIOS["loss (1e-4)"] = max(RATIOS.get("loss (1e-4)", 0.0), abs(loss - want) / (1e-4 * max(1.0, abs(want))))
    assert abs(loss - want) <= 1e-4 * max(1.0, abs(want)), (loss, want)
    for k in FORWARD_KEYS:
        r = _ratio("forward tensors (1e-4, 2e-5)", out[k], oout[k], 1e-4, 2e-5)
        print(f"  {k:18s} {r:.3f} x tolerance")
        close(out[k], oout[k], 1e-4, 2e-5, what=k)
    if c["ss"] < 1.0:
        grads_match_oracle(model, named, ref["grads"], c["rec"], lambda force: ref["grads"])
        got = ref["grads"]
    else:
        def under(force):
            if c["under"] is None:
                c["under"] = _oracle_under(c, force)["grads"]
            return c["under"]
        got = grads_match_oracle(model, named, c["ores"]["grads"], c["rec"], under)
    for k, b in got.items():                                  # (the ratios for DESIGN.md; grads_match_oracle has asserted them)
        if not k.startswith("encoder."):
            b = b.double()
            lim = 2e-4 * max(float(b.abs().max()), 1e-3) + 2e-3 * b.abs()
            g = "attention gradients" if ".attn." in k or "word_attn" in k else "other text-side gradients"
            RATIOS[g] = max(RATIOS.get(g, 0.0), float(((named[k].grad.detach().cpu().double() - b).abs() / lim).max()))
    # the intended path ran
    deferred = not c["dis"] and variant != "no_defer"
    assert tags == ["decode_deferred" if deferred else "decode"], tags
    if variant == "no_persist" and persistent and not c["dis"]:
        if "default" not in c["dec"]:
            _hip(c, "default")
        a, b = c["dec"]["default"], c["dec"][variant]
        assert any(not torch.equal(a[k], b[k]) for k in a), "the persistent decode launch did not run in the default variant"


# ================================================================================================ inference and rollouts
# H and A free.  LP_TOL: the |log_softmax(logits)| error of one step call against the oracle, asserted at these widths by
# test_step_modules_vs_oracle_at_unequal_widths below (measured: 3e-7); token comparisons leave out a clip that holds a decision
# whose reference margin is under MARGIN = 20 x LP_TOL, and at most 10 % of a case's clips, rounded down, may be left out.
import beam_finish_util as BF  # noqa: E402
from test_constrained_decoding_gpu import SEARCH, SML, SV, host_loop, search_noise  # noqa: E402
from test_finishing_beam_gpu import finishing_loop  # noqa: E402
from test_model_gpu import DBS_CASES  # noqa: E402

LP_TOL = 1e-5
MARGIN = 20 * LP_TOL
VD, BD, TD = SV, 4, 96                    # vocabulary (that of the host search loops), clips and feature frames of the decodes
# Seeds.  The features of every decode come from DECODE_SEED; the noise of a case (the prior's eps, the sampling noise) from
# NOISE_SEEDS[(E, H, A)][route], chosen with the references alone on the CPU so that EVERY clip's smallest decision margin
# clears MARGIN (the closed-form weights give flat word distributions: under one fixed seed up to 2.4 % of a case's decisions,
# in up to two of its four clips, were under it).  Searched from 700 upwards for the first seed whose smallest margin is at
# least 2 x MARGIN; diverse beam search at (64, 32, 96) has none such below 900 and takes the best found, 837.  Smallest margin
# of each case, in the order of ROUTES:
#   (64, 96, 160)  4.6e-4  7.2e-3  3.7e-2  5.3e-4  5.5e-4        (64, 32, 96)  4.8e-4  1.3e-2  1.8e-2  4.8e-4  3.1e-4
#   (128, 64, 64)  1.2e-3  1.2e-3  2.9e-2  6.3e-4  4.2e-4        (64, 40, 50)  6.4e-4  3.0e-2  5.8e-3  4.8e-4  4.1e-4
DECODE_SEED = 7
NOISE_SEEDS = {(64, 96, 160): dict(greedy=701, sample=700, gumbel=700, beam=701, dbs=711),
               (64, 32, 96): dict(greedy=700, sample=700, gumbel=700, beam=701, dbs=837),
               (128, 64, 64): dict(greedy=701, sample=700, gumbel=700, beam=701, dbs=710),
               (64, 40, 50): dict(greedy=701, sample=700, gumbel=700, beam=702, dbs=751)}
WIDTH_IDS = [f"E{e}_H{h}_A{a}" for e, h, a in W.INFER_SETS]
_dec = {}


def _decode_case(E, H, A, end_bump=0.0):
    key = (E, H, A, end_bump)
    if key not in _dec:
        state = W.make_state(VD, E, H, A, E)
        assert state["decoder.model.weight_ih_l0"].shape == (3 * H, 3 * E) and state["decoder.classifier.weight"].shape == (VD, H)
        if end_bump:
            state["decoder.classifier.bias"] = state["decoder.classifier.bias"].clone()
            state["decoder.classifier.bias"][O.END_IDX] += end_bump
        feats, _, fl, _ = O.synthetic_batch(BD, TD, VD, 7, seed=DECODE_SEED, ragged=True)
        _dec[key] = dict(state=state, feats=feats, fl=fl, model=None)
    return _dec[key]


def _model_of(c, E, H, A):
    if c["model"] is None:
        c["model"] = W.build_model(VD, E, H, A, E, c["state"]).eval()
    return c["model"]


def _compared_rows(tag, margins):
    """The clips whose words are compared: those whose every reference decision clears MARGIN.  A clip with one decision under
    it is left out whole (one other word changes the rest of the clip, and a search's answer is read off its last step), so
    the bound is on CLIPS, as test_fullsize_decode_gpu.guarded has it: at most 10 % of them, rounded down - none of four.  What
    is left out of the comparison is therefore never more than 10 % of the decisions, and never everything."""
    mins = np.array([float(np.min(np.asarray(m, dtype=np.float64))) if len(m) else np.inf for m in margins])
    keep = [i for i in range(len(mins)) if mins[i] >= MARGIN]
    excl = [i for i in range(len(mins)) if mins[i] < MARGIN]
    print(f"{tag}: smallest margin per clip [{' '.join(f'{m:.2e}' for m in mins)}], MARGIN {MARGIN:.0e}, excluded {excl}")
    assert len(excl) <= len(mins) // 10, f"{tag}: {len(excl)} of {len(mins)} clips within MARGIN of a tie (choose another seed)"
    assert keep, tag
    return keep


def _oracle_decode(c, E, route, seed):
    """The CPU reference of one route on the case's features -> (seqs [N, ..], logprobs or None, margins per clip, noise)."""
    state, feats, fl = c["state"], c["feats"], c["fl"]
    g = torch.Generator().manual_seed(seed)
    rec = {}
    with torch.no_grad():
        if route in ("greedy", "sample", "gumbel"):
            noise = dict(eps_p=torch.randn(O.MAX_LENGTH, BD, E, generator=g))
            if route == "gumbel":
                noise["sample_noise"] = -torch.log(-torch.log(torch.rand(O.MAX_LENGTH, BD, VD, generator=g) + 1e-20) + 1e-20)
            elif route == "sample":
                noise["sample_noise"] = torch.empty(O.MAX_LENGTH, BD, VD).exponential_(1, generator=g)
            temp = {"greedy": 1.0, "sample": 0.8, "gumbel": 1.3}[route]
            want = O.hybrid_forward(state, feats, fl.copy(), training=False, method=route, temp=temp, noise=noise, record=rec)
            n = want["_steps_run"]
            return want["seqs"][:, :n], want["sampled_logprobs"], list(rec["margins"].numpy()), dict(noise, temp=temp)
        if route == "beam":
            eps = torch.randn(BD, O.MAX_LENGTH, 3, E, generator=g)
            return O.beam_search(state, feats, fl.copy(), 3, O.MAX_LENGTH, eps, record=rec), None, rec["margins"], dict(eps=eps)
        torch.manual_seed(seed)
        want = O.diverse_beam_search(state, feats, fl.copy(), max_length=O.MAX_LENGTH, record=rec, **DBS_CASES[0])
        return want, None, rec["margins"], {}


ROUTES = ("greedy", "sample", "gumbel", "beam", "dbs")


@pytest.mark.parametrize("S", [9, 20])
@pytest.mark.parametrize("E,H,A", W.INFER_SETS, ids=WIDTH_IDS)
def test_step_modules_vs_oracle_at_unequal_widths(E, H, A, S):
    """pnet(...) and decoder(...) one step against O.prior_step / O.decoder_step with the bounds of
    test_model_gpu.test_single_step_modules_vs_oracle, ragged lens that include 1 and S; S = 20 takes the split-over-frames
    attention where A % 4 == 0 (more than 16 frames).  log_softmax(logits) within LP_TOL, the yardstick of MARGIN."""
    N = 5
    c = _decode_case(E, H, A)
    model, state = _model_of(c, E, H, A), c["state"]
    g = torch.Generator().manual_seed(2 + S)
    mem = torch.randn(N, S, E, generator=g) * 0.5
    lens = torch.tensor([S, 7, 4, 2, 1])
    word = torch.randint(0, VD, (N, 1), generator=g)
    h = torch.rand(1, N, H, generator=g) * 2 - 1
    hp = torch.rand(1, N, E, generator=g) * 2 - 1
    cp = torch.randn(1, N, E, generator=g)
    lz, eps = torch.randn(N, E, generator=g), torch.randn(N, E, generator=g)
    assert (_lib.lib().acvae_attn_fwd_workspace_bytes(N, 1, S, A, E) > 0) == (S > 16 and A % 4 == 0)
    with torch.no_grad():
        op = O.prior_step(state, word, mem, (hp[0], cp[0]), lz, lens, eps)
        od = O.decoder_step(state, word, h[0], mem, lens, op["z"])
        hp_ = model.pnet(word, mem.cuda(), (hp.cuda(), cp.cuda()), lz.cuda(), lens, eps=eps)
        hd_ = model.decoder(word=word, state=h.cuda(), enc_mem=mem.cuda(), enc_mem_lens=lens, z=hp_["z"])
    assert hd_["state"].shape == (1, N, H) and hd_["rnn_input"].shape[-1] == 3 * E
    pairs = [("prior mean", hp_["mean"], op["mean"], 1e-4, 1e-5), ("prior z", hp_["z"], op["z"], 1e-4, 1e-5),
             ("prior h", hp_["hiddens_state"][0][0], op["hiddens_state"][0], 1e-4, 1e-5),
             ("prior c", hp_["hiddens_state"][1][0], op["hiddens_state"][1], 1e-4, 1e-5),
             ("dec logits", hd_["logits"][:, 0], od["logits"], 1e-4, 2e-5), ("dec h", hd_["state"][0], od["state"], 1e-4, 1e-5),
             ("dec attn", hd_["weights"], od["weights"], 1e-4, 1e-5),
             ("rnn_input", hd_["rnn_input"][:, 0], od["rnn_input"], 1e-4, 1e-5)]
    for what, a, b, rtol, atol in pairs:
        _ratio("step modules", a, b, rtol, atol)
        close(a, b, rtol, atol, what=f"{what} (E, H, A) = ({E}, {H}, {A}) S = {S}")
    lp_err = float((torch.log_softmax(hd_["logits"][:, 0].cpu().double(), 1) - torch.log_softmax(od["logits"].double(), 1)).abs().max())
    RATIOS["step log-probabilities (LP_TOL 1e-5)"] = max(RATIOS.get("step log-probabilities (LP_TOL 1e-5)", 0.0), lp_err / LP_TOL)
    print(f"(E, H, A) = ({E}, {H}, {A}) S = {S}: |log_softmax(logits) err| {lp_err:.2e} (bound {LP_TOL:.0e})")
    assert lp_err <= LP_TOL


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("E,H,A", W.INFER_SETS, ids=WIDTH_IDS)
def test_decoding_routes_vs_oracle_at_unequal_widths(E, H, A, route):
    """Greedy, multinomial and Gumbel sampling with replayed noise, beam 3 and diverse beam search against acvae_oracle: words
    equal on every clip whose reference decisions all clear MARGIN - with the seeds of NOISE_SEEDS every clip (_compared_rows
    allows none of four to be left out); sampled_logprobs to close(1e-4, 2e-5)."""
    c = _decode_case(E, H, A)
    seed = NOISE_SEEDS[(E, H, A)][route]
    want, want_lp, margins, noise = _oracle_decode(c, E, route, seed)
    keep = _compared_rows(f"{route} (E, H, A) = ({E}, {H}, {A})", margins)
    model = _model_of(c, E, H, A)
    f, fl = c["feats"].cuda(), c["fl"]
    with torch.no_grad():
        if route in ("greedy", "sample", "gumbel"):
            model.noise = {k: v for k, v in noise.items() if k != "temp"}
            got = model(f, fl.copy(), method=route, temp=noise["temp"])
            n = want.shape[1]
            assert torch.equal(got["seqs"].cpu()[keep, :n], want[keep]), route
            _ratio("sampled_logprobs of the decodes (1e-4, 2e-5)", got["sampled_logprobs"].cpu()[keep, :n], want_lp[keep], 1e-4, 2e-5)
            close(got["sampled_logprobs"].cpu()[keep, :n], want_lp[keep], 1e-4, 2e-5, what=f"{route} sampled_logprobs")
            return
        if route == "beam":
            model.noise = dict(eps_beam=noise["eps"])
            got = model(f, fl.copy(), method="beam", beam_size=3)["seqs"].cpu()
        else:
            torch.manual_seed(seed)
            got = model(f, fl.copy(), method="dbs", max_length=O.MAX_LENGTH, **DBS_CASES[0])["seqs"].cpu()
    assert got.shape == want.shape and torch.equal(got[keep], want[keep]), (route, [i for i in keep if not torch.equal(got[i], want[i])])


@pytest.mark.parametrize("E,H,A", W.INFER_SETS, ids=WIDTH_IDS)
def test_finishing_beam_vs_the_twin_at_unequal_widths(E, H, A):
    """method="beam" with finish_on_end=True (beam 3, length_penalty 1.0, the three best) against the route's reference: the
    host loop over the step API with beam_finish_util's retire step behind each top-k (test_finishing_beam_gpu.finishing_loop)
    and beam_finish_util.finish on its tables.  The <end> bias is raised by 1.0 so that hypotheses finish early.  Every clip is
    compared: a gap under MARGIN among the slots compared fails the case (_compared_rows; the loop and the call share their
    step kernels, so the gaps the MI355X measured, 6.5e-4 at the least, are the loop's own)."""
    beam = 3
    c = _decode_case(E, H, A, end_bump=1.0)
    model = _model_of(c, E, H, A)
    f, fl = c["feats"].cuda(), c["fl"]
    eps = [torch.randn(BD, SML, beam, E, generator=torch.Generator().manual_seed(DECODE_SEED * 100 + 11))]
    parent, word, frec, permuted = finishing_loop([model], f, fl, eps, beam, {})
    norm = BF.length_norm(SML, 1.0)
    want = BF.finish(parent, word, frec, norm, BD, beam, beam, O.END_IDX)
    gaps = []
    for n in range(BD):
        s = sorted((float(np.float32(frec[t, n * beam + j] / norm[t])) for t in range(SML) for j in range(beam)
                    if frec[t, n * beam + j] > BF.NEG_INF), reverse=True)
        gaps.append([a - b for a, b in zip(s[:beam], s[1:beam + 1])])
    keep = _compared_rows(f"finishing beam (E, H, A) = ({E}, {H}, {A})", gaps)
    assert permuted and int((want["lengths"] < SML).sum()) > 0, (permuted, want["lengths"])
    model.noise = dict(eps_beam=eps[0])
    with torch.no_grad():
        got = model(f, np.asarray(fl).copy(), method="beam", beam_size=beam, max_length=SML, finish_on_end=True,
                    length_penalty=1.0, nbest=beam)
    got = {k: v.cpu() for k, v in got.items()}
    assert np.array_equal(got["nbest_seqs"].numpy()[keep], want["seqs"][keep])
    assert np.array_equal(got["nbest_lengths"].numpy()[keep], want["lengths"][keep])
    assert float(np.abs(got["nbest_scores"].numpy()[keep] - want["scores"][keep]).max()) <= LP_TOL
    assert torch.equal(got["seqs"], got["nbest_seqs"][:, 0])


def test_constrained_beam_search_equals_the_host_loop_at_unequal_widths():
    """One constrained decode at (E, H, A) = (64, 96, 160): beam 3 under repetition penalty, n-gram ban, min_length and
    suppressed words against test_constrained_decoding_gpu.host_loop (the step API, constrain_util's twin on the downloaded
    rows, the histories gathered by parent) - the same kernels in the same order, so token for token."""
    E, H, A = W.INFER_SETS[0]
    c = _decode_case(E, H, A)
    model = _model_of(c, E, H, A)
    f, fl = c["feats"].cuda(), c["fl"]
    eps = search_noise(BD, 3, DECODE_SEED * 100 + 12)[:1]
    want, _, permuted = host_loop([model], f, fl, eps, 3, False, SEARCH)
    assert permuted
    model.noise = dict(eps_beam=eps[0])
    with torch.no_grad():
        out = model(f, np.asarray(fl).copy(), method="beam", beam_size=3, max_length=SML, **SEARCH)
    assert torch.equal(out["seqs"].cpu(), want)


def test_g19_inference_goldens_token_for_token():
    """The reference's own tokens at unequal widths (tests/golden/g19_unequal_widths.npz): greedy at (E, H, A) = (64, 64, 160)
    - the reference's greedy loop runs with H == E only - and beam 3 at (64, 96, 160), on the noise of the stored seeds."""
    g = load_golden("g19_unequal_widths")
    B, Tt, V, E, H, A, beam = (int(x) for x in g["infer_dims"])
    seed = int(g["infer_seed"])
    feats, _, fl, _ = O.synthetic_batch(B, Tt, V, 7, seed=seed, ragged=True)
    model = W.build_model(V, E, E, A, E, W.make_state(V, E, E, A, E)).eval()
    torch.manual_seed(seed + 1)
    model.noise = dict(eps_p=torch.stack([torch.randn(B, E) for _ in range(O.MAX_LENGTH)]))
    with torch.no_grad():
        o = model(feats.cuda(), fl.copy(), method="greedy")
    steps = int(g["greedy_steps_run"])
    assert np.array_equal(o["seqs"].cpu().numpy(), g["greedy_seqs"])
    close(o["sampled_logprobs"][:, :steps], g["greedy_logprobs"], 1e-4, 2e-5, what="g19 greedy logprobs")
    model = W.build_model(V, E, H, A, E, W.make_state(V, E, H, A, E)).eval()
    torch.manual_seed(seed + 2)
    eps = torch.stack([torch.stack([torch.randn(beam, E) for _ in range(O.MAX_LENGTH)]) for _ in range(B)])
    model.noise = dict(eps_beam=eps)
    with torch.no_grad():
        o = model(feats.cuda(), fl.copy(), method="beam", beam_size=beam)
    assert np.array_equal(o["seqs"].cpu().numpy(), g["beam_seqs"])


def test_training_forward_with_h_not_e_is_refused_and_the_model_still_decodes():
    """mean_log_out = Linear(E, 2E) is fed the pooled GRU outputs, so a training forward needs H == E: ValueError in front of
    every launch (the encoder's included: its dropout masks are never asked for), and the model decodes as before."""
    E, H, A = W.INFER_SETS[0]
    c = _decode_case(E, H, A)
    model = _model_of(c, E, H, A)
    f, fl = c["feats"].cuda(), c["fl"]
    noise = dict(eps_p=torch.randn(O.MAX_LENGTH, BD, E, generator=torch.Generator().manual_seed(1)))
    model.noise = dict(noise)
    with torch.no_grad():
        before = model(f, fl.copy(), method="greedy")["seqs"].clone()
    caps, cl = W.ragged_caps(BD, L, VD, torch.Generator().manual_seed(1))
    model.train()
    calls = []
    hook = model.encoder.register_forward_pre_hook(lambda m, a: calls.append(1))
    with pytest.raises(ValueError, match="hidden_size"):
        model(f, fl.copy(), caps, cl, ss_ratio=1.0, dis_ratio=0)
    hook.remove()
    assert not calls
    # the C entry refuses the shape as well (ACVAE_EUNSUPPORTED), should a caller come past the module
    torch.cuda.synchronize()
    model.eval()
    model.noise = dict(noise)
    with torch.no_grad():
        after = model(f, fl.copy(), method="greedy")["seqs"]
    assert torch.equal(before, after)
    model.check_persistent_launches()
