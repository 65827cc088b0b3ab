"""GPU: every decoding method against the oracle at BASELINE.json's full sizes (V=5000, E=512, S=62 / 187 frames), at row
counts R (clips x beams) on both sides of each kernel-choice boundary of the step functions:
  - logits GEMM (M=R, N=V, K=512): skinny 32x32-tile kernel for R <= 256, the 128-row tile kernel above (skinny_plan);
    the GRU / LSTM / attention-query GEMMs take the skinny kernel at every R here, without split-K: at E=512 none of them
    has the <= 16 tiles that split K;
  - attention: split-over-frames form for R <= 128 (acvae_attn_fwd_workspace_bytes > 0), one workgroup per row above it
    (1024 threads below R = 256, 256 threads from there).
Token-exact comparisons are guarded by the oracle's own decision margins (record=): a clip whose smallest margin is below
MARGIN = 20 x LP_TOL is within the fp32 rounding of the HIP path from going the other way and is excluded - at most 10 %
of a case's clips, rounded down - while every other clip's tokens must be exact."""
import os

import numpy as np
import pytest
import torch

import acvae_oracle as O
from acvae_amd import _lib
from parity_util import close
from test_fullsize_gpu import build
from test_model_gpu import DBS_CASES

pytestmark = pytest.mark.gpu
V, E, L = 5000, 512, 22
# |log_softmax(logits)| error of one step API call against the oracle on the encoder's own memory (the decoders' input in
# every test below): measured max 2.9e-6 over the step cases (see the -s output)
LP_TOL = 1e-5
MARGIN = 20 * LP_TOL
# the same on random N(0, 1) memory: ~200x the encoder's scale at this initialisation, sharp attention; the context's
# absolute error scales with |mem| (measured max 1.1e-5)
LP_TOL_RANDN = 4e-5


@pytest.fixture(autouse=True)
def _threads():
    n = torch.get_num_threads()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    yield
    torch.set_num_threads(n)


def model_and_state(seed=5, end_bump=0.0):
    model = build(seed).eval()
    if end_bump:
        with torch.no_grad():
            model.decoder.classifier.bias[O.END_IDX] += end_bump
    return model, {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}


def lib_plans(R, S):
    """Kernel choices of one step over R rows: the split-K factor of the logits and GRU input GEMMs (0 = the 128-row tile
    kernel) and the attention's split-over-frames workspace (0 = one workgroup per row)."""
    lib = _lib.lib()
    return dict(logits=lib.acvae_gemm_nt_split_plan(R, V, E, 0, 1), gru=lib.acvae_gemm_nt_split_plan(R, 3 * E, 3 * E, 0, 1),
                lstm=lib.acvae_gemm_nt_split_plan(R, 4 * E, 3 * E, 0, 1), attn=lib.acvae_attn_fwd_workspace_bytes(R, 1, S, E, E))


def assert_plans(R, S):
    p = lib_plans(R, S)
    assert p["logits"] == (1 if R <= 256 else 0), (R, p)
    assert p["gru"] == 1 and p["lstm"] == 1, (R, p)
    assert (p["attn"] > 0) == (R <= 128), (R, S, p)
    return p


def encode_once(monkeypatch, state, feats, fl, reps=1):
    """The oracle's Cnn10 on the distinct clips once (eval mode: clip by clip independent); the decoders under test then
    read it, tiled `reps` times as feats.repeat(reps, 1, 1) tiles the batch."""
    with torch.no_grad():
        enc = O.cnn10_forward(state, feats, fl.copy(), training=False)
    rep = {"audio_embeds": enc["audio_embeds"].repeat(reps, 1, 1), "audio_embeds_pooled": enc["audio_embeds_pooled"].repeat(reps, 1),
           "state": None, "audio_embeds_lens": torch.as_tensor(enc["audio_embeds_lens"]).repeat(reps)}

    def cached(state_, feats_, feat_lens, training=True, *a, **kw):
        assert not training and feats_.shape[0] == rep["audio_embeds"].shape[0]
        return dict(rep)
    monkeypatch.setattr(O, "cnn10_forward", cached)
    return int(rep["audio_embeds"].shape[1])


def guarded(tag, margins):
    """Indices of the clips whose every decision clears MARGIN; at most 10 % (rounded down) may fall under it."""
    mins = np.array([float(np.min(m)) if len(m) else np.inf for m in margins])
    out = [i for i in range(len(mins)) if mins[i] >= MARGIN]
    excl = [i for i in range(len(mins)) if mins[i] < MARGIN]
    print(f"{tag}: smallest margin per clip [{' '.join(f'{m:.2e}' for m in mins)}], "
          f"MARGIN {MARGIN:.1e}, excluded {excl}")
    assert len(excl) <= len(mins) // 10, f"{tag}: {len(excl)} of {len(mins)} clips within MARGIN of a tie (change the seed)"
    return out


# ------------------------------------------------------------------------------------------------ step API
STEP_R = [1, 12, 33, 96, 129, 260]
_lp_err = {}
_enc_mem = {}


def encoder_memory(S):
    """The oracle's Cnn10 output of four clips (T = 1000 -> S = 62, T = 3000 -> S = 187), computed once per S."""
    if S not in _enc_mem:
        T = {62: 1000, 187: 3000}[S]
        _, state = model_and_state()
        feats, _, fl, _ = O.synthetic_batch(4, T, V, L, seed=S, ragged=False)
        with torch.no_grad():
            _enc_mem[S] = O.cnn10_forward(state, feats, fl.copy(), training=False)["audio_embeds"].contiguous()
        assert _enc_mem[S].shape[1] == S
    return _enc_mem[S]


@pytest.mark.parametrize("memory", ["encoder", "randn"])
@pytest.mark.parametrize("S", [62, 187])
@pytest.mark.parametrize("R", STEP_R)
def test_step_modules_vs_oracle_at_full_size(R, S, memory):
    """pnet.forward / decoder.forward one step on R rows with ragged lengths (1 and S among them), with and without the
    attn_split override, against O.prior_step / O.decoder_step: every output within the `close` bounds of
    test_single_step_modules_vs_oracle, and log_softmax(logits) within LP_TOL.  Memory: the encoder's output of four clips
    tiled over the rows (what the decoders see), or N(0, 1) noise (sharp attention weights; rnn_input holds the attention
    context, a weighted sum of memory frames, so its absolute bound is taken in units of max |mem|, and the log-softmax
    bound is LP_TOL_RANDN).  The step entry points take no flags: the override only reaches acvae_attn_fwd's direct
    callers, so both runs take the attention form the plan names."""
    model, state = model_and_state()
    p = assert_plans(R, S)
    g = torch.Generator().manual_seed(R * 1000 + S)
    if memory == "encoder":
        mem = encoder_memory(S).repeat((R + 3) // 4, 1, 1)[:R].contiguous()
    else:
        mem = torch.randn(R, S, E, generator=g)
    lens = torch.randint(1, S + 1, (R,), generator=g)
    lens[0] = S
    if R > 1:
        lens[-1] = 1
    word = torch.randint(0, V, (R, 1), generator=g)
    h = torch.rand(1, R, E, generator=g) * 2 - 1
    hp = torch.rand(1, R, E, generator=g) * 2 - 1
    cp = torch.randn(1, R, E, generator=g)
    lz, eps = torch.randn(R, E, generator=g), torch.randn(R, E, generator=g)
    with torch.no_grad():
        op = O.prior_step(state, word, mem, (hp[0], cp[0]), lz, lens, eps)
        od = O.decoder_step(state, word, h[0], mem, lens, op["z"])
    lp_want = torch.log_softmax(od["logits"].double(), 1)
    lp_tol = LP_TOL if memory == "encoder" else LP_TOL_RANDN
    mscale = max(1.0, float(mem.abs().max()))
    for split in (True, False):
        with _lib.override(attn_split=split), torch.no_grad():
            hp_ = model.pnet(word, mem.cuda(), (hp.cuda(), cp.cuda()), lz.cuda(), lens, eps=eps)
            hd_ = model.decoder(word=word, state=h.cuda(), enc_mem=mem.cuda(), enc_mem_lens=lens, z=hp_["z"])
        tag = f"R={R} S={S} {memory} memory, attn_split={split}"
        close(hp_["mean"], op["mean"], what=tag + " prior mean"); close(hp_["z"], op["z"], what=tag + " prior z")
        close(hp_["hiddens_state"][0][0], op["hiddens_state"][0], what=tag + " prior h")
        close(hp_["hiddens_state"][1][0], op["hiddens_state"][1], what=tag + " prior c")
        close(hd_["logits"][:, 0], od["logits"], 1e-4, 2e-5, what=tag + " dec logits")
        close(hd_["state"][0], od["state"], what=tag + " dec h")
        close(hd_["weights"], od["weights"], what=tag + " dec attn")
        close(hd_["rnn_input"][:, 0], od["rnn_input"], 1e-4, 1e-5 * mscale, what=tag + " rnn_input")
        lp_err = float((torch.log_softmax(hd_["logits"][:, 0].cpu().double(), 1) - lp_want).abs().max())
        _lp_err[(R, S, memory, split)] = lp_err
        worst = max(v for k, v in _lp_err.items() if k[2] == memory)
        print(f"{tag}: plans {p}; |log_softmax(logits) err| {lp_err:.2e} (bound {lp_tol:.0e}); max so far {worst:.2e}")
        assert lp_err <= lp_tol, (tag, lp_err)


# ------------------------------------------------------------------------------------------------ beam search
BEAM_CASES = {                       # beam, clips, T, seed of the features, seed of the prior's noise
    "beam3_4clips": (3, 4, 1000, 1, 101),            # R = 12: attention split over frames
    "beam5_8clips": (5, 8, 1000, 2, 102),            # R = 40
    "beam16_2clips": (16, 2, 1000, 6, 106),          # n = 16 x 5000 = 80 000 scores per top-k
    "beam3_6clips_t3000": (3, 6, 3000, 9, 45),       # S = 187
    "beam5_53clips": (5, 53, 160, 3, 103),           # R = 265: logits on the 128-row tile kernel, 256-thread attention
}


@pytest.mark.parametrize("case", list(BEAM_CASES))
def test_beam_search_vs_oracle_at_full_size(case, monkeypatch):
    """method="beam" (one library call for the whole batch) against O.beam_search with the same replayed eps_beam."""
    beam, N, T, fseed, eseed = BEAM_CASES[case]
    model, state = model_and_state()
    feats, _, fl, _ = O.synthetic_batch(N, T, V, L, seed=fseed, ragged=True)
    for b in range(N):
        feats[b, int(fl[b]):] = 0.0
    S = encode_once(monkeypatch, state, feats, fl)
    p = assert_plans(N * beam, S)
    eps = torch.randn(N, O.MAX_LENGTH, beam, E, generator=torch.Generator().manual_seed(eseed))
    rec = {}
    with torch.no_grad():
        want = O.beam_search(state, feats, fl.copy(), beam, O.MAX_LENGTH, eps, record=rec)
        model.noise = dict(eps_beam=eps)
        got = model(feats.cuda(), fl.copy(), method="beam", beam_size=beam)["seqs"].cpu()
    print(f"{case}: R={N * beam} S={S} plans {p}")
    keep = guarded(case, rec["margins"])
    assert torch.equal(got[keep], want[keep]), (case, [i for i in keep if not torch.equal(got[i], want[i])])


# ------------------------------------------------------------------------------------------------ diverse beam search
DBS_FULL = [(0, 0.0, 42), (1, 0.0, 46), (2, 0.0, 42), (3, 0.0, 43), (0, 6.0, 40)]   # DBS_CASES index, <end> bias raised
                                                                                   # (beams finish early), generator seed


@pytest.mark.parametrize("ci,bump,seed", DBS_FULL)
def test_diverse_beam_search_vs_oracle_at_full_size(ci, bump, seed, monkeypatch):
    """method="dbs" (step API + acvae_dbs_scores with one count vector per clip + acvae_topk_flat_batched) on 3 clips
    against O.diverse_beam_search drawing the prior's noise from the same generator state."""
    kw = DBS_CASES[ci]
    model, state = model_and_state(end_bump=bump)
    feats, _, fl, _ = O.synthetic_batch(3, 1000, V, L, seed=11, ragged=True)
    for b in range(3):
        feats[b, int(fl[b]):] = 0.0
    encode_once(monkeypatch, state, feats, fl)
    rec = {}
    torch.manual_seed(seed)                    # the prior's randn draws: CPU generator, call order (clip, t, group)
    with torch.no_grad():
        want = O.diverse_beam_search(state, feats, fl.copy(), max_length=O.MAX_LENGTH, record=rec, **kw)
    torch.manual_seed(seed)
    with torch.no_grad():
        got = model(feats.cuda(), fl.copy(), method="dbs", max_length=O.MAX_LENGTH, **kw)["seqs"].cpu()
    ended_early = int((want[..., :-1] == O.END_IDX).any(-1).sum())
    print(f"dbs {kw} end bump {bump}: {ended_early} of {want.shape[0] * want.shape[1]} output beams ended before the last step")
    if bump:
        assert ended_early > 0
    keep = guarded(f"dbs {kw} bump {bump}", rec["margins"])
    assert torch.equal(got[keep], want[keep]), (kw, bump)


# ------------------------------------------------------------------------------------------------ sampling and greedy
SAMPLE_SHAPES = {20: (4, 1000), 40: (8, 500)}       # N = clips x 5 z-samples; N <= 32: the persistent decode launch


@pytest.mark.parametrize("N", [20, 40])
@pytest.mark.parametrize("method", ["sample", "gumbel", "greedy"])
def test_sampled_decoding_vs_oracle_at_full_size(method, N, monkeypatch):
    """method="sample" / "gumbel" with replayed sample_noise at temp 0.7 / 1.0 / 1.5, and greedy; N = 20 (one persistent
    launch) and N = 40 (per-step launches).  Tokens exact per guarded row, sampled_logprobs within close(1e-4, 2e-5)."""
    clips, T = SAMPLE_SHAPES[N]
    model, state = model_and_state()
    feats, _, fl, _ = O.synthetic_batch(clips, T, V, L, seed=N + 1, ragged=True)
    for b in range(clips):
        feats[b, int(fl[b]):] = 0.0
    S = encode_once(monkeypatch, state, feats, fl, reps=5)
    f5 = feats.repeat(5, 1, 1).cuda()
    l5 = [int(x) for _ in range(5) for x in fl]
    temps = (1.0,) if method == "greedy" else (0.7, 1.0, 1.5)
    for ti, temp in enumerate(temps):
        g = torch.Generator().manual_seed(100 * N + 10 * ti + len(method))
        eps = torch.randn(O.MAX_LENGTH, N, E, generator=g)
        noise = dict(eps_p=eps)
        if method == "gumbel":
            U = torch.rand(O.MAX_LENGTH, N, V, generator=g)
            noise["sample_noise"] = -torch.log(-torch.log(U + 1e-20) + 1e-20)
        elif method == "sample":
            noise["sample_noise"] = torch.empty(O.MAX_LENGTH, N, V).exponential_(1, generator=g)
        rec = {}
        with torch.no_grad():
            want = O.hybrid_forward(state, f5.cpu(), np.asarray(l5), training=False, method=method, temp=temp, noise=noise,
                                    record=rec)
            model.noise = dict(noise)
            got = model(f5, list(l5), method=method, temp=temp)
        n = want["_steps_run"]
        keep = guarded(f"{method} N={N} S={S} temp={temp}", rec["margins"].numpy())
        assert torch.equal(got["seqs"].cpu()[keep, :n], want["seqs"][keep, :n]), (method, N, temp)
        close(got["sampled_logprobs"].cpu()[keep, :n], want["sampled_logprobs"][keep], 1e-4, 2e-5,
              what=f"{method} N={N} temp={temp} sampled_logprobs")
