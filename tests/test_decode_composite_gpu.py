"""GPU: acvae_decode_fwd / acvae_decode_fwd_sampled / acvae_decode_bwd element by element against float64.

The composite is the only way into csrc/decoder.hip, the persistent BPTT of csrc/decode_persist.hip and the backward glue of
csrc/rnn.hip (gru_bwd / lstm_bwd / pool_bwd / embed_scatter / colsum_rows / add_rows kernels).  Every case of
tests/decode_ref.py CASES is called THROUGH THE C ABI with guarded, 0xFF-filled workspaces (tests/ws_guard.py; the scratch
is poisoned again between forward and backward), NaN-prefilled outputs and gradients, and random upstream gradients on the
case's subset of the six outputs (the rest NULL).  Every forward output (the rows' log-sum-exp in `saved` included), every
parameter gradient the call owns, d_mem_in and d_q_z is compared with the float64 run of tests/decode_ref.py, no element
left out, under

    |got - ref| <= max(1e-5, 8 r32) max(|ref|, rms(ref))        r32: the float32 run of the same reference against float64

per tensor and per case (tests/decode_ref.py tolerance; tests/test_decode_ref_cpu.py shows the bound flags eleven kinds of
wrong backward, the two mistakes of a split attention backward at every S > 64 case itself).  A tensor no given upstream reaches is exactly zero in the reference and must be written as exactly zero.
d_mem_in at frames >= mem_lens[n] is exactly zero in the reference; what the HIP path leaves there is printed and held to
the bound like every other element.  The max-pool margin of the float64 outputs is asserted (>= 1e-4), so no arg-max
decision is close enough to flip.

Every case asserts the path it means to take and prints it: what widths_util.plans says about both persistent launches at
its shape, the flags it passes, acvae_decode_bwd_defers, the split attention's eligibility, and the persistent launches'
status words afterwards.  Cases that feed model words (mixed scheduled sampling, the differentiable rollouts) replay the
HIP forward's own `seqs` into the reference as constants, so no decision is compared.

Clips of more than 64 frames (decode_ref.S_LONG): the persistent BPTT's attention role then runs as 2 or 3 workgroups per
clip.  Each such case also asserts and prints rc_splits, dqd_part_floats > 0, dv_rows = N rc_splits, which forward attention
form the plan chooses (memory-resident or streamed; both occur) and that both grids fit the device at one workgroup per CU.
They cover a last share of 1, 2, 59 and 64 frames, clips that leave one or two of their shares fully masked, Tc = 1 and 2,
N = 1 and 32, a per-step forward feeding the split backward, a NULL d_logits, embedding dropout, A = 512 (the batched sum of
the d qd shares) and E = 512 with three shares; S = 66, 130 and 187 also run per step on the same reference.

Worst measured error / tolerance on the MI355X, per tensor group (test_zz_worst_ratio_per_group prints the table):
    forward outputs               0.20  (cp, E512_A512_S66)
    input gradients               0.39  (d_mem_in, S66-Tc1)
    decoder gradients             0.57  (attn.h2attn.bias, S66)
    prior gradients               0.36  (word_attn.h2attn.bias, only_p_logs)
    mean_log_out / ln gradients   0.15  (ln.weight, only_outputs)
No tensor needed more than the factor 8; d_mem_in at frames >= mem_lens was exactly 0 in every case; the smallest max-pool
margin was 2.6e-4.

What these cases found: with rc_splits > 1 the persistent BPTT writes the sum of the d qd shares for steps 1 .. Tc - 1
only, and the query half of decoder.attn.h2attn.weight's gradient multiplied whatever the scratch held in step 0's rows by
h_{-1} = 0: NaN under the 0xFF fill of this file, in every persistent case above and in no other tensor.
acvae_decode_bwd now zeroes dqd at its entry.  See DESIGN.md section 2."""
import ctypes

import pytest
import torch

import decode_ref as R
import widths_util as W
from acvae_amd import _lib
from acvae_amd.decoder import _ProjTableFn
from ws_guard import guarded, ws_guards  # noqa: F401  (autouse fixture: every guard intact after each test)

pytestmark = pytest.mark.gpu
NAN = float("nan")
INT_FILL = -77

TABLE = ["decoder.word_embeddings.weight", "decoder.model.weight_ih_l0", "decoder.model.weight_hh_l0",
         "decoder.model.bias_ih_l0", "decoder.model.bias_hh_l0", "decoder.classifier.weight", "decoder.classifier.bias",
         "decoder.attn.v", "decoder.attn.h2attn.weight", "decoder.attn.h2attn.bias"] + [None] * 11 + \
        ["pnet.word_embedding.weight", "pnet.word_attn.v", "pnet.word_attn.h2attn.weight", "pnet.word_attn.h2attn.bias",
         "pnet.network.weight_ih_l0", "pnet.network.weight_hh_l0", "pnet.network.bias_ih_l0", "pnet.network.bias_hh_l0",
         "pnet.mean_log_out.weight", "pnet.mean_log_out.bias", "mean_log_out.weight", "mean_log_out.bias", "ln.weight", "ln.bias"]
assert len(TABLE) == _lib.ENUMS_TEXT_N
FLAGS = {"persist": 0, "per_step": _lib.FLAG_NO_PERSIST, "no_split": _lib.FLAG_NO_PERSIST | _lib.FLAG_NO_ATTN_SPLIT,
         "defer": _lib.FLAG_DEFER_PARAM_GRADS, "defer_per_step": _lib.FLAG_DEFER_PARAM_GRADS | _lib.FLAG_NO_PERSIST}
WORST = {}          # (group, tensor) -> (error / tolerance, case)
_aux = []


def group_of(name):
    if name.startswith("fwd."):
        return "forward outputs"
    if name in ("d_mem", "d_q_z"):
        return "input gradients"
    if name.startswith("g.decoder."):
        return "decoder gradients"
    if name.startswith("g.pnet."):
        return "prior gradients"
    return "mean_log_out / ln gradients"


def nans(*shape):
    return torch.full(shape, NAN, device="cuda")


def aux_stream():
    if not _aux:
        _aux.append(torch.cuda.Stream())
    return _aux[0]


def run_hip(c):
    """The case on the HIP path, its path asserted and printed -> ({tensor name: device tensor}, the fed words [N, Tc] on the
    host, the case's inputs)."""
    N, Tc, S, E, H, A, V, Eenc = dims = (c.N, c.Tc, c.S, c.E, c.H, c.A, c.V, c.Eenc)
    d, state = R.inputs(c), R.make_state(c)
    dev = {k: v.cuda().contiguous() for k, v in state.items()}
    proj = None
    if c.proj:       # the library sees one [V, E] table; Embedding . Linear^T + bias and its backward are _ProjTableFn's products
        proj = [dev["decoder.word_embeddings.%s" % k].requires_grad_(True) for k in ("0.weight", "1.weight", "1.bias")]
        table = _ProjTableFn.apply(None, *proj)
        dev["decoder.word_embeddings.weight"] = table.detach()
    params = [None if k is None else dev.get(k) for k in TABLE]
    assert (params[33] is not None) == c.ln
    flags = FLAGS[c.path] | (_lib.FLAG_ROLLOUT_GRAD if c.rollout else 0)
    defer_asked = c.path.startswith("defer")
    main = _lib.current_stream()
    aux = aux_stream().cuda_stream if defer_asked else None
    IntArr = ctypes.c_int * Tc
    dis_arr, ss_arr = IntArr(*([1] * Tc if c.rollout else R.dis_flags(c))), IntArr(*R.ss_flags(c))

    # ---- the path this case means to take
    path = {"flags": flags}
    if not c.rollout:
        plan = W.plans(N, Tc, S, E, H, A, E)
        path["persistent launches eligible"] = bool(plan["fwd_ok"] and plan["bwd_ok"])
        assert path["persistent launches eligible"] == c.persist_ok, (c.name, plan)
        persist = c.persist_ok and not (flags & _lib.FLAG_NO_PERSIST) and c.dis == "none"
        path["forward"] = "persistent" if persist and c.ss == "all" else "per step"
        path["backward"] = "persistent" if persist else "per step"
        assert (c.path in ("persist", "defer")) == (persist or c.dis != "none"), c.name
        defers = int(_lib.lib().acvae_decode_bwd_defers(dis_arr, Tc, main, aux, flags))
        assert defers == int(defer_asked and c.dis == "none"), (c.name, defers)
        path["parameter gradients deferred"] = bool(defers)
        if c.S >= 64:
            assert plan["rc_splits"] == -(-c.S // 64), plan            # 64 frames per attention workgroup of the BPTT
            path["attention shares per clip (BPTT)"] = plan["rc_splits"]
        if c.S > 64:      # the split attention role: d qd handed over as shares, one dvpart row per clip and share
            assert plan["dqd_part_floats"] == plan["rc_splits"] * N * Tc * A > 0, plan
            assert plan["dv_rows"] == N * plan["rc_splits"], plan
            assert not c.att or plan["fwd_att_resident"] == int(c.att == "resident"), (c.name, plan)
            path.update({"dqd_part_floats": plan["dqd_part_floats"], "dv_rows": plan["dv_rows"],
                         "att_resident (forward)": plan["fwd_att_resident"], "grids": (plan["fwd_grid"], plan["bwd_grid"])})
            if persist:   # one workgroup per CU always fits (LDS <= 150 KB): then the library takes the launches it is asked for
                cus = torch.cuda.get_device_properties(0).multi_processor_count
                assert max(plan["fwd_grid"], plan["bwd_grid"]) <= cus, (c.name, plan, cus)
                path["grid resident"] = True
        if c.path in ("per_step", "no_split") and c.S == 64:
            assert _lib.call("acvae_attn_fwd_workspace_bytes", N, 1, S, A, E) > 0      # the split form is eligible here ...
            path["attention"] = "one workgroup (NO_ATTN_SPLIT)" if c.path == "no_split" else "split over frames"
    else:
        path["forward"] = path["backward"] = "per step (rollout)"
    print(f"\n{c.name}: path {path}")

    mem, mem_lens = d["mem"].cuda(), d["mem_lens"].cuda()
    caps, lens1 = d["caps"].cuda().contiguous(), d["lens1"].cuda()
    q_z, eps_p = d["q_z"].cuda(), d["eps_p"].cuda()
    keep = None if d["emb_keep"] is None else d["emb_keep"].cuda().contiguous()
    noise = None if d["noise"] is None else d["noise"].cuda()
    O = {"logits": nans(N, Tc, V), "outputs": nans(N, Tc, H), "slp": nans(N, Tc), "attn_w": nans(N, Tc, S),
         "p_means": nans(N, Tc, E), "p_logs": nans(N, Tc, E), "p_z": nans(N, Tc, E),
         "p_means_utt": None if c.rollout else nans(N, 2 * E), "h": nans(N, H), "hp": nans(N, E), "cp": nans(N, E)}
    seqs = torch.full((N, Tc), INT_FILL, dtype=torch.long, device="cuda")
    nb = {"saved": _lib.call("acvae_decode_saved_bytes", *dims), "scratch": _lib.call("acvae_decode_scratch_bytes", *dims)}
    assert min(nb.values()) > 0, nb
    ws = {k: guarded(n, 0xFF, what=f"{c.name} {k}") for k, n in nb.items()}
    _lib.persist_status(torch.device("cuda"))
    head = (params, mem, mem_lens) + ((None, 0, None, None) if c.rollout else (caps, caps.stride(0), lens1, q_z)) + \
           (eps_p, None if c.rollout else ss_arr, dis_arr, O["logits"], O["outputs"], seqs, O["slp"], O["attn_w"], O["p_means"],
            O["p_logs"], O["p_z"], O["p_means_utt"], O["h"], O["hp"], O["cp"], ws["saved"].data_ptr(), nb["saved"],
            ws["scratch"].data_ptr(), nb["scratch"], *dims, R.START, R.END, main, aux)
    fwd_flags = flags & ~_lib.FLAG_DEFER_PARAM_GRADS
    if c.rollout:
        _lib.call("acvae_decode_fwd_sampled", *head, 2, 0.8, noise, None, 0.0, fwd_flags)
    elif keep is not None:
        _lib.call("acvae_decode_fwd_sampled", *head, 0, 1.0, None, keep, c.p, fwd_flags)
    else:
        _lib.call("acvae_decode_fwd", *head, fwd_flags)
    torch.cuda.synchronize()
    assert not bool((seqs == INT_FILL).any()) and not bool(torch.isnan(O["slp"]).any()), c.name
    ws["scratch"].refill(0xFF)                      # the backward must not count on what the forward left in the scratch

    own = [i for i, k in enumerate(TABLE) if params[i] is not None and not (c.rollout and i in (31, 32))]
    grads = [torch.full_like(params[i], NAN) if i in own else None for i in range(len(TABLE))]
    d_mem, d_q_z = nans(N, S, Eenc), None if c.rollout else nans(N, Tc, E)
    ups = [d["ups"][k].cuda() if k in d["ups"] else None for k in R.UPS]
    _lib.call("acvae_decode_bwd", params, grads, mem, mem_lens, None if c.rollout else lens1, eps_p,
              None if c.rollout else dis_arr, O["outputs"], O["attn_w"], O["p_logs"], *ups, d_mem, d_q_z, ws["saved"].data_ptr(),
              nb["saved"], ws["scratch"].data_ptr(), nb["scratch"], *dims, main, aux, keep, c.p, flags)
    if aux is not None:
        torch.cuda.current_stream().wait_stream(aux_stream())       # the trailing parameter gradients: joined before reading
    torch.cuda.synchronize()
    _lib.check_persist_status(torch.device("cuda"))                 # a persistent launch that gave up would say so here
    for h in ws.values():
        h.check()

    off = _lib.call("acvae_decode_saved_lse_offset", *dims)
    assert 0 <= off and off + N * Tc * 4 <= nb["saved"] and off % 4 == 0
    got = {"fwd." + k: v for k, v in O.items() if v is not None and k != "slp"}
    got["fwd.lse"] = ws["saved"].view[off:off + N * Tc * 4].clone().view(torch.float32).view(N, Tc)
    got["d_mem"] = d_mem
    if d_q_z is not None:
        got["d_q_z"] = d_q_z
    for i in own:
        got["g." + TABLE[i]] = grads[i]
    if proj is not None:
        table.backward(got.pop("g.decoder.word_embeddings.weight"))
        torch.cuda.synchronize()
        for k, p in zip(("0.weight", "1.weight", "1.bias"), proj):
            got["g.decoder.word_embeddings." + k] = p.grad
    words = R.fed_words(c, d["caps"], seqs.cpu())
    return got, words, d


@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_decode_composite(case):
    c = case
    got, words, d = run_hip(c)
    replayed = c.rollout or c.ss != "all"
    y = R.yardstick_for(c, words) if replayed else R.yardstick(c)
    assert set(got) == set(y), sorted(set(got) ^ set(y))            # no tensor left out
    if not c.rollout:
        margin = R.margin_of(y["fwd.outputs"][0], d["lens1"])
        print(f"{c.name}: max-pool margin {margin:.2e}")
        assert margin >= R.POOL_MARGIN, (c.name, margin)
    past = torch.arange(c.S).view(1, -1, 1) >= d["mem_lens"].view(-1, 1, 1)
    left = got["d_mem"].detach().cpu() * past
    print(f"{c.name}: d_mem_in at frames >= mem_lens: max |value| {float(left.abs().max()):.3e} "
          f"(reference: exactly 0; {int(past.sum()) * c.Eenc} elements)")
    bad = []
    for k, (ref, r32) in sorted(y.items()):
        g = got[k]
        assert not bool(torch.isnan(g).any()), f"{c.name} {k}: left NaN (never written)"
        ex = R.excess(g, ref, r32)
        key = (group_of(k), k[2:] if k.startswith("g.") else k)
        if ex > WORST.get(key, (-1.0, ""))[0]:
            WORST[key] = (ex, c.name)
        if ex > 1.0:
            bad.append(f"{k}: error / tolerance {ex:.3g} (r32 {r32:.2e}, rms(ref) {float(ref.double().pow(2).mean().sqrt()):.3e})")
    worst = max(((R.excess(got[k], ref, r32), k) for k, (ref, r32) in y.items()))
    print(f"{c.name}: worst error / tolerance {worst[0]:.3f} ({worst[1]}) over {len(y)} tensors, "
          f"{sum(v[0].numel() for v in y.values())} elements")
    assert not bad, f"{c.name}: " + "; ".join(bad)


def test_zz_worst_ratio_per_group():
    """Prints the worst measured error / tolerance per tensor group and tensor (the figures of DESIGN.md section 2); runs
    last, over whatever cases ran before it."""
    groups = {}
    for (grp, name), (ex, case) in WORST.items():
        groups.setdefault(grp, []).append((ex, name, case))
    for grp in sorted(groups):
        top = max(groups[grp])
        print(f"\n{grp}: worst error / tolerance {top[0]:.3f} ({top[1]} in {top[2]})")
        for ex, name, case in sorted(groups[grp], reverse=True):
            print(f"    {name:44s} {ex:6.3f}  {case}")
    assert all(ex <= 1.0 for ex, _ in WORST.values())
