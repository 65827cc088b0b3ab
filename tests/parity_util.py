"""Comparison helpers shared by the GPU parity tests (test_model_gpu.py, test_fullsize_grads_gpu.py,
test_sched_sampling_gpu.py): element-wise closeness, every parameter gradient of the HIP model against the oracle's autograd
under the HIP path's own ReLU decisions, and the HIP path's own words against the oracle's decisions one by one."""
import torch


def close(a, b, rtol=1e-4, atol=1e-5, what=""):
    a = torch.as_tensor(a).detach().cpu().double(); b = torch.as_tensor(b).detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = (a - b).abs()
    ok = err <= atol + rtol * b.abs()
    assert bool(ok.all()), f"{what}: max abs err {float(err.max()):.3e} (ref max {float(b.abs().max()):.3e}), " \
                           f"{int((~ok).sum())}/{ok.numel()} out of tolerance"


def grads_match_oracle(model, named, natural_grads, rec, oracle_grads_under, tol_enc=5e-4, flip_zone=1e-4, tol_enc_of=None):
    """All parameter gradients of the HIP model against the oracle, with no tolerance for ReLU-boundary flips: the HIP
    encoder reports the ReLU decisions its backward used (model.encoder.relu_masks(); keep_saved must be set before the
    forward); they may differ from the oracle's only where its pre-activation is within rounding distance of zero
    (asserted); the oracle is re-evaluated under exactly those decisions and every tensor must agree - encoder tensors
    to `tol_enc` relative L2 (or the bound `tol_enc_of` gives that tensor by name), text-side tensors to 2e-3 / 2e-4 x max.
    Returns the oracle gradients that were matched."""
    def check(ref_grads):
        worst, worst_text = (0.0, None), (0.0, None)
        for k, ref in ref_grads.items():
            a = named[k].grad.detach().cpu().double(); b = ref.double()
            if k.startswith("encoder."):
                tol = (tol_enc_of or {}).get(k, tol_enc)
                e = float((a - b).pow(2).sum().sqrt() / max(float(b.pow(2).sum().sqrt()), 1e-12)) / tol
            else:
                lim = 2e-4 * max(float(b.abs().max()), 1e-3) + 2e-3 * b.abs()
                e = float(((a - b).abs() / lim).max())
            if e > worst[0]:
                worst = (e, k)
            if e > worst_text[0] and not k.startswith("encoder."):
                worst_text = (e, k)
        return worst + worst_text
    assert set(k for k, p in named.items() if p.grad is not None) == set(natural_grads)
    masks = [m.cpu() for m in model.encoder.relu_masks()]
    nflip, zmax = 0, 0.0
    for m, z in zip(masks, rec["relu_z"]):
        d = m != (z > 0)
        nflip += int(d.sum())
        if bool(d.any()):
            zmax = max(zmax, float(z[d].abs().max()))
    assert zmax < flip_zone, f"{nflip} ReLU decisions differ from the oracle, one at |z| = {zmax:.2e}"
    ref = natural_grads if nflip == 0 else oracle_grads_under({i: m for i, m in enumerate(masks)})
    w = check(ref)
    print(f"grads_match_oracle: worst tensor {w[1]} at {w[0]:.3f} x its tolerance, worst text-side tensor {w[3]} at {w[2]:.3f} x "
          f"({nflip} ReLU decisions differ from z > 0)")
    assert w[0] <= 1.0, f"{w[1]}: {w[0]:.2f} x tolerance under the HIP path's own ReLU decisions ({nflip} differ from z > 0)"
    return ref


def words_match_by_margin(tag, hip_seqs, hip_logits, ora_out, margins, max_left_out=0.10):
    """Token check per decision, not free-running: `ora_out` is the oracle's training forward fed the HIP path's own words
    (noise["fed_words"]), so its logits at every (row, step) answer the same input as the HIP logits there; the HIP word must
    equal the oracle's own decision wherever the oracle's margin (record["margins"]) exceeds 20 x the largest |logit
    difference| of this run.  At most `max_left_out` of the decisions may fall under that threshold: a case that leaves out
    more fails instead of passing on nothing.  Returns (share left out, threshold)."""
    hip_seqs = torch.as_tensor(hip_seqs).cpu()
    d = float((hip_logits.detach().cpu().double() - ora_out["logits"].detach().double()).abs().max())
    thr = 20 * d
    keep = margins > thr
    share = 1.0 - float(keep.double().mean())
    wrong = (hip_seqs != ora_out["seqs"]) & keep
    print(f"{tag}: max |logit difference| {d:.2e}, margin threshold {thr:.2e}, {int((~keep).sum())}/{keep.numel()} decisions "
          f"({share:.1%}) left out, smallest margin {float(margins.min()):.2e}, "
          f"{int((hip_seqs != ora_out['seqs']).sum())} words differ in all")
    assert share <= max_left_out, f"{tag}: {share:.1%} of the decisions are within {thr:.2e} of a tie (choose another seed)"
    assert not bool(wrong.any()), f"{tag}: {int(wrong.sum())} words differ from the oracle's decision at margins above " \
                                  f"{thr:.2e} (smallest such margin {float(margins[wrong].min()):.2e})"
    return share, thr
