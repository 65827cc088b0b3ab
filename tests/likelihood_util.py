"""The yardstick of acvae_amd/likelihood.py and csrc/likelihood.hip: float64, written from the definitions.

  logprob[r,t] = x[tgt] - logsumexp(x) (torch.logsumexp in float64);   rank[r,t] by explicit counting:
  #{v : x_v > x_tgt} + #{v < tgt : x_v == x_tgt};   kl[r,t] = sum_e text_ref.kl_terms;   a cell is valid iff t < lens1[r],
  every invalid cell is zero;   per-row sums sequentially in t;   logmeanexp with a max shift.
Bounds (from text_ref's helpers, nothing here is fitted to the kernels):
  logprob: text_ref.ce_fwd_tol(logits, targets, lens1, 0.0, lse_tol(logits)) per cell - the unsmoothed CE row is -logprob;
  kl per cell: as text_ref.kl_fwd_tol builds its own - the root-sum-square of the per-element rounding
           U6 (8 R + 3 (|lv1|/2 + |lv2|/2 + R + 1/2)), R = (exp(lv1) + (mu1 - mu2)^2) / (2 exp(lv2)), plus sum_tol over E;
  rank, tokens, hit1, hit5: equality;   the float64 sums: bit equality with the sequential host loop;
  logmeanexp: LME_TOL (1 + |result|), float64 rounding of a K <= 16 term sum with generous room.
The mutants are wrong versions the bounds must flag (tests/test_likelihood_cpu.py).
"""
import numpy as np
import torch

import text_ref as R
from text_ref import D, U6

LME_TOL = 1e-12
TERM_MUTANTS = ("mask_at_len+1", "tie_rule_reversed", "kl_unmasked")
LME_MUTANTS = ("mean_in_place_of_logmeanexp", "no_max_shift")


def mask(lens1, N, T, mutant=None):
    if lens1 is None:
        return torch.ones(N, T, dtype=torch.bool)
    lens1 = torch.as_tensor(lens1).view(-1, 1)
    return torch.arange(T).view(1, T) < (lens1 + 1 if mutant == "mask_at_len+1" else lens1)


def terms(logits, targets, lens1, gauss=None, mutant=None):
    """logits [N,T,V], targets int [N,T], lens1 [N] or None, gauss (q_means, q_logs, p_means, p_logs) [N,T,E] or None
    -> logprob f64, rank i64, kl f64, each [N,T]."""
    x = logits.to(D)
    N, T, V = x.shape
    tg = targets.long()
    m = mask(lens1, N, T, mutant)
    xt = x.gather(-1, tg.unsqueeze(-1))
    logprob = xt.squeeze(-1) - torch.logsumexp(x, -1)
    idx = torch.arange(V).view(1, 1, V)
    before = idx > tg.unsqueeze(-1) if mutant == "tie_rule_reversed" else idx < tg.unsqueeze(-1)
    rank = (x > xt).sum(-1) + ((x == xt) & before).sum(-1)
    zero = torch.zeros((), dtype=D)
    logprob = torch.where(m, logprob, zero)
    rank = torch.where(m, rank, torch.zeros((), dtype=torch.long))
    kl = torch.zeros(N, T, dtype=D)
    if gauss is not None:
        E = gauss[0].shape[-1]
        kl = R.kl_terms(*gauss).view(N, T, E).sum(-1)
        if mutant != "kl_unmasked":
            kl = torch.where(m, kl, zero)
    return logprob, rank, kl


def logprob_tol(logits, targets, lens1):
    return R.ce_fwd_tol(logits, targets.long(), lens1, 0.0, R.lse_tol(logits))[0]


def kl_tol(gauss, lens1):
    mu1, lv1, mu2, lv2 = (g.to(D) for g in gauss)
    N, T, E = mu1.shape
    t = R.kl_terms(mu1, lv1, mu2, lv2).view(N, T, E)
    Rr = (torch.exp(lv1) + (mu1 - mu2) ** 2) / (2 * torch.exp(lv2))
    e = U6 * (8 * Rr + 3 * (lv1.abs() / 2 + lv2.abs() / 2 + Rr + .5))
    tol = R.rss(e, -1) + R.sum_tol(t.sum(-1), t.pow(2).sum(-1), E)
    return torch.where(mask(lens1, N, T), tol, torch.zeros((), dtype=D))


def sums(logprob, rank, kl, lens1):
    """The per-row sums of the GIVEN cells (any dtype, taken to float64 exactly), sequentially in t over the valid cells:
    numpy float64 [N] nll, kl and int64 [N] tokens, hit1, hit5."""
    lp, kk = np.asarray(logprob, dtype=np.float64), np.asarray(kl, dtype=np.float64)
    rk = np.asarray(rank)
    N, T = lp.shape
    n = np.full(N, T) if lens1 is None else np.clip(np.asarray(lens1), 0, T)
    nll, ks = np.zeros(N), np.zeros(N)
    h1, h5 = np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int64)
    for r in range(N):
        for t in range(int(n[r])):
            nll[r] = nll[r] + -lp[r, t]
            ks[r] = ks[r] + kk[r, t]
            h1[r] += rk[r, t] < 1
            h5[r] += rk[r, t] < 5
    return nll, ks, n.astype(np.int64), h1, h5


def logmeanexp(x, mutant=None):
    x = np.asarray(x, dtype=np.float64)
    if mutant == "mean_in_place_of_logmeanexp":
        return x.mean(axis=-1)
    with np.errstate(divide="ignore", over="ignore"):
        if mutant == "no_max_shift":
            return np.log(np.exp(x).mean(axis=-1))
        m = x.max(axis=-1, keepdims=True)
        return np.log(np.exp(x - m).mean(axis=-1)) + m[..., 0]


def lme_ok(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return bool(np.all(np.isfinite(got)) and np.all(np.abs(got - ref) <= LME_TOL * (1 + np.abs(ref))))


# ------------------------------------------------------------------------------------------------ planted rows
def planted(V, seed=0):
    """One row [1, 9, V] of steps that pin the rules, and its targets: the target at 0 and at V - 1; values equal to the
    target's before and after it; all logits equal; one logit 60 above the rest with the target on it and off it; every
    logit shifted by 1e4; -inf off the target (twice: the first and the last word)."""
    g = torch.Generator().manual_seed(1000 + V + seed)
    x = torch.randn(1, 9, V, generator=g) * 2
    tg = torch.randint(0, V, (1, 9), generator=g)
    tg[0, 0], tg[0, 1] = 0, V - 1
    mid = V // 2                                         # ties on both sides of the target (V >= 2: at least one side)
    tg[0, 2] = mid
    x[0, 2, ::2] = x[0, 2, mid]
    x[0, 2, mid] = x[0, 2, 0]
    x[0, 2, V - 1] = x[0, 2, 0]
    x[0, 3] = 0.25
    tg[0, 4] = V - 1
    x[0, 4, V - 1] += 60
    tg[0, 5] = 0
    x[0, 5, V - 1] += 60
    x[0, 6] += 1e4
    tg[0, 7] = V - 1
    x[0, 7, 0] = -float("inf")
    tg[0, 8] = 0
    x[0, 8, V - 1] = -float("inf")
    return x, tg
