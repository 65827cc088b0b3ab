"""The float64 yardstick of the KL objective (acvae_kl_objective_fwd / bwd, acvae_amd.train_util.KLObjective), written
from the definitions and not from the kernels.  Nothing of the package is imported.

    k[r,t,e] = lv_p/2 - lv_q/2 + (exp(lv_q) + (mu_q - mu_p)^2) / (2 exp(lv_p)) - 1/2          (text_ref.kl_terms)
    S, D:     reduction "all": every (r,t), D = R*T;   "valid": t < lens1[r], D = sum(lens1)
    free_bits None:        KL = (1/D) sum_{c in S} sum_e k[c,e]
    free_bits lam, "dim":  m_e = (1/D) sum_{c in S} k[c,e];  KL = sum_e max(m_e, lam);   dKL/dk[c,e] = [m_e > lam] / D on S
    free_bits lam, "cell": s_c = sum_e k[c,e];  KL = (1/D) sum_{c in S} max(s_c, lam);   dKL/dk[c,e] = [s_c > lam] / D on S
Cells outside S are selected away (torch.where), never multiplied by zero.

Tolerances for a kernel that evaluates k and every sum in float64 and rounds each output to fp32 once: the store's
half-ulp U |ref| (U = 2^-24), plus twice (the kernel's error and this yardstick's own) a float64 evaluation bound: the
per-element expression of text_ref.kl_fwd_tol with the float64 unit 2^-53 in place of 2^-24, added up linearly over what
an output sums (no cancellation assumed), plus K 2^-53 sum|k| for the K additions.  The clamp is 1-Lipschitz, so the
clamped sums inherit the bound of the unclamped ones.  Gradients are fp32 like kl_bwd_kernel's: text_ref.kl_bwd_tol with
D for rows, and a tolerance of exactly 0 where the gate is closed or the cell lies outside S."""
import torch

from text_ref import D as F64, U, kl_bwd, kl_bwd_tol, kl_terms

U64 = 2.0 ** -53
MODES = [(red, fb, over) for red in ("all", "valid") for fb, over in ((None, "dim"), ("lam", "dim"), ("lam", "cell"))]
MUTANTS = ("mask_ignored", "d_is_all_cells", "gate_not_strict", "clamp_other_axis", "padded_times_zero")


def cell_mask(lens1, R, T, reduction):
    if reduction == "all":
        return torch.ones(R, T, dtype=torch.bool)
    return torch.arange(T)[None, :] < torch.as_tensor(lens1).to(torch.long)[:, None]


def objective(mu_q, lv_q, mu_p, lv_p, lens1, reduction="all", free_bits=None, over="dim", mutant=None):
    """-> dict: value, raw (scalars), dims [E], steps [T], s_c [R,T] (0 outside S), gates (bool [E] / [R,T] / None), gate_full
    (bool [R,T,E]: dKL/dk * D), gates_open, mask, D.  All float64."""
    R, T, E = mu_q.shape
    k = kl_terms(mu_q, lv_q, mu_p, lv_p).reshape(R, T, E)
    mask = cell_mask(lens1, R, T, reduction)
    Dv = int(mask.sum())
    if mutant == "mask_ignored":
        mask = torch.ones(R, T, dtype=torch.bool)
    if mutant == "d_is_all_cells":
        Dv = R * T
    m3 = mask[:, :, None].expand(R, T, E)
    kS = k * m3.to(F64) if mutant == "padded_times_zero" else torch.where(m3, k, torch.zeros_like(k))
    m_e = kS.sum((0, 1)) / Dv
    s_c = kS.sum(-1)
    raw = m_e.sum()
    n_t = mask.sum(0)
    steps = torch.where(n_t > 0, s_c.sum(0) / n_t.clamp_min(1), torch.zeros(T, dtype=F64))
    open_ = (lambda a, lam: a >= lam) if mutant == "gate_not_strict" else (lambda a, lam: a > lam)
    if mutant == "clamp_other_axis" and free_bits is not None:
        over = "cell" if over == "dim" else "dim"
    if free_bits is None:
        value, gates, gate_full = raw, None, m3.clone()
        n_open = E if over == "dim" else int(mask.sum())
    elif over == "dim":
        value = torch.clamp(m_e, min=float(free_bits)).sum()
        gates = open_(m_e, free_bits)
        gate_full = m3 & gates[None, None, :]
        n_open = int(gates.sum())
    else:
        value = torch.where(mask, torch.clamp(s_c, min=float(free_bits)), torch.zeros_like(s_c)).sum() / Dv
        gates = mask & open_(s_c, free_bits)
        gate_full = m3 & gates[:, :, None]
        n_open = int(gates.sum())
    return {"value": value, "raw": raw, "dims": m_e, "steps": steps, "s_c": s_c, "gates": gates, "gate_full": gate_full,
            "gates_open": n_open, "mask": mask, "D": Dv}


def gradients(mu_q, lv_q, mu_p, lv_p, ref, g=1.0):
    """The four gradients (mu_q, lv_q, mu_p, lv_p) of g * value in float64: g * gate / D times the analytic derivatives."""
    outs = kl_bwd(mu_q, lv_q, mu_p, lv_p, g, ref["D"])
    return tuple(torch.where(ref["gate_full"], o, torch.zeros_like(o)) for o in outs)


def gradient_tols(mu_q, lv_q, mu_p, lv_p, ref, g=1.0):
    """text_ref.kl_bwd_tol scaled by the gate: 0 where the gradient is an exact zero.  Inputs outside S may hold anything."""
    sel = ref["gate_full"]
    clean = [torch.where(sel, t.to(F64), torch.zeros_like(t, dtype=F64)) for t in (mu_q, lv_q, mu_p, lv_p)]
    tols = kl_bwd_tol(*clean, g, ref["D"])
    return tuple(torch.where(sel, t, torch.zeros_like(t)) for t in tols)


def forward_tols(mu_q, lv_q, mu_p, lv_p, ref):
    """-> dict of tolerances for value, raw, dims, steps (see the module docstring)."""
    R, T, E = mu_q.shape
    m3 = ref["mask"][:, :, None].expand(R, T, E)
    a, b, c, d = (torch.where(m3, t.to(F64), torch.zeros_like(t, dtype=F64)) for t in (mu_q, lv_q, mu_p, lv_p))
    k = torch.where(m3, kl_terms(a, b, c, d).reshape(R, T, E), torch.zeros(R, T, E, dtype=F64))
    Rt = (torch.exp(b) + (a - c) ** 2) / (2 * torch.exp(d))
    e = 6 * U64 * (8 * Rt + 3 * (b.abs() / 2 + d.abs() / 2 + Rt + .5))          # kl_fwd_tol's expression at the float64 unit
    e = torch.where(m3, e, torch.zeros_like(e))
    Dv = ref["D"]
    n_t = ref["mask"].sum(0).clamp_min(1)
    f64_all = 2 * (e.sum() + R * T * E * U64 * k.abs().sum()) / Dv
    f64_dims = 2 * (e.sum((0, 1)) + R * T * U64 * k.abs().sum((0, 1))) / Dv
    f64_cell = 2 * (e.sum(-1) + E * U64 * k.abs().sum(-1))
    f64_steps = (f64_cell.sum(0) + 2 * R * U64 * ref["s_c"].abs().sum(0)) / n_t
    return {"value": U * ref["value"].abs() + f64_all, "raw": U * ref["raw"].abs() + f64_all,
            "dims": U * ref["dims"].abs() + f64_dims, "steps": U * ref["steps"].abs() + f64_steps,
            "m_e": f64_dims, "s_c": f64_cell}


def case(R, T, E, seed=0, lens=None):
    """Inputs with a per-dimension scale exp(U(-3, 0)) so that m_e and s_c spread; lens1 ragged with the longest row at T
    unless given."""
    g = torch.Generator().manual_seed(seed)
    scale = torch.exp(-3 * torch.rand(E, generator=g))
    mu_q = torch.randn(R, T, E, generator=g) * scale
    mu_p = torch.randn(R, T, E, generator=g) * scale
    lv_q = torch.randn(R, T, E, generator=g) * scale - .5
    lv_p = torch.randn(R, T, E, generator=g) * scale * .5
    if lens is None:
        lens = torch.randint(0, T + 1, (R,), generator=g)
        lens[0] = T
    return mu_q, lv_q, mu_p, lv_p, torch.as_tensor(lens).to(torch.long)


def place_lam(values):
    """lam at the midpoint of the widest gap in the middle half of the sorted values -> (lam, half-gap).  Fewer than four
    values: the widest gap of all of them; a single value: half of it."""
    v = torch.sort(values.to(F64).reshape(-1)).values
    n = v.numel()
    if n == 1:
        return float(v[0]) / 2, float(v[0].abs()) / 2
    lo, hi = (n // 4, n - n // 4) if n >= 4 else (0, n)
    mid = v[lo:hi] if hi - lo >= 2 else v
    gaps = mid[1:] - mid[:-1]
    i = int(torch.argmax(gaps))
    return float((mid[i] + mid[i + 1]) / 2), float(gaps[i] / 2)
