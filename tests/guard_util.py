"""Shared by the non-finite guard's tests: a numpy twin of acvae_guard_witness / acvae_guard_decide / acvae_guard_restore
written from the definitions in include/acvae_hip.h (counters as Python ints, scalars in float64 rounded once to fp32), the
brute-force form it is checked against, and the record's layout as the GPU tests read it back."""
import math

import numpy as np

RECORD_WORDS = 28                       # ACVAE_GUARD_RECORD_BYTES / 4
MAX_GROUPS = 8
ADAM, SGD = 0, 1


def nonfinite(x):
    return not bool(np.isfinite(np.asarray(x, dtype=np.float32)).all())


def host_scalars(lr, beta1, beta2, t):
    """(step_size, bc2_sqrt) as acvae_adamw_groups_step forms them on the host for step = t: double, rounded once."""
    bc1 = 1.0 - math.pow(beta1, float(t))
    bc2 = 1.0 - math.pow(beta2, float(t))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.float32(np.float64(lr) / np.float64(bc1)), np.float32(math.sqrt(bc2))


def host_ema_w(decay, updates, warmup):
    """(float)(1 - ema_decay_at(decay, updates, warmup)), the weight acvae_ema_step forms from the host's decay."""
    d = min(float(decay), (1.0 + updates) / (10.0 + updates)) if warmup else float(decay)
    return np.float32(1.0 - d)


def sequence(seed, n=60, groups=2):
    """[(witness calls [(loss, buf)], total_norm, lr[], beta1[], beta2[])]: ok and bad decisions of every kind, the betas and
    learning rates changing on the way."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        calls = []
        for _ in range(int(rng.integers(0, 3))):
            loss = np.float32(rng.normal())
            buf = rng.normal(size=int(rng.integers(0, 9))).astype(np.float32)
            r = rng.random()
            if r < 0.12:
                loss = np.float32([np.nan, np.inf, -np.inf][int(rng.integers(0, 3))])
            elif r < 0.24 and buf.size:
                buf[int(rng.integers(0, buf.size))] = [np.nan, np.inf, -np.inf][int(rng.integers(0, 3))]
            calls.append((loss, buf))
        norm = np.float32(abs(rng.normal()) * 3)
        if rng.random() < 0.15:
            norm = np.float32([np.nan, np.inf][int(rng.integers(0, 2))])
        era = i // 20
        lr = [1e-3 * (1 + k) / (1 + era) for k in range(groups)]
        b1 = [0.9 - 0.01 * k - 0.02 * era for k in range(groups)]
        b2 = [0.999 - 0.001 * k - 0.002 * era for k in range(groups)]
        out.append((calls, norm, lr, b1, b2))
    return out


class GuardTwin:
    """The record and the three entries that move it.  ``mutant`` names one deliberate mistake (the CPU test shows that the
    brute-force comparison catches each): "t_before", "streak_kept", "flag_kept", "ema_on_skip"."""

    def __init__(self, mutant=None):
        self.applied = self.skipped = self.streak = self.ema_updates = 0
        self.ok = self.window_bad = 0
        self.step_size = np.zeros(MAX_GROUPS, np.float32)
        self.bc2_sqrt = np.zeros(MAX_GROUPS, np.float32)
        self.ema_w = np.float32(0)
        self.mutant = mutant

    def witness(self, loss=None, buf=None):
        bad = (loss is not None and nonfinite(loss)) or (buf is not None and nonfinite(buf))
        self.window_bad |= int(bad)

    def decide(self, total_norm, kind, lr, beta1=None, beta2=None, ema_decay=-1.0, ema_warmup=False):
        ok = int(not nonfinite(total_norm) and not self.window_bad)
        if ok:
            self.applied += 1
            t = self.applied - 1 if self.mutant == "t_before" else self.applied
            if self.mutant != "streak_kept":
                self.streak = 0
            if kind == ADAM:
                for k in range(len(lr)):
                    self.step_size[k], self.bc2_sqrt[k] = host_scalars(lr[k], beta1[k], beta2[k], t)
        else:
            self.skipped += 1
            self.streak += 1
        if ema_decay >= 0 and (ok or self.mutant == "ema_on_skip"):
            self.ema_w = host_ema_w(ema_decay, self.ema_updates, ema_warmup)
            self.ema_updates += 1
        self.ok = ok
        if self.mutant != "flag_kept":
            self.window_bad = 0
        return ok

    def restore(self, dst, snapshot):
        if not self.ok:
            dst[...] = snapshot

    def fields(self):
        return {"applied": self.applied, "skipped": self.skipped, "streak": self.streak, "ema_updates": self.ema_updates,
                "ok": self.ok, "window_bad": self.window_bad}


def brute_force(history, kind, ema_decay=-1.0, ema_warmup=False):
    """The record after ``history`` = [(bad_witness, total_norm, lr[], beta1[], beta2[])], recomputed from the whole
    history at once: no state is carried from decision to decision."""
    oks = []
    for bad, norm, *_ in history:
        oks.append(not bad and bool(np.isfinite(np.float32(norm))))
    applied = sum(oks)
    streak = 0
    for o in reversed(oks):
        if o:
            break
        streak += 1
    out = {"applied": applied, "skipped": len(oks) - applied, "streak": streak, "ok": int(oks[-1]) if oks else 0,
           "window_bad": 0, "ema_updates": applied if ema_decay >= 0 else 0}
    step_size, bc2_sqrt, ema_w = np.zeros(MAX_GROUPS, np.float32), np.zeros(MAX_GROUPS, np.float32), np.float32(0)
    if applied:
        if kind == ADAM:
            # groups beyond the last decision's keep what an earlier applied decision with more groups left there
            for i, o in enumerate(oks):
                if o:
                    t = sum(oks[:i + 1])
                    _, _, lr, b1, b2 = history[i]
                    for k in range(len(lr)):
                        step_size[k], bc2_sqrt[k] = host_scalars(lr[k], b1[k], b2[k], t)
        if ema_decay >= 0:
            ema_w = host_ema_w(ema_decay, applied - 1, ema_warmup)
    out.update(step_size=step_size, bc2_sqrt=bc2_sqrt, ema_w=ema_w)
    return out


def read_record(rec):
    """A device (or host) int32 [28] record tensor -> dict of Python ints and fp32 arrays."""
    w = rec.detach().cpu().numpy().astype(np.int32)
    c = w[:8].view(np.int64)
    return {"applied": int(c[0]), "skipped": int(c[1]), "streak": int(c[2]), "ema_updates": int(c[3]),
            "ok": int(w[8]), "window_bad": int(w[9]), "step_size": w[10:18].view(np.float32).copy(),
            "bc2_sqrt": w[18:26].view(np.float32).copy(), "ema_w": w[26:27].view(np.float32)[0], "reserved": int(w[27])}
