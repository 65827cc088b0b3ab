"""The declared scratch of the eight search size functions (acvae_beam_search*, acvae_ensemble_search*, acvae_dbs_search,
acvae_ensemble_dbs_search: `_scratch_bytes`) at a few shapes: host arithmetic, no GPU.  One line per value,
<shape> <function> <bytes>; run it from two trees and compare to see whether a layout change moved a size.

  python tools/search_scratch_sizes.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from acvae_amd import _lib  # noqa: E402


def arr(*v):
    return np.ascontiguousarray(v, dtype=np.int32)


V = 60
shapes = {
    "N3_beam3_T20_S4_equal": dict(N=3, beam=3, T=20, m=[(4, 64, 64, 64)]),
    "one_member_H!=E!=A": dict(N=3, beam=3, T=20, m=[(4, 64, 96, 160)]),
    "M2_unequal": dict(N=3, beam=3, T=20, m=[(4, 64, 96, 160), (4, 128, 64, 64)]),
    "odd_R_N3_beam5_S7": dict(N=3, beam=5, T=7, m=[(7, 64, 40, 50)]),
}


def show(shape, tag, fn, *args):
    print(shape, tag + fn, _lib.call(fn, *args))


for name, s in shapes.items():
    N, beam, T, m = s["N"], s["beam"], s["T"], s["m"]
    cols = [arr(*[x[j] for x in m]) for j in range(4)]              # HOST arrays S, E, H, A of the ensemble entries
    host = [c.ctypes.data for c in cols]
    for suf in ("", "_constrained", "_finishing"):
        if len(m) == 1:
            show(name, "", f"acvae_beam_search{suf}_scratch_bytes", N, beam, T, *m[0], V)
        show(name, "", f"acvae_ensemble_search{suf}_scratch_bytes", len(m), N, beam, T, *host, V)
    for G, bdash in ((5, 1), (2, 2), (3, 2)):
        if len(m) == 1:
            show(name, f"G{G}_b{bdash} ", "acvae_dbs_search_scratch_bytes", N, G, bdash, T, *m[0], V)
        show(name, f"G{G}_b{bdash} ", "acvae_ensemble_dbs_search_scratch_bytes", len(m), N, G, bdash, T, *host, V)
