"""Write tests/golden/augment_ref.npz: the reference's own training-time transforms (datasets/augment.py random_crop,
time_roll, spec_augment), in the order utils/train_util.py:parse_augments builds them, run over synthetic clips.

CPU only.  The reference's augment module is imported from its checkout at run time (``--reference``, or the
ACVAE_REFERENCE_ROOT environment variable); only its outputs are stored.  The clips are not stored: they are
regenerated from ``clip_seed`` (``clips()`` below; tests/test_augment_cpu.py restates it and checks ``clip_sums``).

Per config ``c``: ``c{c}_config`` (JSON: the augments list, or the keyword arguments of a direct spec_augment call),
``c{c}_seed`` (``random.seed`` / ``np.random.seed`` before the first clip), the reference's output for clip i (clips in
order) and ``c{c}_next_random`` / ``c{c}_next_np`` (the next ``random.random()`` / ``np.random.random()`` after the
last clip).

An output is stored losslessly relative to its input clip, which keeps the file small: ``c{c}_src{i}`` (int16, per
output row the clip row it was taken from: the reference only crops and rolls rows), ``c{c}_exc{i}`` (np.packbits of
the row-major map of cells that differ from that clip row: the masked cells) and ``c{c}_val{i}`` (float32, their values
in row-major order).  ``decode()`` below rebuilds the output bit for bit; tests/test_augment_cpu.py restates it.

Seeds are searched from ``c{c}_seed`` upwards until the run exercises what the config is there for (a crop that
fires, masks on some clips and not on others).

    python tools/make_augment_golden.py --reference <reference checkout>
"""
import argparse
import importlib
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "augment_ref.npz")
CLIP_SEED = 20261015
LENGTHS = (35, 999, 1000, 1001, 1500)
F = 64


def clips(seed=CLIP_SEED, lengths=LENGTHS, F=F):
    """Log-mel-like float32 clips (values on a 1/4 grid)."""
    rs = np.random.RandomState(seed)
    return [(np.round(rs.randn(L, F) * 4.0) / 4.0 - 4.0).astype(np.float32) for L in lengths]


CONFIGS = [
    ("list", [], lambda outs, cl: True),
    ("list", ["timemask", "freqmask"],
     lambda outs, cl: any(o.shape == c.shape and not np.array_equal(o, c) for o, c in zip(outs, cl)) and
     any(np.array_equal(o, c) for o, c in zip(outs, cl))),
    ("list", ["randomcrop", "timeroll", "timemask", "freqmask"],
     lambda outs, cl: any(len(o) == 1000 and len(c) > 1000 for o, c in zip(outs, cl))),
    ("list", ["timeroll", "randomcrop", "freqmask"],
     lambda outs, cl: any(len(o) == 1000 and len(c) > 1000 for o, c in zip(outs, cl))),
    ("spec_augment", dict(p=1.0, num_timemask=4, num_freqmask=4), lambda outs, cl: True),
]


def encode(out, clip):
    """(src, exc bits, values) of ``out`` relative to ``clip`` (see the module docstring).  ``src`` is, per output row,
    the clip row that agrees with it in the most cells; any choice decodes exactly, this one makes ``exc`` small."""
    src = np.empty(len(out), dtype=np.int16)
    for a in range(0, len(out), 128):
        eq = (out[a:a + 128, None, :] == clip[None, :, :]).sum(axis=2)
        src[a:a + 128] = eq.argmax(axis=1)
    exc = out != clip[src.astype(np.int64)]
    return src, np.packbits(exc.reshape(-1)), out[exc].astype(np.float32)


def decode(src, bits, vals, clip):
    out = clip[src.astype(np.int64)].copy()
    exc = np.unpackbits(bits)[:out.size].astype(bool).reshape(out.shape)
    out[exc] = vals
    return out


def transforms(aug, kind, cfg):
    if kind == "spec_augment":
        return [aug.spec_augment(**cfg)]
    kw = {"timemask": False, "freqmask": False, "timewarp": False}      # utils/train_util.py:parse_augments
    ts = []
    for name in cfg:
        if name in kw:
            kw[name] = True
        elif name == "randomcrop":
            ts.append(aug.random_crop)
        elif name == "timeroll":
            ts.append(aug.time_roll)
    return ts + [aug.spec_augment(**kw)]


def run(aug, kind, cfg, seed, cl):
    random.seed(seed)
    np.random.seed(seed)
    ts = transforms(aug, kind, cfg)
    outs = []
    for c in cl:
        x = c
        for t in ts:
            x = t(x)
        outs.append(np.asarray(x, dtype=np.float32))
    return outs, random.random(), np.random.random()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", default=os.environ.get("ACVAE_REFERENCE_ROOT"),
                    help="the reference checkout (default: $ACVAE_REFERENCE_ROOT)")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    if not args.reference or not os.path.isdir(os.path.join(args.reference, "datasets")):
        ap.error("--reference must name the reference checkout (the directory holding datasets/augment.py)")
    sys.path.insert(0, os.path.abspath(args.reference))
    aug = importlib.import_module("datasets.augment")

    cl = clips()
    data = {"clip_seed": np.int64(CLIP_SEED), "lengths": np.array(LENGTHS, dtype=np.int64), "F": np.int64(F),
            "clip_sums": np.array([float(c.astype(np.float64).sum()) for c in cl])}
    for k, (kind, cfg, wanted) in enumerate(CONFIGS):
        seed = 1000 * (k + 1)
        while True:
            outs, nr, nn = run(aug, kind, cfg, seed, cl)
            if wanted(outs, cl):
                break
            seed += 1
        data[f"c{k}_config"] = np.array(json.dumps({"kind": kind, "config": cfg}))
        data[f"c{k}_seed"] = np.int64(seed)
        data[f"c{k}_next_random"] = np.float64(nr)
        data[f"c{k}_next_np"] = np.float64(nn)
        for i, (o, c) in enumerate(zip(outs, cl)):
            src, bits, vals = encode(o, c)
            assert np.array_equal(decode(src, bits, vals, c).view(np.uint32), o.view(np.uint32))
            data[f"c{k}_src{i}"], data[f"c{k}_exc{i}"], data[f"c{k}_val{i}"] = src, bits, vals
        print(f"config {k} {kind} {cfg}: seed {seed}, output lengths {[len(o) for o in outs]}")
    np.savez_compressed(args.out, **data)
    print(f"{args.out}: {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
