"""Host reference of the encoders' device-drawn dropout, written from the definition (helper module, no tests).

The rule (include/acvae_hip.h at acvae_bn_relu_pool_fwd, DESIGN.md "Device-drawn dropout"):
  * element e of a site's STORED output - flat index in NHWC order of the pooled / output tensor, n*C + c for the two head
    sites - belongs to quad q = e >> 2;
  * r = Philox4x32-10(key = (seed lo, seed hi), counter = (lo32(q), hi32(q), site, 0x5eed5eed));
  * the element uses word e & 3 of r and is kept iff float32(word >> 8) * 2^-24 >= float32(p).

Everything is numpy uint64 arithmetic masked to 32 bits; nothing here reads the kernels' sources.
"""
import numpy as np

_U = np.uint64
_M32 = _U(0xFFFFFFFF)
_S32 = _U(32)
PHILOX_M0, PHILOX_M1 = _U(0xD2511F53), _U(0xCD9E8D57)       # Salmon et al., "Parallel random numbers: as easy as 1, 2, 3"
PHILOX_W0, PHILOX_W1 = _U(0x9E3779B9), _U(0xBB67AE85)
DROPOUT_TAG = 0x5EED5EED                                    # counter word 3 of every dropout draw


def _u32(x):
    return np.asarray(x, dtype=np.uint64) & _M32


def philox4x32_10(key0, key1, c0, c1, c2, c3):
    """Philox4x32 with ten rounds, vectorised over the counters.  Returns the four output words as uint32 arrays."""
    k0, k1 = _u32(key0), _u32(key1)
    c0, c1, c2, c3 = np.broadcast_arrays(_u32(c0), _u32(c1), _u32(c2), _u32(c3))
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2             # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _M32, (p0 >> _S32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + PHILOX_W0) & _M32, (k1 + PHILOX_W1) & _M32
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def quad_words(seed, site, quads):
    """The Philox block of each dropout quad: uint32 [len(quads), 4]."""
    seed = int(seed)
    q = np.asarray(quads, dtype=np.uint64)
    return np.stack(philox4x32_10(seed & 0xFFFFFFFF, seed >> 32, q & _M32, q >> _S32, int(site), DROPOUT_TAG), axis=-1)


def keep_decision(words, p):
    """keep iff float32(word >> 8) * 2^-24 >= float32(p): p reaches the kernel as a C float."""
    v = (np.asarray(words, dtype=np.uint32) >> np.uint32(8)).astype(np.float32)      # 24 bits: exact
    return v * np.float32(2.0 ** -24) >= np.float32(p)


def element_words(seed, site, e):
    """The 32-bit word of each element index e (any shape)."""
    e = np.asarray(e, dtype=np.uint64)
    quads, inverse = np.unique(e >> _U(2), return_inverse=True)
    w = quad_words(seed, site, quads)
    return w[inverse.reshape(e.shape), (e & _U(3)).astype(np.intp)]


def keep_mask_nhwc(seed, site, p, shape_nhwc):
    """bool keep-mask of a site in its stored order (any shape: NHWC for the 4-D sites, [N, C] for the head sites)."""
    n = int(np.prod(shape_nhwc))
    w = quad_words(seed, site, np.arange((n + 3) // 4, dtype=np.uint64)).reshape(-1)[:n]
    return keep_decision(w, p).reshape(shape_nhwc)


def keep_mask_nchw(seed, site, p, shape_nchw):
    """The same mask in [N, C, H, W] order: the layout of `dropout_masks` and of the kernels' keep_mask argument."""
    N, C, H, W = shape_nchw
    return np.ascontiguousarray(keep_mask_nhwc(seed, site, p, (N, H, W, C)).transpose(0, 3, 1, 2))


def keep_mask_rows(seed, site, p, shape_nc):
    """[N, C] mask of a head site (element n*C + c)."""
    N, C = shape_nc
    return keep_mask_nhwc(seed, site, p, (N, C))


# ------------------------------------------------------------------------------------------------ the cases of the GPU file
# (tests/test_dropout_philox_gpu.py runs them; tests/test_philox_ref_cpu.py shows on the host that each wrong rule changes
# the mask at each of them)
SEED_HI = 0x1E3779B9F74A7C15          # non-zero high half, bit 31 of the low half set
SEED_BASE = 1234                      # a _seed_base; the kernel-level seed is what the encoders' _next_seed() makes of it
ENCODER_SEED_BASE = 0x1E3779B9F74A    # the _seed_base of the encoder-level runs: its seeds have a non-zero high half, which
                                      # the two head sites (reachable through an encoder only) would otherwise never see
SITES = (0, 5, 20)
PROBS = (0.1, 0.2, 0.5)
# (N, H, W, C, pool) of the kernel's INPUT; the stored tensor is [N, H/2, W/2, C] (pool) or [N, H, W, C]
SMALL_SHAPES = [(3, 10, 6, 64, 1), (2, 7, 5, 128, 1), (3, 6, 4, 512, 1), (2, 4, 4, 2048, 1), (2, 5, 2, 2048, 0)]
# more quads (2 359 296) than one pass of the element-wise grid (8192 blocks x 256 threads = 2 097 152)
WRAP_SHAPES = [(9, 32, 32, 1024, 0), (9, 64, 64, 1024, 1)]
# A draw whose 24-bit value is exactly 2^23 = 0.5 * 2^24: kept under `>=` at p = 0.5, dropped under `>`.  Found with
# find_boundary_draw() below over SEED_HI + k; tests/test_philox_ref_cpu.py re-derives the hit.
PLANT_SEED, PLANT_SITE, PLANT_QUAD, PLANT_WORD = 0x1E3779B9F74A7C2A, 20, 1509, 0          # = SEED_HI + 21
PLANT_SHAPE = (2, 8, 6, 256, 1)       # stored [2, 4, 3, 256]: element 4 * 1509 + 0 = 6036 is (n 1, ho 3, wo 2, c 148)
# the kernel-level cases: every small shape through a pool and through dropout alone (the issue's own pairings among them)
KERNEL_CASES = sorted({(n, h, w, c, pl) for n, h, w, c, _ in SMALL_SHAPES for pl in (0, 1)})
PLANT_CASES = [PLANT_SHAPE, (2, 4, 3, 256, 0)]             # the same stored tensor behind a pool and behind dropout alone
WRAP_DRAW = (SEED_HI, 5, 0.2)                              # the one (seed, site, p) of the wrap shapes
# p of each dropout site in forward order: ConvBlock sites p_block = 0.2 (0.1 inside ResNet38's residual blocks), the two head
# sites p_fc = 0.5
ENCODER_SITE_PROBS = {"Cnn10": [0.2] * 4 + [0.5] * 2, "Cnn14_16k": [0.2] * 6 + [0.5] * 2,
                      "ResNet38": [0.2] + [0.1] * 16 + [0.2, 0.2, 0.5, 0.5]}


def stored_shape(N, H, W, C, pool):
    return (N, H // 2, W // 2, C) if pool else (N, H, W, C)


def find_boundary_draw(seeds, sites=SITES, max_quads=65536, value=1 << 23):
    """First (seed, site, quad, word) whose 24-bit value equals `value` (offline search for the PLANT_* constants)."""
    q = np.arange(max_quads, dtype=np.uint64)
    for seed in seeds:
        for site in sites:
            hit = np.argwhere((quad_words(seed, site, q) >> np.uint32(8)) == np.uint32(value))
            if len(hit):
                return int(seed), int(site), int(hit[0][0]), int(hit[0][1])
    return None
