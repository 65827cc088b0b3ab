"""The host reference of the device-drawn dropout (tests/philox_ref.py) checked on its own, without a GPU:

  * the bare generator against known answers (two of them the published Random123 vectors of Philox4x32-10),
  * the keep decision at its edge,
  * the keep rate of every (seed, site, p) that tests/test_dropout_philox_gpu.py uses,
  * that sites and seeds select different streams,
  * and, for every shape of the GPU file, that each plausible wrong rule (a wrong counter, order, index, word order, site,
    seed half, comparison or channel-chunk offset) changes the mask - so the GPU file's equalities can fail for that
    error at that shape.
"""
import math
from types import SimpleNamespace

import numpy as np
import pytest

import philox_ref as R

U = np.uint64


# ------------------------------------------------------------------------------------------------ the generator
KNOWN = [
    ((0, 0), (0, 0, 0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),                       # Random123 kat_vectors
    ((0xFFFFFFFF,) * 2, (0xFFFFFFFF,) * 4, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0xA4093822, 0x299F31D0), (0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344),                     # Random123 kat_vectors
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("key,ctr,out", KNOWN)
def test_philox4x32_10_known_answers(key, ctr, out):
    got = tuple(int(w) for w in R.philox4x32_10(*key, *ctr))
    assert got == out, " ".join(f"{w:08x}" for w in got)


def test_philox_is_vectorised_over_counters():
    c0 = np.array([0, 0xFFFFFFFF, 0x243F6A88, 7], dtype=np.uint64)
    w = R.philox4x32_10(0xA4093822, 0x299F31D0, c0, 0x85A308D3, 0x13198A2E, 0x03707344)
    assert all(x.dtype == np.uint32 and x.shape == (4,) for x in w)
    assert tuple(int(x[2]) for x in w) == KNOWN[2][2]
    one = R.philox4x32_10(0xA4093822, 0x299F31D0, 7, 0x85A308D3, 0x13198A2E, 0x03707344)
    assert tuple(int(x[3]) for x in w) == tuple(int(x) for x in one)


def test_quad_words_put_the_quad_index_in_counter_words_0_and_1():
    q = (5 << 32) | 0x80000001                    # a quad index >= 2^32: counter word 1 carries its high half
    w = R.quad_words(R.SEED_HI, 5, [q])[0]
    ref = R.philox4x32_10(R.SEED_HI & 0xFFFFFFFF, R.SEED_HI >> 32, 0x80000001, 5, 5, 0x5EED5EED)
    assert [int(x) for x in w] == [int(x) for x in ref]


# ------------------------------------------------------------------------------------------------ the decision
def keep_of_value(v, p):
    return bool(R.keep_decision(np.uint32(v << 8), p))


def test_keep_decision_at_its_edge():
    assert keep_of_value(1 << 23, 0.5) and not keep_of_value((1 << 23) - 1, 0.5)
    first = {}
    for p in (0.2, 0.1):
        first[p] = math.ceil(float(np.float32(p)) * 2 ** 24)          # exact in a double: 24 bits times a power of two
        assert keep_of_value(first[p], p) and not keep_of_value(first[p] - 1, p), p
    assert first[0.2] == 3355444 and first[0.1] == 1677722
    # the low byte of a word takes no part; p = 0 keeps everything, the largest value is kept at every p used
    assert keep_of_value(0, 0.0) and all(keep_of_value((1 << 24) - 1, p) for p in R.PROBS)
    assert bool(R.keep_decision(np.uint32(((1 << 23) << 8) | 0xFF), 0.5)) and \
        not bool(R.keep_decision(np.uint32((((1 << 23) - 1) << 8) | 0xFF), 0.5))


def test_mask_layouts_agree():
    N, C, H, W = 2, 8, 3, 5
    a = R.keep_mask_nhwc(R.SEED_HI, 5, 0.2, (N, H, W, C))
    b = R.keep_mask_nchw(R.SEED_HI, 5, 0.2, (N, C, H, W))
    assert a.dtype == np.bool_ and b.shape == (N, C, H, W) and b.flags["C_CONTIGUOUS"]
    for n, c, h, w in [(0, 0, 0, 0), (1, 7, 2, 4), (1, 3, 1, 2), (0, 5, 2, 0)]:
        e = ((n * H + h) * W + w) * C + c
        word = R.quad_words(R.SEED_HI, 5, [e >> 2])[0][e & 3]
        assert a[n, h, w, c] == b[n, c, h, w] == bool(R.keep_decision(word, 0.2))
    rows = R.keep_mask_rows(R.SEED_HI, 20, 0.5, (3, 10))              # 30 elements: a trailing half quad
    assert rows.shape == (3, 10)
    assert np.array_equal(rows.reshape(-1), R.keep_mask_nhwc(R.SEED_HI, 20, 0.5, (32,))[:30])
    e = np.array([[0, 1, 2, 3], [29, 28, 4, 11]])
    assert np.array_equal(R.keep_decision(R.element_words(R.SEED_HI, 20, e), 0.5), rows.reshape(-1)[e])


# ------------------------------------------------------------------------------------------------ what the GPU file draws
def encoder_seeds(base=R.SEED_BASE):
    """The seeds of the first two forwards of an encoder with _seed_base = base, from the encoders' own method."""
    from acvae_amd.encoder import _PannsCnn
    mod = SimpleNamespace(_seed_base=base, _calls=0)
    return [_PannsCnn._next_seed(mod), _PannsCnn._next_seed(mod)]


def gpu_draws():
    """Every (seed, site, p) of tests/test_dropout_philox_gpu.py."""
    out = {(seed, site, p) for seed in (R.SEED_HI, encoder_seeds()[0]) for site in R.SITES for p in R.PROBS}
    out.add((R.PLANT_SEED, R.PLANT_SITE, 0.5))
    for probs in R.ENCODER_SITE_PROBS.values():
        out |= {(seed, site, p) for seed in encoder_seeds(R.ENCODER_SEED_BASE) for site, p in enumerate(probs)}
    return sorted(out)


def test_keep_rate_of_every_draw_the_gpu_tests_use():
    n = 1 << 18
    draws = gpu_draws()
    assert len(draws) > 60
    words = {}
    for seed, site, p in draws:
        if (seed, site) not in words:
            words[seed, site] = R.quad_words(seed, site, np.arange(n // 4, dtype=np.uint64)).reshape(-1)
        rate = float(R.keep_decision(words[seed, site], p).mean())
        bound = 4 * math.sqrt(p * (1 - p) / n)
        assert abs(rate - (1 - p)) <= bound, f"seed {seed:#x} site {site} p {p}: rate {rate:.5f}, bound {bound:.5f}"
    assert abs(float(R.keep_mask_nhwc(1234, 3, 0.2, (n,)).mean()) - 0.80060) < 1e-5


def test_sites_and_seeds_select_different_streams():
    shape = (2, 6, 4, 64)
    base = R.keep_mask_nhwc(R.SEED_HI, 0, 0.2, shape)
    assert np.array_equal(base, R.keep_mask_nhwc(R.SEED_HI, 0, 0.2, shape))
    assert not np.array_equal(base, R.keep_mask_nhwc(R.SEED_HI, 5, 0.2, shape))                  # two sites, one seed
    assert not np.array_equal(base, R.keep_mask_nhwc(encoder_seeds()[0], 0, 0.2, shape))         # two seeds, one site
    assert not np.array_equal(base, R.keep_mask_nhwc(R.SEED_HI ^ (1 << 40), 0, 0.2, shape))      # ... equal low halves
    assert not np.array_equal(base, R.keep_mask_nhwc(R.SEED_HI ^ 1, 0, 0.2, shape))
    s1, s2 = encoder_seeds()
    assert s1 != s2 and not np.array_equal(R.keep_mask_nhwc(s1, 0, 0.2, shape), R.keep_mask_nhwc(s2, 0, 0.2, shape))


def test_the_seeds_have_the_halves_the_cases_need():
    assert R.SEED_HI >> 32 and R.SEED_HI & 0x80000000
    assert R.PLANT_SEED >> 32 and R.PLANT_QUAD < 65536 and R.PLANT_SITE in R.SITES
    assert all(s >> 32 for s in encoder_seeds(R.ENCODER_SEED_BASE))


# ------------------------------------------------------------------------------------------------ the planted draw
def plant_element():
    return 4 * R.PLANT_QUAD + R.PLANT_WORD


def test_planted_draw_sits_on_the_boundary():
    w = R.quad_words(R.PLANT_SEED, R.PLANT_SITE, [R.PLANT_QUAD])[0][R.PLANT_WORD]
    assert int(w) >> 8 == 1 << 23
    e = plant_element()
    stored = R.stored_shape(*R.PLANT_SHAPE)
    assert e < int(np.prod(stored))
    assert R.keep_mask_nhwc(R.PLANT_SEED, R.PLANT_SITE, 0.5, stored).reshape(-1)[e]
    found = R.find_boundary_draw([R.PLANT_SEED], sites=[R.PLANT_SITE])
    assert found == (R.PLANT_SEED, R.PLANT_SITE, R.PLANT_QUAD, R.PLANT_WORD)


# ------------------------------------------------------------------------------------------------ mutants
def sample_elements(case):
    """Flat stored indices a mutant is judged on: all of a small shape; the first and the last 2^16 of a wrap shape (the last
    ones lie behind one pass of the grid stride)."""
    total = int(np.prod(R.stored_shape(*case)))
    if total <= 1 << 18:
        return np.arange(total, dtype=np.uint64)
    return np.concatenate([np.arange(1 << 16, dtype=np.uint64), np.arange(total - (1 << 16), total, dtype=np.uint64)])


def coords(case, idx):
    _, Ho, Wo, C = R.stored_shape(*case)
    c = idx % U(C); t = idx // U(C)
    wo = t % U(Wo); t = t // U(Wo)
    return t // U(Ho), t % U(Ho), wo, c                      # n, ho, wo, c


def decide(seed, site, e, p):
    return R.keep_decision(R.element_words(seed, site, e), p)


def m_counter_is_element(case, seed, site, p, idx):
    return R.keep_decision(R.quad_words(seed, site, idx)[np.arange(len(idx)), (idx & U(3)).astype(np.intp)], p)


def m_order_nchw(case, seed, site, p, idx):
    _, Ho, Wo, C = R.stored_shape(*case)
    n, ho, wo, c = coords(case, idx)
    return decide(seed, site, ((n * U(C) + c) * U(Ho) + ho) * U(Wo) + wo, p)


def m_unpooled_index(case, seed, site, p, idx):
    N, H, W, C, pool = case
    n, ho, wo, c = coords(case, idx)
    return decide(seed, site, ((n * U(H) + U(2) * ho) * U(W) + U(2) * wo) * U(C) + c, p)


def m_words_reversed(case, seed, site, p, idx):
    return R.keep_decision(R.quad_words(seed, site, idx >> U(2))[np.arange(len(idx)), (U(3) - (idx & U(3))).astype(np.intp)], p)


def m_next_site(case, seed, site, p, idx):
    return decide(seed, site + 1, idx, p)


def m_seed_low_half(case, seed, site, p, idx):
    return decide(seed & 0xFFFFFFFF, site, idx, p)


def m_chunk_offset_dropped(case, seed, site, p, idx):
    C = case[3]
    n, ho, wo, c = coords(case, idx)
    return decide(seed, site, idx - c + c % U(1024), p)


def m_greater_than(case, seed, site, p, idx):
    v = (R.element_words(seed, site, idx) >> np.uint32(8)).astype(np.float32)
    return v * np.float32(2.0 ** -24) > np.float32(p)


def gpu_shapes():
    """Every (N, H, W, C, pool) whose stored tensor the GPU file draws."""
    assert set(R.SMALL_SHAPES) <= set(R.KERNEL_CASES)
    return sorted(set(R.KERNEL_CASES + R.WRAP_SHAPES + R.PLANT_CASES))


@pytest.mark.parametrize("case", gpu_shapes(), ids=lambda c: "x".join(map(str, c[:4])) + f"-p{c[4]}")
def test_every_wrong_rule_changes_the_mask_at_every_gpu_shape(case):
    N, H, W, C, pool = case
    idx = sample_elements(case)
    small = len(idx) <= 1 << 16
    for seed in (R.SEED_HI, encoder_seeds()[0]) if small else R.WRAP_DRAW[:1]:
        for site in R.SITES if small else R.WRAP_DRAW[1:2]:
            for p in R.PROBS if small else R.WRAP_DRAW[2:]:
                ref = decide(seed, site, idx, p)
                if small:
                    assert np.array_equal(ref, R.keep_mask_nhwc(seed, site, p, R.stored_shape(*case)).reshape(-1))
                mutants = [m_counter_is_element, m_order_nchw, m_words_reversed, m_next_site]
                if pool:
                    mutants.append(m_unpooled_index)
                if seed >> 32:
                    mutants.append(m_seed_low_half)
                if C == 2048:
                    mutants.append(m_chunk_offset_dropped)
                for m in mutants:
                    assert not np.array_equal(ref, m(case, seed, site, p, idx)), (m.__name__, hex(seed), site, p)


def test_greater_than_differs_exactly_at_the_planted_draw():
    case = R.PLANT_SHAPE
    idx = sample_elements(case)
    ref = decide(R.PLANT_SEED, R.PLANT_SITE, idx, 0.5)
    mut = m_greater_than(case, R.PLANT_SEED, R.PLANT_SITE, 0.5, idx)
    diff = np.flatnonzero(ref != mut)
    assert plant_element() in diff and ref[plant_element()] and not mut[plant_element()]
    # the other wrong rules change this mask too
    for m in (m_counter_is_element, m_order_nchw, m_unpooled_index, m_words_reversed, m_next_site, m_seed_low_half):
        assert not np.array_equal(ref, m(case, R.PLANT_SEED, R.PLANT_SITE, 0.5, idx)), m.__name__
