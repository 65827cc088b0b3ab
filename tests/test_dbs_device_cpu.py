"""CPU: the one-call diverse beam search without a GPU - the numpy twin of its bookkeeping (tests/dbs_util.py) against a
naive list-of-hypotheses search on random score tables, the header's new entries, their refusal codes and scratch
arithmetic (host code: nothing is launched), and Ensemble's acceptance of method="dbs" up to the first device call."""
import ctypes

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import dbs_util as D
from acvae_amd import _lib
from test_ensemble_cpu import cpu_model

EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -3, -4
END = 2


def tables(seed, N, G, bdash, T, V, end_logp=None, step=0.25):
    """logp[g][lt] f32 [R, V]: multiples of `step` from a small set, so that sums tie often and the fp64 keys c / (lt + 1)
    tie too (2 * 0.25 / 2 == 0.25 / 1).  end_logp: the <end> column, per group (None: as drawn)."""
    rng = np.random.default_rng(seed)
    R = N * bdash
    logp = [[(-step * rng.integers(1, 9, size=(R, V))).astype(np.float32) for _ in range(T)] for _ in range(G)]
    if end_logp is not None:
        for g in range(G):
            if end_logp[g] is not None:
                for lt in range(T):
                    logp[g][lt][:, END] = np.float32(end_logp[g])
    return logp


def both(logp, N, G, bdash, T, V, lam, group_nbest):
    want = D.naive_search(logp, N, G, bdash, T, V, lam, group_nbest, END)
    got, tabs = D.table_search(logp, N, G, bdash, T, V, lam, group_nbest, END)
    for a, b, what in zip(got, want, ("seqs", "scores", "lengths")):
        assert a.shape == b.shape and a.dtype == b.dtype, what
        assert np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a,
                              b.view(np.int64) if b.dtype == np.float64 else b), what
    return got, tabs


@pytest.mark.parametrize("N,G,bdash,T,V,lam", [(2, 2, 2, 5, 7, 0.5), (3, 3, 2, 6, 9, 0.75), (1, 1, 16, 4, 40, 0.5),
                                               (2, 5, 1, 6, 6, 0.25), (1, 16, 1, 3, 5, 1.0), (2, 2, 3, 1, 8, 0.5)])
@pytest.mark.parametrize("group_nbest", [True, False])
def test_twin_vs_naive_search_on_random_tables(N, G, bdash, T, V, lam, group_nbest):
    for seed in range(3):
        both(tables(seed, N, G, bdash, T, V), N, G, bdash, T, V, lam, group_nbest)


def test_twin_vs_naive_with_planted_ties_in_the_fp64_score():
    """First every word at -0.25: all scores of a step tie and the lower flat index decides.  Then <end> at -0.25 and every
    other word at -0.25 or below: a row that ends at step lt after best words only has c = -0.25 * (lt + 1), so records of
    different lengths share the key -0.25 exactly and the order of recording decides among them."""
    N, G, bdash, T, V = 2, 2, 3, 5, 6
    logp = [[np.full((N * bdash, V), -0.25, np.float32) for _ in range(T)] for _ in range(G)]
    both(logp, N, G, bdash, T, V, 0.0, True)                    # every score of a step ties: the lower index decides
    both(logp, N, G, bdash, T, V, 0.5, False)
    logp = tables(5, N, G, bdash, T, V, end_logp=[-0.25, -0.25])
    for g in range(G):
        for lt in range(T):
            logp[g][lt][:, :] = np.minimum(logp[g][lt], np.float32(-0.25))
            logp[g][lt][:, END] = np.float32(-0.25)
    (seqs, scores, lengths), (par_tab, word_tab, rec) = both(logp, N, G, bdash, T, V, 0.0, True)
    assert len(np.unique(lengths)) > 1                          # records of several lengths were ranked against each other
    keys = [np.float64(rec[0, lt, r]) / (lt + 1) for lt in range(T) for r in range(bdash) if rec[0, lt, r] == rec[0, lt, r]]
    assert len(keys) > len(set(keys))                           # and some of their fp64 keys are equal


def test_twin_vs_naive_rows_that_end_twice():
    """A retired row (c - 1000) loses to every child of a live row, so it is expanded again only once all rows of its group
    have retired.  <end> is out of reach at lt = 0, where all other words tie, and the best word by far from then on: at
    lt = 1 every row emits <end> and retires, and from lt = 2 on retired rows are expanded, emit <end> and are recorded again."""
    for bdash in (1, 2, 3):
        N, G, T, V = 2, 2, 6, 7
        logp = tables(7, N, G, bdash, T, V, end_logp=[-0.125, -0.125])
        for g in range(G):
            logp[g][0][:, :] = np.float32(-0.25)
            logp[g][0][:, END] = np.float32(-1.0e4)
        (seqs, scores, lengths), (par_tab, word_tab, rec) = both(logp, N, G, bdash, T, V, 0.0, True)
        twice = 0
        for g in range(G):
            for lt in range(1, T):
                for r in range(N * bdash):
                    p = par_tab[g, lt, r]
                    twice += int(rec[g, lt, r] == rec[g, lt, r] and rec[g, lt - 1, p] == rec[g, lt - 1, p])
        assert twice > 0, bdash
        assert (rec[rec == rec] < -900).any()                   # a record below -900: made by a retired row
        both(logp, N, G, bdash, T, V, 0.5, False)


def test_twin_vs_naive_groups_where_only_the_last_step_records():
    """<end> is out of reach for group 1 (and free for group 0): group 1's records all come from lt = T - 1."""
    N, G, bdash, T, V = 3, 2, 3, 5, 8
    logp = tables(9, N, G, bdash, T, V, end_logp=[-0.25, -1.0e4])
    (seqs, scores, lengths), (par_tab, word_tab, rec) = both(logp, N, G, bdash, T, V, 0.5, True)
    assert not (rec[1, :T - 1] == rec[1, :T - 1]).any() and (rec[1, T - 1] == rec[1, T - 1]).all()
    assert (lengths[:, bdash:] == T).all() and (lengths[:, :bdash] < T).any()


def test_advance_and_dense_counts_by_hand():
    c = np.array([-1.5, -2.0, -0.5], np.float32)
    par, word, rec, after = D.advance(c, [1, 0, 2], [4, END, 7], END, last=False)
    assert par.dtype == word.dtype == np.int32 and par.tolist() == [1, 0, 2] and word.tolist() == [4, END, 7]
    assert np.isnan(rec[0]) and rec[1] == np.float32(-2.0) and np.isnan(rec[2])
    assert after.tolist() == [-1.5, -1002.0, -0.5]
    _, _, rec, after = D.advance(c, [1, 0, 2], [4, END, 7], END, last=True)
    assert rec.tolist() == c.tolist() and after.tolist() == [-1001.5, -1002.0, -1000.5]
    # one clip, bdash 2, T 3: group 0 has run steps 0..2; beam 0 at step 2 descends from row 1, row 1 at step 1 from row 0
    par_tab = np.zeros((2, 3, 2), np.int32)
    word_tab = np.zeros((2, 3, 2), np.int32)
    word_tab[0, 0] = [5, 6]
    par_tab[0, 1] = [0, 0]
    par_tab[0, 2] = [1, 1]
    # group 1 at lt = 0 sees group 0 after its step 1: both rows descend from row 0 -> word 5 twice
    assert D.dense_counts(par_tab, word_tab, 1, 2, 3, 8, 1, 0)[0].tolist() == [0, 0, 0, 0, 0, 2, 0, 0]
    par_tab[0, 1] = [1, 0]
    # now row 0 of step 1 descends from row 1 (word 6), row 1 from row 0 (word 5)
    assert D.dense_counts(par_tab, word_tab, 1, 2, 3, 8, 1, 0)[0].tolist() == [0, 0, 0, 0, 0, 1, 1, 0]
    # group 1 at lt = 1 (t = 2) sees group 0 after its step 2, whose rows both descend from row 1 of step 1
    word_tab[0, 1] = [3, 4]
    assert D.dense_counts(par_tab, word_tab, 1, 2, 3, 8, 1, 1)[0].tolist() == [0, 0, 0, 0, 2, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ the library
NEW = {"acvae_dbs_scores_sparse": 16, "acvae_dbs_advance": 10, "acvae_dbs_finish": 13, "acvae_dbs_search_scratch_bytes": 9,
       "acvae_dbs_search": 24, "acvae_ensemble_dbs_search_scratch_bytes": 10, "acvae_ensemble_dbs_search": 25}


def test_header_declares_the_new_entries_and_the_library_exports_them():
    ge.build()
    lib = _lib.lib()
    for name, n_args in NEW.items():
        assert name in _lib.PROTOS and hasattr(lib, name), name
        ret, args = _lib.PROTOS[name]
        assert len(args) == n_args, (name, len(args))
        assert ret is (ctypes.c_int64 if name.endswith("_bytes") else ctypes.c_int)
        assert getattr(lib, name).argtypes == [t for _, t in args]
    assert lib.acvae_abi_version() == 3 and int(_lib._defs["ACVAE_ABI_VERSION"]) == 3
    names = dict(_lib.PROTOS["acvae_dbs_search"][1])
    assert names["temperature"] is ctypes.c_float and names["diversity_lambda"] is ctypes.c_float
    assert names["scores"] is ctypes.c_void_p and names["scratch_bytes"] is ctypes.c_int64


class Args:
    """A well-formed argument set (fake non-null device pointers: every case below is refused before any launch)."""

    def __init__(self, M=2, N=3, G=2, bdash=2, T=6, V=50):
        self.M, self.N, self.G, self.bdash, self.T, self.V = M, N, G, bdash, T, V
        self.start, self.end = 1, 2
        self.temperature, self.lam, self.nbest = 1.0, 0.5, 1
        self.S = np.full(M, 4, np.int32)
        self.E = np.full(M, 64, np.int32)
        self.H = np.full(M, 64, np.int32)
        self.A = np.full(M, 64, np.int32)
        self.tab = (ctypes.c_void_p * M)(*([0x1000] * M))
        self.params = self.mem = self.lens = self.eps = ctypes.cast(self.tab, ctypes.c_void_p).value
        self.seqs = self.scores = self.lengths = self.scratch = 0x1000
        self.scratch_bytes = None

    def dims(self):
        return [a.ctypes.data for a in (self.S, self.E, self.H, self.A)]

    def ens_bytes(self):
        return _lib.lib().acvae_ensemble_dbs_search_scratch_bytes(self.M, self.N, self.G, self.bdash, self.T, *self.dims(), self.V)

    def one_bytes(self):
        return _lib.lib().acvae_dbs_search_scratch_bytes(self.N, self.G, self.bdash, self.T, 4, 64, 64, 64, self.V)

    def ens(self):
        sb = self.ens_bytes() if self.scratch_bytes is None else self.scratch_bytes
        return _lib.lib().acvae_ensemble_dbs_search(self.params, self.mem, self.lens, self.eps, *self.dims(), self.M, self.start,
                                                    self.end, self.N, self.G, self.bdash, self.T, self.V, self.temperature,
                                                    self.lam, self.nbest, self.seqs, self.scores, self.lengths, self.scratch, sb,
                                                    None)

    def one(self):
        sb = self.one_bytes() if self.scratch_bytes is None else self.scratch_bytes
        return _lib.lib().acvae_dbs_search(0x1000, 0x1000, 0x1000, 0x1000, self.start, self.end, self.N, self.G, self.bdash, self.T,
                                           4, 64, 64, 64, self.V, self.temperature, self.lam, self.nbest, self.seqs, self.scores,
                                           self.lengths, self.scratch, sb, None)


def test_refusals_and_scratch_arithmetic_of_both_entries():
    ge.build()
    for call in ("one", "ens"):
        def code(**kw):
            a = Args()
            for k, v in kw.items():
                setattr(a, k, v)
            return getattr(a, call)()
        assert code(G=17) == EUNSUPPORTED and code(bdash=17) == EUNSUPPORTED
        assert code(N=(1 << 20) // 2 + 1) == EUNSUPPORTED
        for k in ("N", "G", "bdash", "T"):
            assert code(**{k: 0}) == EINVAL, k
        assert code(start=-1) == EINVAL and code(start=50) == EINVAL and code(end=-1) == EINVAL and code(end=50) == EINVAL
        assert code(temperature=0.0) == EINVAL and code(temperature=float("nan")) == EINVAL
        assert code(lam=float("inf")) == EINVAL
        for k in ("seqs", "scores", "lengths", "scratch"):
            assert code(**{k: None}) == EINVAL, k
        a = Args()
        sb = getattr(a, call + "_bytes")()
        assert sb > 0 and code(scratch_bytes=sb - 1) == EWORKSPACE
    assert Args(M=1).ens_bytes() == Args(M=1).one_bytes()           # one driver: the single-model entry is its M = 1 case
    assert Args(M=2).ens_bytes() > Args(M=1).ens_bytes()            # a second member's states, and the mix rows
    assert Args(G=17).one_bytes() == -1 and Args(bdash=17).ens_bytes() == -1
    a = Args()
    a.tab[1] = None
    assert a.ens() == EINVAL                                          # a NULL entry of a member table
    assert Args(M=9).ens_bytes() == -1
    grow = [Args(M=1, G=g).one_bytes() for g in (1, 2, 3)]
    assert grow[0] < grow[1] < grow[2]                                # every group keeps its own states and tables
    lib = _lib.lib()
    assert lib.acvae_dbs_scores_sparse(0x1000, 50, 1.0, 0.5, None, 0x1000, None, None, 3, 2, 6, 50, 2, 1, 0, None) == EINVAL
    assert lib.acvae_dbs_scores_sparse(0x1000, 50, 1.0, 0.5, None, 0x1000, 0x1000, 0x1000, 3, 17, 6, 50, 2, 1, 0, None) == EUNSUPPORTED
    assert lib.acvae_dbs_scores_sparse(0x1000, 50, 1.0, 0.5, None, 0x1000, 0x1000, 0x1000, 3, 2, 6, 50, 2, 2, 0, None) == EINVAL
    assert lib.acvae_dbs_scores_sparse(0x1000, 50, 1.0, 0.5, None, 0x1000, 0x1000, 0x1000, 3, 2, 6, 50, 2, 1, 6, None) == EINVAL
    assert lib.acvae_dbs_advance(None, 0x1000, 0x1000, 0x1000, 0x1000, 0x1000, 2, 0, 4, None) == EINVAL
    assert lib.acvae_dbs_finish(0x1000, 0x1000, 0x1000, 0x1000, 0x1000, None, 3, 2, 2, 6, 1, 2, None) == EINVAL
    assert lib.acvae_dbs_finish(0x1000, 0x1000, 0x1000, 0x1000, 0x1000, 0x1000, 3, 17, 2, 6, 1, 2, None) == EUNSUPPORTED


# ------------------------------------------------------------------------------------------------ the Python side
def test_ensemble_accepts_dbs_up_to_the_first_device_call():
    from acvae_amd.ensemble import Ensemble
    ens = Ensemble([cpu_model(1), cpu_model(2, embed=128)])
    feats, fl = torch.zeros(1, 64, 64), np.array([64])
    with pytest.raises(RuntimeError, match="no CPU fallback"):        # every check passed; the tensors are not on a device
        ens(feats, fl, method="dbs", beam_size=4, group_size=2, diversity_lambda=0.7, temperature=1.5, group_nbest=False)
    with pytest.raises(ValueError, match="1..16"):
        ens(feats, fl, method="dbs", beam_size=2, group_size=3)
    with pytest.raises(ValueError, match="1..16"):
        ens(feats, fl, method="dbs", beam_size=34, group_size=2)
    with pytest.raises(ValueError, match="at most 16"):
        ens(feats, fl, method="dbs", beam_size=17, group_size=17)
    with pytest.raises(ValueError, match="temperature"):
        ens(feats, fl, method="dbs", temperature=0.0)
    with pytest.raises(ValueError):                                   # the decoding constraints stay refused with "dbs"
        ens(feats, fl, method="dbs", no_repeat_ngram_size=2)
    with pytest.raises(ValueError):
        ens(feats, fl, method="dbs", finish_on_end=True)
    with pytest.raises(ValueError, match="method"):
        ens(feats, fl, method="sample")


def test_model_keyword_dbs_impl():
    m = cpu_model(1)
    assert hasattr(m, "diverse_beam_search_host")
    with pytest.raises(ValueError, match="dbs_impl"):
        m.diverse_beam_search({}, 6, 4, 2, 0.5, 1.0, True, dbs_impl="graph")
    with pytest.raises(ValueError, match="1..16"):
        m.diverse_beam_search({}, 6, 34, 2, 0.5, 1.0, True)


# ------------------------------------------------------------------------------------------------ the rules as plain C++
CXX = "/opt/rocm/llvm/bin/clang++"
DRIVER = r"""
// The kernels' shared rules (csrc/dbs_rules.h) run serially on the host: finish, the penalty's counts, advance.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "dbs_rules.h"
namespace D = acvae::dbs;

template <class T> std::vector<T> rd(FILE* f, size_t n) {
  std::vector<T> v(n);
  if (n && std::fread(v.data(), sizeof(T), n, f) != n) { std::puts("short input"); std::exit(2); }
  return v;
}
template <class T> void wr(FILE* f, const std::vector<T>& v) { if (!v.empty()) std::fwrite(v.data(), sizeof(T), v.size(), f); }

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = std::fopen(argv[1], "rb");
  FILE* out = std::fopen(argv[2], "wb");
  if (!in || !out) return 2;
  const std::vector<int> h = rd<int>(in, 7);
  const int N = h[0], G = h[1], bdash = h[2], T = h[3], V = h[4], keep = h[5], end_idx = h[6], R = N * bdash;
  const size_t n_tab = (size_t)G * T * R;
  const std::vector<int> par = rd<int>(in, n_tab), word = rd<int>(in, n_tab);
  const std::vector<float> rec = rd<float>(in, n_tab);
  std::vector<float> c = rd<float>(in, 2 * (size_t)R);           // advance: [last = 0 | last = 1][R]
  const std::vector<int64_t> aword = rd<int64_t>(in, R);

  // finish, as dbs_finish_kernel does it with one lane
  const int rows = G * keep;
  std::vector<int64_t> seqs((size_t)N * rows * T, -9);
  std::vector<double> scores((size_t)N * rows, 0.0);
  std::vector<int> lengths((size_t)N * rows, -9);
  for (int n = 0; n < N; ++n)
    for (int g = 0; g < G; ++g) {
      std::vector<int> sel;
      for (int q = 0; q < keep; ++q) {
        double bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int i = 0; i < T * bdash; ++i) {
          const int lt = D::cand_step(i, bdash);
          const float fv = rec[D::at(g, lt, D::cand_row(i, bdash, n), T, R)];
          if (!D::is_record(fv)) continue;
          bool taken = false;
          for (int p : sel) taken = taken || p == i;
          const double v = D::key(fv, lt);
          if (!taken && D::better(v, i, bv, bi)) { bv = v; bi = i; }
        }
        sel.push_back(bi == 0x7fffffff ? -1 : bi);
        const int i = sel.back();
        const int t0 = i < 0 ? -1 : D::cand_step(i, bdash);
        const long r = i < 0 ? 0 : D::cand_row(i, bdash, n);
        const long o = D::out_row(n, g, q, G, keep);
        scores[o] = i < 0 ? -INFINITY : D::key(rec[D::at(g, t0, r, T, R)], t0);
        lengths[o] = t0 + 1;
        D::trace(par.data(), word.data(), g, t0, r, T, R, end_idx, seqs.data() + o * T);
      }
    }
  wr(out, seqs); wr(out, scores); wr(out, lengths);

  // the penalty's counts for every (g, lt), as dbs_scores_sparse_kernel lists and counts them: [G][T][N][V]
  std::vector<float> counts((size_t)G * T * N * V, 0.f);
  for (int g = 0; g < G; ++g)
    for (int lt = 0; lt < T; ++lt)
      for (int n = 0; n < N; ++n) {
        std::vector<int> lw(g * bdash);
        for (int i = 0; i < g * bdash; ++i)
          lw[i] = D::column_word(par.data(), word.data(), i / bdash, g, lt, (long)n * bdash + i % bdash, T, R);
        for (int i = 0; i < g * bdash; ++i) {
          bool first;
          const int mult = D::multiplicity(lw.data(), g * bdash, i, &first);
          if (first && lw[i] >= 0 && lw[i] < V) counts[(((size_t)g * T + lt) * N + n) * V + lw[i]] = (float)mult;
        }
      }
  wr(out, counts);

  // advance
  std::vector<float> arec(2 * (size_t)R);
  for (int last = 0; last < 2; ++last)
    for (int r = 0; r < R; ++r) {
      float& v = c[(size_t)last * R + r];
      const bool ends = D::recorded(aword[r], end_idx, last);
      arec[(size_t)last * R + r] = ends ? v : D::no_record();
      if (ends) v = D::retired(v);
    }
  wr(out, arec); wr(out, c);
  std::fclose(in); std::fclose(out);
  std::puts("ok");
  return 0;
}
"""


@pytest.fixture(scope="module")
def rules_binary(tmp_path_factory):
    """csrc/dbs_rules.h built as plain C++ with the host compiler, address and undefined-behaviour sanitizers on."""
    import os
    import subprocess
    d = tmp_path_factory.mktemp("dbs_rules")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "acvae_amd", "csrc")
    r = subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", csrc, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


@pytest.mark.parametrize("N,G,bdash,T,V,group_nbest", [(3, 2, 3, 6, 9, 1), (2, 16, 1, 4, 5, 0), (1, 1, 16, 20, 40, 1),
                                                       (4, 3, 2, 1, 7, 1), (2, 5, 4, 33, 12, 0), (2, 16, 16, 3, 300, 1)])
def test_shared_rules_as_plain_cpp_vs_twin(rules_binary, tmp_path, N, G, bdash, T, V, group_nbest):
    import subprocess
    rng = np.random.default_rng(N * 1000 + G * 10 + bdash)
    R = N * bdash
    base = (np.arange(R) // bdash) * bdash
    par = (base[None, None, :] + rng.integers(0, bdash, size=(G, T, R))).astype(np.int32)
    par[0, :, 0] = [-3, R + 5][G % 2]                                   # a parent out of range is clamped, not followed
    word = rng.integers(0, min(V, 6), size=(G, T, R)).astype(np.int32)
    rec = np.full((G, T, R), D.NONE, np.float32)
    pick = rng.random((G, T, R))
    steps = np.arange(1, T + 1, dtype=np.float32)[None, :, None]
    rec = np.where(pick < 0.4, -0.5 * steps, rec).astype(np.float32)                      # fp64 keys that tie
    rec = np.where((pick >= 0.4) & (pick < 0.5), rng.standard_normal((G, T, R)) - 1000, rec).astype(np.float32)
    rec[:, T - 1, :] = (rng.standard_normal((G, R)) * 2 - 3 - 2 * T).astype(np.float32)
    rec[0, T - 1, 0] = -np.inf
    c = (rng.standard_normal(R) * 4).astype(np.float32)
    aword = rng.integers(0, 4, size=R).astype(np.int64)
    keep = bdash if group_nbest else 1
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(np.array([N, G, bdash, T, V, keep, END], np.int32).tobytes())
        for a in (par, word, rec, np.concatenate([c, c]), aword):
            fh.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([str(rules_binary), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
    raw = open(tmp_path / "out.bin", "rb").read()
    rows, off = G * keep, 0

    def take(dtype, shape):
        nonlocal off
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        a = np.frombuffer(raw[off:off + n], dtype).reshape(shape)
        off += n
        return a
    seqs, scores, lengths = take(np.int64, (N, rows, T)), take(np.float64, (N, rows)), take(np.int32, (N, rows))
    counts = take(np.float32, (G, T, N, V))
    arec, after = take(np.float32, (2, R)), take(np.float32, (2, R))
    assert off == len(raw)
    want = D.finish(par, word, rec, N, G, bdash, T, group_nbest, END)
    assert np.array_equal(seqs, want[0]) and np.array_equal(scores.view(np.int64), want[1].view(np.int64))
    assert np.array_equal(lengths, want[2])
    for g in range(G):
        for lt in range(T):
            assert np.array_equal(counts[g, lt], D.dense_counts(par, word, N, bdash, T, V, g, lt)), (g, lt)
    for last in (0, 1):
        _, _, w_rec, w_after = D.advance(c, np.zeros(R, np.int64), aword, END, last)
        assert np.array_equal(np.isnan(arec[last]), np.isnan(w_rec))
        assert np.array_equal(np.nan_to_num(arec[last]).view(np.int32), np.nan_to_num(w_rec).view(np.int32))
        assert np.array_equal(after[last].view(np.int32), w_after.view(np.int32))
