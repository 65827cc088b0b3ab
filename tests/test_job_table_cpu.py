"""CPU: the bounded job tables of the batched launches (acvae_amd/csrc/job_table.h).  A small C++ driver is built against the
header with ROCm's host compiler (no HIP): a table fills to its capacity, an add past it stores nothing and marks the table
not ok, and seal / find map every index of a range table to the job that owns it."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "acvae_amd", "csrc")
CXX = "/opt/rocm/llvm/bin/clang++"

DRIVER = r"""
#include <cstdio>
#include "job_table.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

struct Job { int id; long payload; };
struct Span { long size; };

// the table as the first member, so that a write past job[] would land in n or in the guard
template <class T> struct Guarded { T t; long guard = 0x5a5a5a5a; };

template <class Index, int MAX>
void check_ranges(const long* sizes, int count) {
  acvae::RangeTable<Span, MAX, Index> t;
  for (int l = 0; l < count; ++l) t.add({sizes[l]});
  CHECK(t.ok());
  long total = 0;
  for (int l = 0; l < count; ++l) total += sizes[l];
  CHECK(t.seal([](const Span& s) { return (Index)s.size; }) == (Index)total);
  CHECK(t.start[0] == 0 && t.start[count] == (Index)total);
  for (int l = 0; l < count; ++l) {
    CHECK(t.start[l + 1] - t.start[l] == (Index)sizes[l]);
    CHECK(t.find(t.start[l]) == l);                  // first index of the job
    CHECK(t.find(t.start[l + 1] - 1) == l);          // last index of the job
  }
  for (Index i = 0; i < (Index)total; ++i) {
    const int l = t.find(i);
    CHECK(l >= 0 && l < count && t.start[l] <= i && i < t.start[l + 1]);
  }
}

int main() {
  constexpr int MAX = 5;
  Guarded<acvae::JobTable<Job, MAX>> g;
  auto& t = g.t;
  CHECK(t.n == 0 && t.ok() && t.capacity == MAX);
  for (int k = 0; k < MAX; ++k) t.add({k, 100L + k});
  CHECK(t.n == MAX && t.ok());
  t.add({99, 999});                                  // one past the capacity
  CHECK(t.n == MAX + 1 && !t.ok());
  for (int k = 0; k < MAX; ++k) CHECK(t.job[k].id == k && t.job[k].payload == 100L + k);
  CHECK(g.guard == 0x5a5a5a5a);
  t.add({98, 998});
  CHECK(t.n == MAX + 2 && !t.ok() && t.job[MAX - 1].id == MAX - 1);

  Guarded<acvae::RangeTable<Span, 3>> r;
  for (int k = 0; k < 4; ++k) r.t.add({7});
  CHECK(r.t.n == 4 && !r.t.ok() && r.guard == 0x5a5a5a5a);

  const long mixed[] = {1, 5, 1, 3, 64, 1};          // jobs of size 1, the last one ending the range
  check_ranges<long, 6>(mixed, 6);                   // filled to capacity
  check_ranges<int, 8>(mixed, 6);
  const long ones[] = {1, 1, 1, 1};
  check_ranges<long, 4>(ones, 4);
  const long single[] = {9};
  check_ranges<int, 1>(single, 1);
  const long big[] = {1L << 33, 1};                  // 64-bit ranges (elements of a large table)
  acvae::RangeTable<Span, 2> b;
  b.add({big[0]}); b.add({big[1]});
  CHECK(b.seal([](const Span& s) { return s.size; }) == (1L << 33) + 1);
  CHECK(b.find(0) == 0 && b.find((1L << 33) - 1) == 0 && b.find(1L << 33) == 1);

  if (failures == 0) std::printf("ok\n");
  return failures == 0 ? 0 : 1;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not os.path.exists(CXX):
        pytest.fail(f"{CXX} not found: the ROCm host compiler is needed to build the job-table driver")
    d = tmp_path_factory.mktemp("job_table")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    r = subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return str(exe)


def test_job_table_bounds_and_range_lookup(driver):
    r = subprocess.run([driver], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr

