// Bounded job tables: the argument of every kernel that runs several small jobs in one launch.  Header-only and free of HIP,
// so that a plain C++ compiler builds it too (tests/test_job_table_cpu.py).
#pragma once
#ifdef __HIPCC__
#define ACVAE_HD __host__ __device__
#else
#define ACVAE_HD
#endif

namespace acvae {

// Up to MAX jobs, passed by value as a kernel argument.  add() counts every call but stores only what fits: n > MAX records an
// overflow, and every launcher refuses such a table (ok() false) before it makes any HIP call.
template <class Job, int MAX>
struct JobTable {
  static constexpr int capacity = MAX;
  Job job[MAX];
  int n = 0;
  void add(const Job& j) {
    if (n < MAX) job[n] = j;
    ++n;
  }
  ACVAE_HD bool ok() const { return n <= MAX; }
};

// Jobs that cover consecutive ranges of one flat index space (elements, tiles, blocks): job l owns [start[l], start[l + 1]).
template <class Job, int MAX, class Index = long>
struct RangeTable : JobTable<Job, MAX> {
  Index start[MAX + 1];
  // host, on a table that is ok(): fills start[] with the prefix sums of size(job) and returns the total
  template <class Size>
  Index seal(Size size) {
    start[0] = 0;
    for (int l = 0; l < this->n; ++l) start[l + 1] = start[l] + size(this->job[l]);
    return start[this->n];
  }
  // the job that owns index i (0 <= i < start[n])
  ACVAE_HD int find(Index i) const {
    int l = 0;
    while (l + 1 < this->n && i >= start[l + 1]) ++l;
    return l;
  }
};

}  // namespace acvae
