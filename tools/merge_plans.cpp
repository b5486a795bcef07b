// Host-only view of plan_merge (fenix_amd/csrc/knn_merge.hip): no GPU needed.
//
//   merge_plans grid    one line per (nq, lists, list length, k) of a grid:
//                       return code, then per level G and the dynamic LDS
//                       bytes run_merge asks for, then ws_bytes.  Built against
//                       two versions of the library, `diff` of the two
//                       outputs shows which plans a change to plan_merge moved.
//   merge_plans probe   the plans fx_code_probe makes: for code spaces of
//                       1 .. 64 lists of 4 096 (and the shapes named in
//                       tests/test_gpu_probe.py) and EVERY probes <= pmax, each
//                       level fits 160 KB and needs no more scratch than the
//                       plan at pmax, which is what probe_layout reserves.
//                       Prints the per-level (G, bytes) of the named shapes;
//                       exit status 1 on a violation.
//
// Build (after the library):
//   hipcc -std=c++17 -I include tools/merge_plans.cpp -o tools/_tmp_merge_plans \
//       -L fenix_amd/lib -lfenix_knn -Wl,-rpath,$PWD/fenix_amd/lib
#include <stdio.h>
#include <string.h>

#include "../fenix_amd/csrc/fx_internal.h"
#include "../fenix_amd/csrc/fx_select.h"

using fx::MergePlan;

static int64_t next_pow2(int64_t v) {
  int64_t p = 1;
  while (p < v) p <<= 1;
  return p;
}

// merge_kernel's carve-up of its dynamic LDS, restated (not shared with the
// library: an independent check of what plan_merge sized)
static size_t level_bytes(const MergePlan& p, int lv, int64_t k) {
  const int64_t P2 = next_pow2(k), rcap = P2 > k ? P2 : k;
  const int64_t in = p.group[lv] * p.klen[lv];
  return sizeof(fx::MergeShared) + (size_t)rcap * 8 + (size_t)(in > k ? in : k) * 8;
}

static void print_plan(int64_t nq, int64_t lists, int64_t kin, int64_t k) {
  MergePlan p;
  const int rc = fx::plan_merge(nq, lists, kin, k, &p);
  printf("nq=%lld lists=%lld kin=%lld k=%lld rc=%d", (long long)nq, (long long)lists,
         (long long)kin, (long long)k, rc);
  if (rc == 0) {
    for (int lv = 0; lv < p.levels; ++lv)
      printf(" L%d(lists=%lld G=%lld lds=%zu)", lv, (long long)p.lists[lv], (long long)p.group[lv],
             level_bytes(p, lv, k));
    printf(" ws=%zu", p.ws_bytes);
  }
  printf("\n");
}

static int grid() {
  const int64_t lists[] = {1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 33, 64, 100, 257, 1000, 4096};
  const int64_t kins[] = {1, 10, 64, 100, 128, 256, 1000, 1024, 2048, 4096, 6000, 8192, 8193};
  const int64_t ks[] = {1,    10,   64,   100,  128,  256,  500,  1000, 1024, 1025,
                        2047, 2048, 2049, 3000, 4096, 4097, 6000, 6077, 6078, 8192, 8193};
  for (int64_t nq : {1, 3})
    for (int64_t l : lists)
      for (int64_t kin : kins)
        for (int64_t k : ks) print_plan(nq, l, kin, k);
  return 0;
}

constexpr int64_t kProbeMerge = 4096;  // knn_code.hip
constexpr size_t kBudget = 160 * 1024;

// every probes <= pmax of one code space; returns the number of violations
static int probe_space(int64_t nq, int64_t C, bool show) {
  const int64_t kin = C < kProbeMerge ? C : kProbeMerge;
  const int64_t lists = (C + kin - 1) / kin, pmax = kin;
  MergePlan top;
  if (fx::plan_merge(nq, lists, kin, pmax, &top) != 0) {
    printf("C=%lld: plan at pmax refused: %s\n", (long long)C, fx::last_error());
    return 1;
  }
  int bad = 0;
  for (int64_t probes = 1; probes <= pmax; ++probes) {
    MergePlan p;
    if (fx::plan_merge(nq, lists, kin, probes, &p) != 0) {
      printf("C=%lld probes=%lld refused: %s\n", (long long)C, (long long)probes, fx::last_error());
      ++bad;
      continue;
    }
    if (p.ws_bytes > top.ws_bytes) {
      printf("C=%lld probes=%lld ws %zu > %zu reserved\n", (long long)C, (long long)probes,
             p.ws_bytes, top.ws_bytes);
      ++bad;
    }
    for (int lv = 0; lv < p.levels; ++lv)
      if (level_bytes(p, lv, probes) > kBudget) {
        printf("C=%lld probes=%lld level %d asks %zu > %zu\n", (long long)C, (long long)probes, lv,
               level_bytes(p, lv, probes), kBudget);
        ++bad;
      }
  }
  if (show)
    for (int64_t probes : {(int64_t)100, (int64_t)2048, (int64_t)2049, (int64_t)3000, pmax})
      if (probes <= pmax) print_plan(nq, lists, kin, probes);
  return bad;
}

static int probe() {
  int bad = 0;
  struct Shape { int nb; int64_t ks; };
  const Shape named[] = {{1, 5}, {2, 6}, {3, 5}, {2, 64}, {2, 100}, {2, 111}, {2, 128},
                         {2, 256}, {4, 16}, {3, 64}};
  for (const Shape& s : named) {
    int64_t C = 1;
    for (int j = 0; j < s.nb; ++j) C *= s.ks;
    printf("# (%d,%lld): C=%lld\n", s.nb, (long long)s.ks, (long long)C);
    for (int64_t nq : {1, 3}) bad += probe_space(nq, C, nq == 1);
  }
  // every list count up to 64, full and with a padded tail; small spaces too
  for (int64_t l = 1; l <= 64; ++l)
    for (int64_t C : {l * kProbeMerge, l * kProbeMerge - 1, (l - 1) * kProbeMerge + 1})
      bad += probe_space(2, C, false);
  for (int64_t C : {1, 2, 36, 125, 1000, 3200, 3201, 4095}) bad += probe_space(2, C, false);
  bad += probe_space(1, (int64_t)1 << 24, false);  // 4 096 lists
  printf("%d violations\n", bad);
  return bad ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && strcmp(argv[1], "grid") == 0) return grid();
  if (argc == 2 && strcmp(argv[1], "probe") == 0) return probe();
  fprintf(stderr, "usage: %s grid | probe\n", argv[0]);
  return 2;
}
