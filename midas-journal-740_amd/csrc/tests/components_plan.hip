// Host-only check of the numbering's block plan of the surface components (cuberille_internal.h: comp_scan_plan,
// comp_scan_bytes): for point counts around every size at which the plan takes another shape -- one block, one more than a
// block, a level more, 2^32 - 2 -- the levels cover each other, lie back to back, the top one fits one block, and the plan of a
// smaller count fits inside the plan of a larger one (a blind launch sizes the row for the larger and runs on the smaller).
// Touches no device.  SANITIZE="-Xarch_host -fsanitize=address,undefined" builds it for a sanitizer run.
#include <cstdio>
#include <vector>

#include "../cuberille_internal.h"

using namespace cuberille;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s (nP = %llu)\n", __LINE__, #cond, (unsigned long long)nP); failures++; } } while (0)

static void check(u64 nP) {
  const CompScanPlan p = comp_scan_plan(nP);
  CHECK(p.levels >= 1 && p.levels <= 8);
  u64 below = nP;
  size_t at = 0;
  for (int l = 0; l < p.levels; l++) {
    const u64 want = (below + COMP_SCAN_B - 1) / COMP_SCAN_B;
    CHECK(p.len[l] == want);                      // one entry per block of the level below
    CHECK(p.off[l] == at);                        // back to back
    at += p.len[l];
    below = want;
  }
  CHECK(p.entries == at);
  CHECK(p.len[p.levels - 1] <= (size_t)COMP_SCAN_B);                             // the top level: one block
  CHECK(p.levels == 1 || p.len[p.levels - 2] > (size_t)COMP_SCAN_B);             // ... and no level too many
  CHECK(comp_scan_bytes(nP) == sizeof(u64) + p.entries * sizeof(u32));
  // the levels as a vector: every entry of every level is inside the row
  std::vector<u32> row(p.entries + 2, 0);
  for (int l = 0; l < p.levels; l++)
    if (p.len[l]) { row[p.off[l]] += 1; row[p.off[l] + p.len[l] - 1] += 1; }
  // a smaller count on this plan's offsets (the blind launch): each of its levels is no longer than this plan's
  for (u64 real : {(u64)0, nP / 3, nP - (nP ? 1 : 0), nP}) {
    u64 n = real;
    for (int l = 0; l < p.levels; l++) {
      n = (n + COMP_SCAN_B - 1) / COMP_SCAN_B;
      CHECK(n <= p.len[l]);
    }
    CHECK(n <= (u64)COMP_SCAN_B);
  }
}

int main() {
  const u64 B = COMP_SCAN_B;
  const u64 sizes[] = {0, 1, 2, B - 1, B, B + 1, 2 * B, B * B - 1, B * B, B * B + 1, 131071, 131072, B * B * B - 1, B * B * B,
                       B * B * B + 1, 11100000, 249000000, 0xfffffffeULL};
  for (u64 nP : sizes) check(nP);
  if (failures) { std::printf("components_plan: %d failures\n", failures); return 1; }
  std::printf("components_plan ok\n");
  return 0;
}
