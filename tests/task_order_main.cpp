// Stand-alone check of csrc/task_order.h (built and run by test_task_order_cpu.py):
// t -> (chunk | light position) is a bijection onto {chunks} u {light rows}, each list
// keeps its order, list A is spread evenly through the merged part, where both lists
// run out together, and list B's tail follows in its order.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "task_order.h"

static int fails = 0;
#define CHECK(c, ...)                       \
  do {                                      \
    if (!(c)) {                             \
      if (++fails <= 20) {                  \
        std::printf("FAIL %s: ", #c);       \
        std::printf(__VA_ARGS__);           \
        std::printf("\n");                  \
      }                                     \
    }                                       \
  } while (0)

// Every t of the launch.
static void check_full(int n_chunks, int n_light) {
  const int64_t n = (int64_t)n_chunks + n_light;
  const int n_al = als::task_order_n_a_light(n_light);
  const int64_t a = (int64_t)n_chunks + n_al;
  const int64_t n_tail = als::task_order_n_tail((int)(n - a));
  const int64_t nm = n - n_tail;  // the merged part: A and B without its tail
  const int64_t b = nm - a;       // B's entries in the merged part
  CHECK(n_tail >= 0 && n_tail <= n - a, "tail %lld of %lld", (long long)n_tail, (long long)(n - a));
  CHECK(n_al >= 0 && n_al <= n_light, "nA %d of %d", n_al, n_light);
  CHECK(n_al == 0 ||
            ((int64_t)n_al * als::kTaskSplitDen >= (int64_t)n_light * als::kTaskSplitNum &&
             (int64_t)(n_al - 1) * als::kTaskSplitDen < (int64_t)n_light * als::kTaskSplitNum),
        "nA %d is not ceil(f * %d)", n_al, n_light);
  std::vector<unsigned char> seen_c(n_chunks, 0), seen_l(n_light, 0);
  int64_t next_a = 0, next_b = 0;   // entries of each list taken so far
  int64_t last_a = -1;              // task of the last A entry
  int64_t first_done_a = -1, first_done_b = -1;
  const int64_t window = a > 0 ? (nm + a - 1) / a + 1 : 0;
  for (int64_t t = 0; t < n; ++t) {
    int chunk = -7, light = -7;
    als::decode_task_merged((int)t, n_chunks, n_light, chunk, light);
    CHECK((chunk >= 0) != (light >= 0) && chunk >= -1 && light >= -1, "(%d,%d) t=%lld: %d %d",
          n_chunks, n_light, (long long)t, chunk, light);
    bool in_a;
    int64_t pos;  // position in its list
    if (chunk >= 0) {
      CHECK(chunk < n_chunks, "(%d,%d) t=%lld chunk %d", n_chunks, n_light, (long long)t, chunk);
      if (chunk >= n_chunks) return;
      CHECK(!seen_c[chunk], "(%d,%d) chunk %d twice", n_chunks, n_light, chunk);
      seen_c[chunk] = 1;
      in_a = true;
      pos = chunk;
    } else {
      CHECK(light >= 0 && light < n_light, "(%d,%d) t=%lld light %d", n_chunks, n_light,
            (long long)t, light);
      if (light < 0 || light >= n_light) return;
      CHECK(!seen_l[light], "(%d,%d) light %d twice", n_chunks, n_light, light);
      seen_l[light] = 1;
      in_a = light < n_al;
      pos = in_a ? (int64_t)n_chunks + light : light - n_al;
    }
    // each list in its original order: the next entry of that list, nothing skipped
    if (in_a) {
      CHECK(pos == next_a, "(%d,%d) t=%lld A order %lld != %lld", n_chunks, n_light, (long long)t,
            (long long)pos, (long long)next_a);
      ++next_a;
      CHECK(t - last_a <= window, "(%d,%d) no A entry in tasks (%lld, %lld)", n_chunks, n_light,
            (long long)last_a, (long long)t);
      last_a = t;
    } else {
      CHECK(pos == next_b, "(%d,%d) t=%lld B order %lld != %lld", n_chunks, n_light, (long long)t,
            (long long)pos, (long long)next_b);
      ++next_b;
      if (t >= nm) CHECK(light == t - n_chunks, "(%d,%d) t=%lld tail", n_chunks, n_light, (long long)t);
    }
    if (t >= nm) CHECK(!in_a, "(%d,%d) t=%lld: an A entry in the tail", n_chunks, n_light, (long long)t);
    if (next_a == a && first_done_a < 0) first_done_a = t;
    if (next_b == b && first_done_b < 0) first_done_b = t;
  }
  CHECK(next_a == a && next_b == b + n_tail, "(%d,%d) counts", n_chunks, n_light);
  if (a > 0) CHECK(nm - last_a <= window, "(%d,%d) no A entry at the end", n_chunks, n_light);
  if (a > 0 && b > 0) {  // exhausted within one task of each other
    const int64_t d = first_done_a - first_done_b;
    CHECK(d == 1 || d == -1, "(%d,%d) lists end %lld tasks apart", n_chunks, n_light, (long long)d);
  }
  if (a > 0 && b > 0) CHECK(std::max(first_done_a, first_done_b) == nm - 1, "(%d,%d) merge end", n_chunks, n_light);
  if (a == 0 || b == 0) {  // the plain list: chunks, then light rows
    for (int64_t t = 0; t < n; ++t) {
      int chunk, light;
      als::decode_task_merged((int)t, n_chunks, n_light, chunk, light);
      CHECK(t < n_chunks ? (chunk == t && light == -1) : (chunk == -1 && light == t - n_chunks),
            "(%d,%d) plain list t=%lld", n_chunks, n_light, (long long)t);
    }
  }
}

// Sampled t of a launch too large to enumerate: task t's entry is the one the closed
// form of the merge names (A entries before t = floor(t a / n), in 128-bit arithmetic),
// and t -> entry is strictly increasing within each list over neighbouring tasks.
static void check_sampled(int n_chunks, int n_light) {
  const int64_t n = (int64_t)n_chunks + n_light;
  const int n_al = als::task_order_n_a_light(n_light);
  const int64_t a = (int64_t)n_chunks + n_al;
  const int64_t n_all = n;
  const int64_t nm = n_all - als::task_order_n_tail((int)(n_all - a));
  std::vector<int64_t> ts;
  for (int64_t t = 0; t < 4096; ++t) {
    ts.push_back(t);
    ts.push_back(n - 1 - t);
    ts.push_back(n / 2 + t);
    if (nm - 1 - t >= 0) ts.push_back(nm - 1 - t);
    if (nm + t < n) ts.push_back(nm + t);
  }
  uint64_t s = 0x9e3779b97f4a7c15ull;
  for (int i = 0; i < 200000; ++i) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    ts.push_back((int64_t)((s >> 11) % (uint64_t)n));
  }
  for (int64_t t : ts) {
    int chunk = -7, light = -7;
    als::decode_task_merged((int)t, n_chunks, n_light, chunk, light);
    // the shorter list is the one spread by the floor rule, over the merged part
    const bool a_short = 2 * a <= nm;
    const unsigned __int128 m = a_short ? a : nm - a;
    const int64_t im = (int64_t)((unsigned __int128)t * m / (unsigned __int128)nm);
    const int64_t im1 = (int64_t)((unsigned __int128)(t + 1) * m / (unsigned __int128)nm);
    const int64_t ia = a_short ? im : t - im;
    const bool take_a = (im1 > im) == a_short;
    int want_c = -1, want_l = -1;
    if (t >= nm) {
      want_l = (int)(t - n_chunks);
    } else if (take_a) {
      if (ia < n_chunks) want_c = (int)ia;
      else want_l = (int)(ia - n_chunks);
    } else {
      want_l = (int)(n_al + (t - ia));
    }
    CHECK(chunk == want_c && light == want_l, "(%d,%d) t=%lld: %d %d, want %d %d", n_chunks,
          n_light, (long long)t, chunk, light, want_c, want_l);
    CHECK(chunk < n_chunks && light < n_light, "(%d,%d) t=%lld out of range", n_chunks, n_light,
          (long long)t);
  }
  // both ends: the first task opens a list, the merge's last two tasks close A and B's
  // merged part, the launch's last task is the last light row
  int c0, l0, c1, l1, c2, l2, c3, l3;
  als::decode_task_merged(0, n_chunks, n_light, c0, l0);
  als::decode_task_merged((int)(nm - 1), n_chunks, n_light, c1, l1);
  als::decode_task_merged((int)(nm - 2), n_chunks, n_light, c2, l2);
  als::decode_task_merged((int)(n - 1), n_chunks, n_light, c3, l3);
  CHECK(c0 == -1 ? (l0 == 0 || l0 == n_al) : c0 == 0, "first task %d %d", c0, l0);
  const int last_a_c = n_al == 0 ? n_chunks - 1 : -1, last_a_l = n_al == 0 ? -1 : n_al - 1;
  const int last_b_l = (int)(nm - n_chunks - 1);
  const bool last_two = (c1 == last_a_c && l1 == last_a_l && c2 == -1 && l2 == last_b_l) ||
                        (c2 == last_a_c && l2 == last_a_l && c1 == -1 && l1 == last_b_l);
  if (a > 0 && nm > a) CHECK(last_two, "merge's last tasks %d %d / %d %d", c2, l2, c1, l1);
  if (nm < n) CHECK(c3 == -1 && l3 == n_light - 1, "last task %d %d", c3, l3);
}

int main() {
  for (int c = 0; c <= 48; ++c)
    for (int l = 0; l <= 48; ++l) check_full(c, l);
  check_full(2532, 57518);
  check_full(0, 159097);
  check_full(338772, 946829);
  check_full(1, 0);
  check_full(0, 1);
  check_sampled(338772, 2147483647 - 338772);  // n_chunks + n_light = 2^31 - 1
  check_sampled(1500000000, 647483647);
  if (fails) {
    std::printf("%d checks failed\n", fails);
    return 1;
  }
  std::printf("task order ok (f = %d/%d, tail 1/%d)\n", als::kTaskSplitNum, als::kTaskSplitDen,
              als::kTaskTailDen);
  return 0;
}
