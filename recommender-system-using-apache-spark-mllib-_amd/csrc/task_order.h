// Launch-1 task order of the rank 33-64 explicit solve: which heavy-row chunk or
// light row workgroup t works on.  Plain C++ (the order test under tests/ builds a
// host program from it), __host__ __device__ under hipcc.
//
// The launch has two kinds of task.  Gram-heavy ones (heavy-row chunks: 4096
// ratings, no solve; long light rows) are bound by the factor-row gathers;
// solve-heavy ones (short light rows: a few Gram steps, then a full k x k LDL^T)
// by VALU issue.  Workgroups start in blockIdx order (observed, not a contract:
// only speed depends on it), so the order decides which tasks share a SIMD.
//
//   list A  the chunks in their order, then the first nA = ceil(f * n_light)
//           entries of the light list (the longest rows, longest first)
//   list B  the other light entries, longest first
//
// A is spread evenly through B without B's tail (its last floor(|B| / 8)
// entries, the shortest rows, which run after the merge in their order).  In the
// merged part of M tasks the shorter list m of the two is the one spread: task t
// takes m's next entry exactly when floor((t + 1) |m| / M) > floor(t |m| / M),
// else the other list's, so m entries before task t = floor(t |m| / M).  Both
// lists keep their LPT order and run out within one task of each other, m last.
//
// Tail.  A's last entry (the light row at the f-quantile of the length order, a
// chunk when nA = 0) starts when 1/8 of B's rows, the shortest, are still to
// come: at the ML-25M shape 7.3k item rows of <= 87 ratings (57 us alone) or
// 19.9k user rows of <= 51 ratings (103 us), against 10-20 us for the quantile
// row and ~40 us for a whole 4096-rating chunk.  Without that tail (A and B
// ending together) the user launch measured 0.96 -> 1.03 ms.  Worst case: fewer
// short rows than that behind a chunk-sized last A entry, i.e. one chunk's time.
//
// Measured (DESIGN.md K2 + K3, profiles/r08/task_order.md): the even spread is
// periodic, and a stride |M| / |A| with a small multiple near 256 (one block per
// CU) puts A on the same CUs over and over: f = 1/4 at the ML-25M item shape
// (stride 3.556 = 256 / 72) 0.89 -> 1.03 ms.  f = 1/16 gives strides 8.75 (item)
// and 14.12 (user) there.
//
// |A| = 0 or an empty merged B give the plain list: chunks, then light rows.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define ALS_TASK_HD __host__ __device__ __forceinline__
#else
#define ALS_TASK_HD inline
#endif

namespace als {

// f = kTaskSplitNum / kTaskSplitDen: the share of the light list that joins the
// chunks in list A; 1 / kTaskTailDen: the share of list B, its shortest rows, that
// runs after the merge on its own (0: none).  (Macros: the A/B variants of the sweep.)
#ifndef ALS_TASK_SPLIT_NUM
#define ALS_TASK_SPLIT_NUM 1
#endif
#ifndef ALS_TASK_SPLIT_DEN
#define ALS_TASK_SPLIT_DEN 16
#endif
#ifndef ALS_TASK_TAIL_DEN
#define ALS_TASK_TAIL_DEN 8
#endif
constexpr int kTaskSplitNum = ALS_TASK_SPLIT_NUM;
constexpr int kTaskSplitDen = ALS_TASK_SPLIT_DEN;
constexpr int kTaskTailDen = ALS_TASK_TAIL_DEN;
static_assert(kTaskSplitNum >= 0 && kTaskSplitNum <= kTaskSplitDen && kTaskSplitDen >= 1 &&
                  kTaskSplitDen <= 1024 && kTaskTailDen >= 0 && kTaskTailDen <= 1024,
              "0 <= f <= 1");

// Light entries in list A: ceil(f * n_light).
ALS_TASK_HD int task_order_n_a_light(int n_light) {
  return (int)(((int64_t)n_light * kTaskSplitNum + kTaskSplitDen - 1) / kTaskSplitDen);
}

// Entries of list B (n_b of them) that run after the merge: floor(n_b / kTaskTailDen).
ALS_TASK_HD int task_order_n_tail(int n_b) { return kTaskTailDen > 0 ? n_b / kTaskTailDen : 0; }

// Task t in [0, n_chunks + n_light) -> chunk (light = -1) or position in the light
// list (chunk = -1).  n_chunks + n_light < 2^31; the products need 64 bits.
ALS_TASK_HD void decode_task_merged(int t, int n_chunks, int n_light, int& chunk, int& light) {
  const int n_a_light = task_order_n_a_light(n_light);
  const uint64_t a = (uint64_t)n_chunks + (uint64_t)n_a_light;
  // the merged part: all of A and B without its tail
  const uint64_t n = a + (uint64_t)(n_light - n_a_light - task_order_n_tail(n_light - n_a_light));
  chunk = -1;
  light = -1;
  if ((uint64_t)t >= n) {  // B's tail, in its order
    light = t - n_chunks;
    return;
  }
  // the shorter list m is the one spread: its entries close their strides, so the merge's
  // last task is m's last entry and the one before it the other list's (|A| <= |B|: m = A)
  const bool a_short = 2 * a <= n;
  const uint64_t m = a_short ? a : n - a;
  const uint64_t tm = (uint64_t)t * m;
  const uint64_t im = tm / n;  // m entries before task t
  // floor((t + 1) m / n) > im  <=>  the remainder of t m / n plus m reaches n
  const bool take_m = tm - im * n + m >= n;
  const uint64_t ia = a_short ? im : (uint64_t)t - im;  // A entries before task t
  const bool take_a = take_m == a_short;
  if (take_a) {
    if (ia < (uint64_t)n_chunks) chunk = (int)ia;
    else light = (int)ia - n_chunks;
  } else {
    light = n_a_light + (t - (int)ia);
  }
}

}  // namespace als
