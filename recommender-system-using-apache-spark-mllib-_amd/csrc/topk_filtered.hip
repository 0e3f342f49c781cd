// K5 filtered — the RowFilter instantiations of the top-k sweep (FILT = true, reached
// through als_topk_filtered).  A translation unit of their own: the unfiltered kernels in
// topk.hip's object stay exactly what they were before the filter existed, and the two
// sets of 48 instantiations compile side by side.
#include "topk_sweep.h"

int als::topk_launch_filtered(const TkLaunch& a, const RowFilter& f) {
  return topk_launch_split(a, f);
}
