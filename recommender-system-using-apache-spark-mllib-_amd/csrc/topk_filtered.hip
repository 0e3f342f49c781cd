// K5 filtered — the FILT = true instantiations of the top-k sweep (topk_split_filt_kernel,
// reached through als_topk_filtered).  A translation unit of their own: the unfiltered
// kernels in topk.hip's object stay exactly what they were before the filter existed,
// and the two sets of 48 instantiations compile side by side.
#define ALS_TOPK_FILTERED_TU 1
#include "topk.hip"
