/*
 * als_hip.h — C ABI of libals_hip.so, the MI355X (gfx950) ALS hot path.
 *
 * This is the drop-in boundary for the ALS path of
 * amy-leaf/Recommender-System-using-Apache-Spark-MLlib-.  The reference calls
 * the ALS core through pyspark (RecommenderSystem.py:132 import,
 * :148-149 / :163 / :218 `ALS.train`, :150 / :165 / :222 / :232 `predictAll`);
 * the arithmetic behind those calls lives in Apache Spark
 * (`ml/recommendation/ALS.scala`, not vendored).  Each entry point below
 * replaces one upstream routine on that path; the comment names it and the
 * reference call site that reaches it.
 *
 * Conventions
 *  - Every pointer except the `*_host` ones is DEVICE memory owned by the caller.
 *    The library never allocates on a compute call; scratch comes from a
 *    caller-provided workspace sized by the matching *_workspace_bytes().
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream).
 *    All compute calls are asynchronous on that stream.
 *  - Factor matrices are row-major fp32 with leading dimension `ld`
 *    (ld % 4 == 0, ld >= k, base 16-byte aligned).  Output factor rows are
 *    written in full: columns [k, ld) are written as zero, and factor inputs
 *    (Y_src of als_solve_half / als_yty) must carry zeros there too.
 *  - Return value: 0 on success, negative ALS_E* code on argument error;
 *    als_last_error() returns a thread-local message for the last failure.
 *  - Dense indices: ids are mapped to dense row numbers in ascending id order
 *    (als_index_build), the device analogue of Spark's sorted InBlock.srcIds.
 */
#ifndef ALS_HIP_H
#define ALS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ALS_ABI_VERSION 9

#define ALS_OK 0
#define ALS_EINVAL (-1)   /* bad argument (shape, null pointer, rank) */
#define ALS_EWORKSPACE (-2) /* workspace too small */
#define ALS_EDEVICE (-3)  /* HIP runtime error (launch failure, no device) */
#define ALS_EUNSUPPORTED (-4)

/* ---- library ---------------------------------------------------------- */
int als_abi_version(void);
const char* als_last_error(void);
/* Number of HIP devices visible (0 on a host without a GPU); never launches work. */
int als_device_count(void);

/* ---- K1: rating-block construction (replaces Spark partitionRatings /
 *      makeBlocks / InBlock / LocalIndexEncoder, reached from ALS.train at
 *      RecommenderSystem.py:148-149) ------------------------------------ */

/* Dense id map.  ids[n] in [0, id_space).  Writes map_out[id_space]
 * (dense index or -1 if the id does not occur), uniq_out[<=id_space]
 * (ascending distinct ids) and *n_uniq_dev (device int32). */
size_t als_index_workspace_bytes(int64_t n, int32_t id_space);
int als_index_build(const int32_t* ids, int64_t n, int32_t id_space,
                    int32_t* map_out, int32_t* uniq_out, int32_t* n_uniq_dev,
                    void* ws, size_t ws_bytes, void* stream);

/* Stable counting sort of a COO rating list by dense row (row = row_map[row_ids[e]]),
 * producing CSR: row_ptr_out[n_rows+1] (int64), col_out[nnz] = col_map[col_ids[e]]
 * and val_out[nnz] in input order within each row (Spark keeps duplicates:
 * each (u,i) occurrence is its own term, Appendix A.1).  nnz < 2^31. */
size_t als_csr_workspace_bytes(int64_t nnz, int32_t n_rows);
int als_csr_build(const int32_t* row_ids, const int32_t* row_map,
                  const int32_t* col_ids, const int32_t* col_map,
                  const float* vals, int64_t nnz, int32_t n_rows,
                  int64_t* row_ptr_out, int32_t* col_out, float* val_out,
                  void* ws, size_t ws_bytes, void* stream);

/* Work schedule for one CSR side: rows with <= chunk ratings ("light") are
 * solved one wavefront each, longest first; heavier rows are split into
 * chunk-sized tasks whose partial normal equations (fp32 sums within a task,
 * stored as those fp32 values) are summed in fp64 and solved in a second launch.  Two-step: count (device int32[3] = n_light, n_heavy,
 * n_chunks) then build into caller buffers sized from those counts. */
size_t als_schedule_workspace_bytes(int32_t n_rows);
int als_schedule_count(const int64_t* row_ptr, int32_t n_rows, int32_t chunk,
                       int32_t* counts_dev, void* stream);
int als_schedule_build(const int64_t* row_ptr, int32_t n_rows, int32_t chunk,
                       int32_t n_light, int32_t n_heavy, int32_t n_chunks,
                       int32_t* light_rows, int32_t* heavy_rows,
                       int32_t* heavy_slot_begin /* n_heavy+1 */,
                       int32_t* chunk_row, int64_t* chunk_begin, int64_t* chunk_end,
                       void* ws, size_t ws_bytes, void* stream);

/* ---- K2/K3: normal equations + Cholesky (replaces Spark computeFactors,
 *      NormalEquation.add (dspr/daxpy), CholeskySolver.solve (dppsv)) ---- */

/* One half-sweep: for every dst row j (all rows of the schedule)
 *   explicit:  A_j = sum_s y_s y_s^T + reg*n_j*I,          b_j = sum_s r_js y_s
 *   implicit:  A_j = YtY + sum_s c1 y_s y_s^T + reg*n+_j*I, b_j = sum_{r>0} (1+c1) y_s,
 *              c1 = alpha*|r|, n+_j = #{r_js > 0}
 * from fp32 factors.  The Gram runs on the f16 matrix cores with every value
 * split into two f16 halves (hi*hi + hi*lo + lo*hi: ~2^-21 relative per product)
 * after a power-of-two scaling set by max |Y_src| over its n_src rows and
 * max |rating|.  Explicit: Y_src is split once per call into a table in the
 * workspace ((n_src + 1) x k_pad words) and the rhs runs on the matrix cores too;
 * implicit: the split follows the per-rating confidence weight, in registers.
 * fp32 sums within a task (the schedule's chunk: engine.chunk_for picks 4096
 * ratings, 16384 for explicit fits at k > 64), fp64 across a heavy row's tasks;
 * solved by a square-root-free block LDL^T (the solution of Spark's Cholesky
 * dppsv) in fp32, stored fp32 into X_dst[row*ld ..].  k <= 128, n_src < 2^31.
 * Parity bar: 1e-4 relative per row against the fp64 restatement of Spark's
 * dspr + dppsv (oracle/); the measured maxima per configuration (ranks 1-128,
 * explicit/implicit, full-size half-sweeps) are in DESIGN.md section 1 and
 * tests/test_gpu_kernels.py / test_gpu_configs.py.  yty_packed (implicit only): lower-packed
 * fp64 k_pad x k_pad Gram from als_yty.  status_dev: device int32, set to
 * (row+1) of a row whose Cholesky pivot was not positive (0 = all rows ok;
 * Spark raises from dppsv in that case).  ws: 16-byte aligned.
 * phases (ALS_PHASE_* bits below; ALS_PHASE_ALL = the normal call): PREP = Y_src
 * prep (max |Y_src|; explicit: the split table), RSCALE = rating scale (max
 * |rating| of this block), LAUNCH1 = heavy-row chunk partials + fused primal
 * light-row gram/solve, DUAL = the dual-path light rows (see n_light_primal),
 * LAUNCH2 = heavy-row reduce + solve, RESCUE = re-solve of the rows that missed
 * the split window (below).  They run in the order PREP, RSCALE, LAUNCH1, DUAL,
 * LAUNCH2, RESCUE; split across calls, issue them in that order on one stream
 * with the same workspace (PREP starts an empty rescue list; RESCUE empties it
 * again, so every LAUNCH1 ... RESCUE sequence needs its RESCUE).  Blocks that share Y_src (row chunks of one half-sweep) may share
 * one PREP: it sits at a fixed workspace offset (size the workspace for the
 * largest n_chunks and n_rows).
 * Split window (explicit): the Gram/rhs split uses one power-of-two scale per
 * launch, so a row whose own factor rows (or ratings) all sit more than ~2^18
 * below the launch maxima would lose precision in the f16 lo halves.  Such a row
 * is detected in its task (max diagonal of its Gram / max |rating| against the
 * window) and re-solved in the RESCUE launch with a scale of its own (fp32 rows
 * split in registers, fp32 rhs), so the 1e-4 bar holds for any magnitude spread.
 * n_light_primal (0 <= n_light_primal <= n_light): the first n_light_primal light
 * rows are solved on the k x k normal equations above; the remaining light rows
 * (the tail of the longest-first light list) must have <= 96 ratings (64 < k <= 128)
 * or <= 32 ratings (32 < k <= 64) and are solved through the equivalent n x n dual
 * system (push-through identity (Y^T Y + lambda n I)^-1 Y^T r =
 * Y^T (Y Y^T + lambda n I)^-1 r), allowed for explicit feedback, 32 < k <= 128,
 * reg > 0 only (a longer row there is reported through status_dev).
 * n_light_primal = n_light keeps every row on the primal path.
 * Two-segment schedules (ABI 6; the sharded engine's pipelined item half-sweep,
 * distributed.py): chunk task c of this call writes partial slot chunk_slot0 + c,
 * and heavy_slot_begin2 (nullable, n_heavy + 1 entries) gives each heavy row a
 * second slot range, summed with the first in LAUNCH2.  A half-sweep whose source
 * rows arrive in two parts then runs as two calls on one workspace: the early
 * segments' chunk partials (PREP over the arrived prefix of Y_src, LAUNCH1,
 * chunk_slot0 = 0), then the late segments' (chunk_slot0 = number of early slots)
 * with LAUNCH2 and RESCUE over every row; the workspace is sized for all slots
 * (the slot region sits before the split table, so the two calls' different n_src
 * leave the early partials in place).  Normal calls pass NULL and 0. */
#define ALS_PHASE_LAUNCH1 1
#define ALS_PHASE_LAUNCH2 2
#define ALS_PHASE_PREP 4
#define ALS_PHASE_RSCALE 8
#define ALS_PHASE_DUAL 16
#define ALS_PHASE_RESCUE 32
#define ALS_PHASE_ALL 63
/* n_rows: rows of the block (n_light + n_heavy; the largest block when shared). */
size_t als_solve_workspace_bytes(int32_t k, int32_t n_chunks, int64_t n_src, int32_t n_rows);
int als_solve_half(const int64_t* row_ptr, const int32_t* col, const float* val,
                   const int32_t* light_rows, int32_t n_light, int32_t n_light_primal,
                   const int32_t* heavy_rows, const int32_t* heavy_slot_begin, int32_t n_heavy,
                   const int32_t* chunk_row, const int64_t* chunk_begin, const int64_t* chunk_end,
                   int32_t n_chunks, const int32_t* heavy_slot_begin2, int32_t chunk_slot0,
                   const float* Y_src, int64_t n_src, float* X_dst, int32_t ld, int32_t k,
                   float reg, int implicit, float alpha, const double* yty_packed,
                   int32_t* status_dev, void* ws, size_t ws_bytes, int phases, void* stream);

/* K2b: YtY = sum over all n rows of Y of y y^T in fp64 (replaces Spark
 * computeYtY's dspr + treeAggregate).  Output: lower-packed fp64, k_pad(k_pad+1)/2
 * entries, k_pad = als_k_pad(k). */
int32_t als_k_pad(int32_t k);
size_t als_yty_workspace_bytes(int64_t n, int32_t k);
int als_yty(const float* Y, int64_t n, int32_t ld, int32_t k, double* yty_packed_out,
            void* ws, size_t ws_bytes, void* stream);

/* ---- K4: predict / RMSE (replaces MatrixFactorizationModel.predict (ddot)
 *      reached from predictAll at RecommenderSystem.py:150,165,222,232, and the
 *      computeError join+reduce at RecommenderSystem.py:103-129) --------- */

/* pred_out[e] = <U[umap[u[e]]], V[imap[i[e]]]> in fp64 over fp32 factors,
 * NaN when either id is unknown (out of map range or map == -1).  K4 (als_predict
 * and als_rmse_partial) ignores columns [k, ld) of U and V: whatever they hold,
 * NaN included, never reaches a result. */
int als_predict(const int32_t* u, const int32_t* i, int64_t n,
                const int32_t* umap, int32_t umap_size, const int32_t* imap, int32_t imap_size,
                const float* U, const float* V, int32_t ld, int32_t k,
                double* pred_out, void* stream);

/* sse_count_out[0] = sum (r - p)^2 over pairs whose ids are both known,
 * sse_count_out[1] = number of such pairs (inner-join semantics of
 * computeError).  Deterministic (fixed-order fp64 reduction). */
size_t als_rmse_workspace_bytes(int64_t n);
int als_rmse_partial(const int32_t* u, const int32_t* i, const float* r, int64_t n,
                     const int32_t* umap, int32_t umap_size, const int32_t* imap, int32_t imap_size,
                     const float* U, const float* V, int32_t ld, int32_t k,
                     double* sse_count_out, void* ws, size_t ws_bytes, void* stream);

/* ---- K5: recommendForAll (replaces ALSModel.recommendForAll: blockify +
 *      sgemm + bounded priority queue; reference equivalent is the
 *      predictAll + takeOrdered(20) flow at RecommenderSystem.py:229-247) -- */

/* For each of the n_q query rows of Q, the `top` rows of V with the largest
 * score <q, v>, ordered by score descending then index ascending.
 * idx_out[n_q*top] (dense row index of V, -1 when n_v < top), score_out[n_q*top].
 * Scores: fp32-grade products on the f16 matrix cores (q and v split into f16
 * hi + lo after power-of-two scaling, ~2^-21 relative to |q||v|) for every k and
 * top: V is swept with hi.hi alone against the row's k-th score minus a proven
 * bound on the dropped terms, and blocks past it get the full hi.hi + hi.lo + lo.hi
 * score, so every listed pair carries its exact split score.  Lists: registers of
 * one owner lane for top <= 16; for 16 < top <= 128 every key reaching the row's
 * threshold (its exact k-th best score as of the last cut of its log) is appended to a
 * per-row log in the workspace, from which the exact top keys are selected; sorted LDS
 * lists above.  Rows of V holding NaN score NaN and are never listed.
 * k <= 128, top <= 256.  The n_q x n_v score matrix is never materialised.
 * Workspace (16-byte aligned), sized by als_topk_workspace_bytes: scale words, the hi
 * and lo f16 planes of V in sweep (decreasing norm) order, the order, bucket counts, the
 * scaled row norms and, for 16 < top <= 128, the key logs: one log per query row of one
 * launch (at most 512 workgroups of 128 or 256 rows; a larger n_q runs as several
 * launches over the same logs), each holding `top` rounded up to 32, 64, 100 or 128
 * keys plus one V tile's worth (192 or 384), at least 384, rounded up to 64. */
size_t als_topk_workspace_bytes(int64_t n_q, int64_t n_v, int32_t k, int32_t top);
int als_topk(const float* Q, int64_t n_q, const float* V, int64_t n_v,
             int32_t ld, int32_t k, int32_t top,
             int32_t* idx_out, float* score_out, void* ws, size_t ws_bytes, void* stream);

/* als_topk over the admissible rows of V only (ABI 7; the reference's "movies the user
 * has not rated, with more than 75 ratings" at RecommenderSystem.py:229 and :245).  V row
 * j may be listed by query row r only if
 *  - j is not in ex_col[ex_begin[r] .. ex_end[r]) — dense V rows, ascending within the
 *    range, duplicates allowed; ranges may be empty and ranges of different rows may
 *    alias (a subset or slice of query rows points into one shared list).  ex_begin,
 *    ex_end (n_q entries each) and ex_col are all NULL (no exclusions) or all set;
 *  - bit (j & 31) of allow_bits[j >> 5] is set (ceil(n_v / 32) words); NULL allows every
 *    row.
 * Per query row the `top` admissible rows (allowed, not excluded, score not NaN) by
 * score descending then index ascending; the remaining slots hold idx -1, score -inf.
 * An all-zero query row lists its first `top` admissible rows by index with score 0.
 * Scales, split and summation do not depend on the filter: a pair listed by both calls
 * carries the bit-identical score.  An admissibility test (the bit, then a binary search
 * of the row's range) runs only for a pair whose exact score reaches its row's current
 * threshold, so the thresholds are k-th scores among admissible keys and the coarse
 * filter stays exact.  Same workspace and argument rules as als_topk; with all four
 * filter pointers NULL the call is als_topk. */
int als_topk_filtered(const float* Q, int64_t n_q, const float* V, int64_t n_v,
                      int32_t ld, int32_t k, int32_t top,
                      const int64_t* ex_begin, const int64_t* ex_end, const int32_t* ex_col,
                      const uint32_t* allow_bits,
                      int32_t* idx_out, float* score_out,
                      void* ws, size_t ws_bytes, void* stream);

/* ---- K6: ranking metrics (replaces pyspark.mllib.evaluation.RankingMetrics /
 *      pyspark.ml.evaluation.RankingEvaluator over the lists K5 writes; the reference
 *      scores its models by RMSE alone, RecommenderSystem.py:103-129) ---------- */

/* Precision, recall, average precision and NDCG at `at` (ABI 8) of n_q top-k lists
 * against per-row relevant sets, binary relevance.  idx[r*idx_ld + p], p < at, is the
 * dense row listed at position p of query row r (the layout als_topk / als_topk_filtered
 * write; idx_ld >= at); a negative entry is an empty slot and never a hit.
 * rel_col[rel_begin[r] .. rel_end[r]) holds the relevant rows of r, STRICTLY ascending
 * (the caller removes duplicates); ranges may be empty and ranges of different rows may
 * alias, as the ex_* ranges of als_topk_filtered may.  With m_r the range length,
 * hit(p) = 1 when idx[r, p] is in the range, c(p) the hits at positions 0..p and
 * H = c(at - 1), a row with m_r > 0 scores
 *   precision = H / at                  (divided by `at` even when the list is shorter)
 *   recall    = H / m_r
 *   AP        = (sum_{p: hit} c(p) / (p + 1)) / min(m_r, at)
 *   NDCG      = (sum_{p: hit} d(p)) / (sum_{p < min(m_r, at)} d(p)),  d(p) = 1 / log2(p + 2)
 * which are Spark 3.x's precisionAt, recallAt, meanAveragePrecisionAt and ndcgAt per
 * row.  A row with m_r = 0 contributes nothing and is not counted.
 * sums_out[6] = {sum precision, sum recall, sum AP, sum NDCG, rows with m_r > 0, rows
 * with H > 0}.  per_row_out: NULL, or n_q x 4 fp64 = the four values per row (all 0 for
 * a row with m_r = 0).  All arithmetic is fp64; the sums within a row run in position
 * order, and across rows in a fixed order (per-block partials, then one block), so two
 * calls give bit-identical results.  1 <= at <= 256.  ws: 16-byte aligned, sized by
 * als_rank_metrics_workspace_bytes.  n_q == 0 writes six zeros. */
size_t als_rank_metrics_workspace_bytes(int64_t n_q);
int als_rank_metrics(const int32_t* idx, int64_t n_q, int32_t idx_ld, int32_t at,
                     const int64_t* rel_begin, const int64_t* rel_end, const int32_t* rel_col,
                     double* sums_out, double* per_row_out,
                     void* ws, size_t ws_bytes, void* stream);

/* ---- K7: fold-in (one row of Spark's computeFactors + CholeskySolver.solve for rows
 *      that are not in the model; the reference serves a new user by retraining on
 *      their ratings, RecommenderSystem.py:211-218) ------------------------------ */

/* Factor rows for n_rows new rows against the fixed factor table Y_src (ABI 9): one launch,
 * no schedule, no host sync and no pass over Y_src.
 * Row r's ratings are col[row_ptr[r] .. row_ptr[r+1]) / val[...], dense rows of Y_src in
 * any order; duplicates are kept, each occurrence its own term (as Spark does).  An entry
 * with col < 0 or col >= n_src is an item the model does not know: it is skipped and not
 * counted.  With n the number of used entries and n+ those with r > 0,
 *   explicit:  A = sum y y^T + reg*n*I,               b = sum r y
 *   implicit:  A = YtY + sum c1 y y^T + reg*n+*I,     b = sum_{r>0} (1+c1) y,  c1 = alpha*|r|
 * (the arithmetic of als_solve_half and oracle/als_oracle.py normal_equations + solve);
 * yty_packed is the lower-packed fp64 k_pad Gram als_yty writes, required iff implicit.
 * The sums run in fp64 over the fp32 factors, ratings in row order; A is factored
 * (square-root-free LDL^T, the solution of Spark's dppsv) and solved in fp64, and
 * X_out[r*ld_out ..] gets the fp32 solution in columns [0, k) and zeros in [k, ld_out).
 * Two calls give bit-identical output.  n_used_out (nullable): n_used_out[r] = n, the used
 * entries of row r whatever their sign, in both modes.  Columns [k, ld) of Y_src are
 * ignored: whatever they hold, NaN included, never reaches a result (the rule of K4).
 * A row with no used entry is written as all zeros with n_used_out[r] = 0; it is not an
 * error.  A row with a pivot that is not positive (explicit, reg = 0, fewer ratings than k,
 * for example) sets *status_dev to row+1 if the word is still 0 — ANY ONE failing row of
 * the call, whichever reaches the word first, not necessarily the lowest — and is written
 * as zeros; the other rows are solved as usual.  The caller zeroes status_dev.  Positive
 * means above 2^-46 of that pivot's diagonal entry of A: a smaller one is rounding residue
 * of the fp64 elimination (128 * 2^-53), whose sign is chance, so a rank-deficient A is
 * reported whichever way it rounded (dppsv, testing > 0 alone, would solve some of them).
 * 1 <= k <= 128 (ALS_EUNSUPPORTED outside); ld, ld_out >= k and multiples of 4; Y_src and
 * X_out 16-byte aligned; n_rows < 2^31 - 1, n_src < 2^31.  Null pointers, reg < 0,
 * alpha < 0, implicit without yty_packed and n_rows < 0 are ALS_EINVAL, checked on the
 * host before any device call; n_rows == 0 is a no-op returning 0.  Everything lives in
 * registers and LDS: als_fold_in_workspace_bytes returns 0 and ws may be NULL (the two
 * parameters are kept for uniformity with the other entry points).
 * Parity bar: 1e-4 relative per row against the fp64 oracle; measured maxima (ranks
 * 1-128, both modes) are in DESIGN.md section K7 and tests/test_gpu_fold_in.py. */
size_t als_fold_in_workspace_bytes(int64_t n_rows, int32_t k);
int als_fold_in(const int64_t* row_ptr, const int32_t* col, const float* val, int64_t n_rows,
                const float* Y_src, int64_t n_src, int32_t ld, int32_t k,
                float reg, int implicit, float alpha, const double* yty_packed,
                float* X_out, int32_t ld_out, int32_t* n_used_out, int32_t* status_dev,
                void* ws, size_t ws_bytes, void* stream);

/* ---- K8: regression moments (replaces the MultivariateOnlineSummarizer pass behind
 *      pyspark.ml.evaluation.RegressionEvaluator / pyspark.mllib.evaluation.
 *      RegressionMetrics; the reference scores its rank sweep by validation RMSE and
 *      compares test RMSE with a mean-rating baseline, RecommenderSystem.py:136-177) -- */

/* Added under ABI 9 without a version bump: three new symbols, nothing existing changes, so
 * a caller built against the earlier ABI 9 header keeps working.
 * Everything the five regression metrics need, from one pass over n (label, prediction)
 * rows.  out[8], fp64:
 *   out[0] n          rows used            out[4] M2_pred    sum (p - mean_pred)^2
 *   out[1] mean_label                      out[5] sse        sum (l - p)^2
 *   out[2] M2_label   sum (l - mean_l)^2   out[6] sae        sum |l - p|
 *   out[3] mean_pred                       out[7] n_dropped  rows left out (fused form)
 * M2 is never formed as sum x^2 - (sum x)^2 / n: every 16-lane group (fused) or thread
 * (columns) folds its rows into (n, mean, M2) one at a time, and partials are merged by
 * Chan's rule (d = mean_b - mean_a, mean = mean_a + d n_b / n, M2 = M2_a + M2_b +
 * d^2 n_a n_b / n; an empty partial is the identity) in a fixed order: inside a block,
 * then by a single block over the per-block partials.  All arithmetic is fp64, there are
 * no atomics, and two calls give bit-identical output.
 * als_regression_moments (fused): label = r[e], prediction = the fp64 gather-dot of
 * als_predict for (u[e], i[e]); a pair with an unknown id (outside its map, or mapped to
 * -1) is left out and counted in n_dropped — computeError's inner join.  Arguments and
 * their checks are those of als_rmse_partial, columns [k, ld) of U and V are ignored as
 * K4 ignores them, and sse, n equal als_rmse_partial's sums up to summation order.
 * als_regression_moments_cols: label[n] and pred[n] are fp64 device arrays; every row is
 * used (n_dropped = 0).  A NaN in either column makes every error-derived value NaN
 * (the means and M2 of that column, sse, sae) while n still counts the row, as Spark's
 * summarizer does.  The means are accumulated relative to the column's first element
 * (when finite), so data far from zero loses nothing in the merge.
 * n < 0, null pointers (n > 0) and a bad k / ld are ALS_EINVAL, a short workspace is
 * ALS_EWORKSPACE, all checked on the host before any device call.  n == 0 writes eight
 * zeros (out may then be NULL: nothing is written) and returns 0; when every pair of the
 * fused form is unknown, out is zeros with n_dropped = n.  One workspace size serves both
 * forms. */
size_t als_regression_moments_workspace_bytes(int64_t n);
int als_regression_moments(const int32_t* u, const int32_t* i, const float* r, int64_t n,
                           const int32_t* umap, int32_t umap_size,
                           const int32_t* imap, int32_t imap_size,
                           const float* U, const float* V, int32_t ld, int32_t k,
                           double* out, void* ws, size_t ws_bytes, void* stream);
int als_regression_moments_cols(const double* label, const double* pred, int64_t n,
                                double* out, void* ws, size_t ws_bytes, void* stream);

/* ---- K9: full-ranking positions and metrics (the expected percentile rank of Hu, Koren &
 *      Volinsky's implicit-feedback paper, per-row AUC and reciprocal rank; Spark has no
 *      counterpart, and the reference scores its models by RMSE alone,
 *      RecommenderSystem.py:103-129) ------------------------------------------------- */

/* Added under ABI 9 without a version bump, as K8 was: new symbols only.
 * als_rank_positions: where each relevant (held-out) row of V sits in its query row's
 * ordering of ALL admissible rows of V.  Q [n_q, ld], V [n_v, ld]: fp32 factor rows,
 * 1 <= k <= 128 (ALS_EUNSUPPORTED outside), ld >= k and a multiple of 4, both 16-byte
 * aligned, n_v < 2^31 - 1; columns [k, ld) are ignored (the rule of K4).
 * rel_col[rel_begin[r] .. rel_end[r]): the relevant dense V rows of query row r, STRICTLY
 * ascending, the form als_rank_metrics takes — except that the ranges of different rows
 * must not overlap here, since every entry gets an output of its own.  ex_begin / ex_end /
 * ex_col / allow_bits: the filter of als_topk_filtered with the same meaning (ex_col
 * ascending within a range, duplicates allowed, ranges may alias; the three ex_* all NULL
 * or all set; NULL allow_bits allows every row).  V row j is admissible for query row r
 * when it is allowed, not excluded for r, and its score against r is not NaN (K5's rule:
 * NaN scores are never keys).
 * Outputs, aligned with rel_col: above_out[e] = admissible V rows other than rel_col[e]
 * that score strictly higher, tied_out[e] = admissible other rows that score equal; both
 * -1 for an entry that is itself inadmissible (outside [0, n_v), excluded, not allowed) or
 * scores NaN.  n_adm_out[r] = admissible V rows of query row r, each counted once however
 * often ex_col names it.
 * Scores: the fp32 chain s = fmaf(q_d, v_d, s), d = 0 .. k-1 ascending from s = 0, for
 * every score of the call, so |s - s*| <= k 2^-24 / (1 - k 2^-24) * sum_d |q_d v_d| against
 * the fp64 dot product s* (inside tau = 2 k 2^-24 sum_d |q_d v_d|), and a pair scores
 * bit-identically wherever it is computed.  above and tied are exact counts with respect
 * to those scores (-0 equals +0).  The n_q x n_v matrix is never materialised and no
 * workspace is used: ws may be NULL (the parameters are kept for uniformity).
 * als_rank_positions_table: relevant entries one workgroup (32 query rows) ranks per sweep
 * of V; rows holding more between them are swept again, inside the call.
 *
 * als_full_rank_metrics: the counts reduced to fp64 sums.  For query row r let N = n_adm[r],
 * m = its entries with above >= 0 and p_j = above_j + tied_j / 2 (mid-rank, 0 = top):
 *   percentile rank of an entry  p_j / (N - 1)               (rows with N > 1)
 *   row AUC   1 - (sum_j p_j - m (m - 1) / 2) / (m (N - m))  (rows with N > m > 0)
 *   row RR    1 / (1 + min_j p_j)                            (rows with m > 0)
 * sums_out[11] = { sum w pr, sum w (both over the valid entries of rows with N > 1),
 * sum of row-mean pr, sum row AUC, rows with an AUC, sum row RR, rows with an RR, rows with
 * m > 0, valid entries, dropped entries (above < 0), rows with a row-mean pr }.  w: fp32
 * weight per entry aligned with rel_col, NULL = 1.  per_row_out: NULL or n_q x 3 fp64 =
 * row-mean pr, AUC, RR, NaN where undefined.  Fixed summation order (entries of a row by
 * lane then a fixed tree, rows per wave in row order, waves in wave order, blocks by one
 * final block): two calls give bit-identical output.  ws: 16-byte aligned, sized by
 * als_full_rank_workspace_bytes.  n_q < 0 and null pointers are ALS_EINVAL, a short
 * workspace ALS_EWORKSPACE, all checked on the host before any launch; n_q == 0 zeroes
 * sums_out and returns 0. */
size_t als_full_rank_workspace_bytes(int64_t n_q);
int32_t als_rank_positions_table(void);
int als_rank_positions(const float* Q, int64_t n_q, const float* V, int64_t n_v,
                       int32_t ld, int32_t k,
                       const int64_t* rel_begin, const int64_t* rel_end, const int32_t* rel_col,
                       const int64_t* ex_begin, const int64_t* ex_end, const int32_t* ex_col,
                       const uint32_t* allow_bits,
                       int32_t* above_out, int32_t* tied_out, int32_t* n_adm_out,
                       void* ws, size_t ws_bytes, void* stream);
int als_full_rank_metrics(const int32_t* above, const int32_t* tied, const int32_t* n_adm,
                          int64_t n_q, const int64_t* rel_begin, const int64_t* rel_end,
                          const float* w, double* sums_out, double* per_row_out,
                          void* ws, size_t ws_bytes, void* stream);

/* ---- K10: the training objective (the function whose row-wise minimiser als_solve_half
 *      computes; Spark's ALS never evaluates it, and the reference judges a fit by held-out
 *      RMSE alone, RecommenderSystem.py:103-129) --------------------------------------- */

/* Added under ABI 9 without a version bump, as K8 and K9 were: new symbols only.
 * With s = x_row . y_col in fp64 over the fp32 factors (the arithmetic of als_predict), lambda
 * = regParam and Spark's lambda * numExplicits weighting (als_solve_half):
 *   explicit  L = sum_obs (r - s)^2 + lambda (sum_u n_u |x_u|^2 + sum_i n_i |y_i|^2)
 *   implicit  L = sum_all c (p - s)^2 + lambda (sum_u n+_u |x_u|^2 + sum_i n+_i |y_i|^2),
 *             c = 1 + alpha |r|, p = [r > 0]; an unobserved pair has c = 1, p = 0
 * n = ratings of the row, n+ = those with r > 0.  The sum over all pairs is never formed:
 *   sum_all c (p - s)^2 = <X^T X, Y^T Y>_F + sum_obs [c (p - s)^2 - s^2].
 *
 * als_objective_side: one pass over one CSR side (row_ptr int64 [n_rows + 1], col = dense
 * rows of Y, val; X [n_rows, ld] the side's own factors, Y [n_cols, ld] the other side's).
 * out[5], fp64:
 *   out[0] data   sum over the ratings of (r - s)^2, or of c (p - s)^2 - s^2 when implicit
 *   out[1] scale  sum of the absolute values of those terms
 *   out[2] reg    sum_row n_row |x_row|^2 (n+_row when implicit); NOT multiplied by lambda
 *   out[3] n      ratings            out[4] n_positive  ratings with r > 0
 * Y = NULL: no Y row is read and out[0] = out[1] = 0 (the other side's call for its
 * regulariser: both sides hold the same ratings, so the data term is needed once).  A col
 * outside [0, n_cols) adds no data term and is never dereferenced; its rating still counts
 * in n, n_positive and reg (the counts are taken before the range test).  Work is split by
 * ratings, als_objective_span() per block whichever rows they fall in, so one row of 10^5
 * ratings costs per rating what a short one does.  alpha is widened to fp64 from the fp32
 * the solver takes.  Columns [k, ld) of X and Y are ignored.
 * als_gram_dot_f64: *out = <A^T A, B^T B>_F of two fp32 tables [n_a, ld] and [n_b, ld], the
 * Grams formed HERE in fp64 on the matrix cores (not als_yty's fp32 sums: their ~1e-7
 * relative error moves with the fixed side and would swamp the decrease being measured
 * near convergence).  gram_a_out / gram_b_out: NULL, or k x k row-major fp64 receiving the
 * two Grams.  Columns [k, ld) are masked, not assumed zero.
 * Both: every sum is fp64, there are no atomics, per-block partials are folded in ascending
 * block order and the partition depends on the sizes alone: two calls give bit-identical
 * output.  1 <= k <= 128 (ALS_EUNSUPPORTED outside), ld >= k and a multiple of 4, factors
 * 16-byte aligned, null pointers and negative sizes ALS_EINVAL, a short workspace
 * ALS_EWORKSPACE — all checked on the host before any device call.  nnz == 0 (or, for the
 * Grams, an empty table) writes zeros and returns 0; out may then be NULL.
 * als_objective_workspace_bytes(nnz, n_rows, k) serves both calls for sides of at most nnz
 * ratings and tables of at most n_rows rows. */
size_t als_objective_workspace_bytes(int64_t nnz, int64_t n_rows, int32_t k);
int32_t als_objective_span(void);
int als_objective_side(const int64_t* row_ptr, const int32_t* col, const float* val,
                       int64_t nnz, int32_t n_rows, int32_t n_cols,
                       const float* X, const float* Y, int32_t ld, int32_t k,
                       int implicit, float alpha, double* out,
                       void* ws, size_t ws_bytes, void* stream);
int als_gram_dot_f64(const float* A, int64_t n_a, const float* B, int64_t n_b,
                     int32_t ld, int32_t k, double* out,
                     double* gram_a_out, double* gram_b_out,
                     void* ws, size_t ws_bytes, void* stream);

/* ---- K11: explain a score as one contribution per rating of the row (the follow-up of the
 *      reference's closing top-20 print, RecommenderSystem.py:247: "because you rated X 5
 *      and Y 4"; implicit.explain offers it, Spark does not) ---- */

/* Added under ABI 9 without a version bump: two new symbols, nothing existing changes.
 * A row's factor solves its normal equations, x = A^-1 b with b = sum_j wb_j y_j, so
 *   score(row, t) = y_t^T A^-1 b = sum_j wb_j (z_t . y_j),   z_t = A^-1 y_t,
 * one term per used entry j of the row.  The row's entries, the skipped ones (col < 0 or
 * col >= n_src), duplicates, n, the weights wa / wb, the YtY term, the pivot rule and the
 * status word are exactly als_fold_in's (above); A is formed and factored once per row, in
 * fp64, however many targets the row has.
 * Targets are ragged: row r explains tgt[tgt_ptr[r] .. tgt_ptr[r+1]), dense rows of Y_src;
 * T = tgt_ptr[n_rows] slots in all, and slot s writes
 *   score[s]                  the fp64 sum of ALL the row's contributions in row order
 *                             (not only the listed ones), rounded to fp32
 *   contrib[s*top_n + i]      the i-th largest contribution, fp64 rounded to fp32
 *   contrib_pos[s*top_n + i]  the offset inside the row (0 = col[row_ptr[r]]) of the entry
 *                             that made it
 * ordered by fp64 contribution descending, ties by ascending offset.  Every used entry is a
 * candidate (an implicit entry with r <= 0 has wb = 0 and contributes exactly 0); list
 * slots past the row's used entries hold contrib_pos -1 and contrib 0.  The dot comes
 * first, then the weight, so two entries of one item with one rating tie bit for bit.  A
 * target the row also rated and a repeated target are ordinary.  An unknown target (< 0 or
 * >= n_src), a row without a used entry and a row whose A is not positive definite (which
 * sets *status_dev to row+1 as als_fold_in does) get score 0 and an empty list.  A row
 * without targets is counted (n_used_out) but not factored and cannot set the status.
 * n_used_out is nullable.  Two calls give bit-identical output.
 * 1 <= k <= 128 and 1 <= top_n <= 32 (ALS_EUNSUPPORTED outside); ld >= k and a multiple of
 * 4; Y_src 16-byte aligned; a row has fewer than 2^31 entries.  Null pointers (tgt, score,
 * contrib_pos and contrib too, even when T is 0), reg < 0, alpha < 0, implicit without
 * yty_packed and n_rows < 0 are ALS_EINVAL, checked on the host before any device call;
 * n_rows == 0 is a no-op returning 0.  als_explain_workspace_bytes returns 0 and ws may be
 * NULL.  Measured error against the fp64 reference and the cost against als_fold_in:
 * DESIGN.md section K11. */
size_t als_explain_workspace_bytes(int64_t n_rows, int32_t k);
int als_explain(const int64_t* row_ptr, const int32_t* col, const float* val, int64_t n_rows,
                const float* Y_src, int64_t n_src, int32_t ld, int32_t k,
                float reg, int implicit, float alpha, const double* yty_packed,
                const int64_t* tgt_ptr, const int32_t* tgt, int32_t top_n,
                float* score, int32_t* contrib_pos, float* contrib,
                int32_t* n_used_out, int32_t* status_dev,
                void* ws, size_t ws_bytes, void* stream);

/* ---- K12: similar items / users (cosine nearest neighbours of a few query vectors among
 *      the rows of one factor table; what Spark users do on the host over itemFactors, and
 *      what other factorisation libraries offer as similar_items / similar_users) ---- */

/* Added under ABI 9 without a version bump: three new symbols, nothing existing changes.
 * als_similar: for each of the n_q query vectors Q [n_q, ldq] the `top` rows of the table
 * T [n, ld] with the largest cosine, score = <q, t> / (|q| |t|) over columns [0, k) of the
 * raw fp32 rows (columns [k, ld) and [k, ldq) are ignored, whatever they hold).  The grid
 * runs over contiguous slices of T, one pass per 16 queries; |t|^2 comes from the registers
 * that hold the row for the dot products: no normalised copy, no norm array and no pass
 * over T before the sweep.  fp32 throughout except |q|, which is fp64; the dot errs by at
 * most k 2^-24 |q||t|.  Order: score descending, ties by ascending row (the exact 64-bit
 * key of als_topk), so the lists depend neither on `slices` nor on the order workgroups
 * finish, and a (query, row) pair scores the same bits wherever it is computed.
 * Never listed: row self_rows[q] (by index; -1 or a NULL self_rows: none — another row
 * with the same factors is listed, at score 1); a row whose bit is clear in allow_bits
 * (als_topk_filtered's mask; NULL: every row); a row whose fp32 |t|^2 is zero, NaN or Inf
 * (an all-zero row, a row holding a NaN or an Inf; also one so small or so large that the
 * fp32 sum of squares leaves the normal range).  A query with zero norm, a NaN or an Inf
 * gets an empty list.  Empty and open slots: idx -1, score -inf.
 * slices: 0 = 8 per compute unit, at most n / max(256, 2 top); otherwise the number of
 * slices, 1 .. 4096.  Each slice writes `top` keys per query to the workspace with plain
 * stores (no atomics); a second launch, one wavefront per query (two stages above 64
 * slices), selects, ranks and unpacks them.
 * 1 <= k <= 128 and 1 <= top <= 256 (ALS_EUNSUPPORTED outside); ld, ldq >= k and multiples
 * of 4; T, Q and ws 16-byte aligned; n < 2^31 - 1.  Bad sizes, slices outside [0, 4096] and
 * null pointers are ALS_EINVAL, a short workspace ALS_EWORKSPACE, all checked on the host
 * before any launch; n_q == 0 is a no-op.  als_similar_workspace_bytes returns 0 for
 * arguments als_similar rejects.
 * als_similar_unit_rows: out [n, ld] = t / |t| per row (fp64 norm over columns [0, k),
 * fp32 quotient, columns [k, ld) zero), for callers that hand a normalised table to
 * als_topk_filtered.  A row that can be nobody's neighbour (zero norm, NaN, Inf) becomes
 * zeros, has its bit cleared in allow_bits (nullable; ceil(n / 32) words, bits past n are
 * cleared too) and 0 in valid_out (nullable, int32 [n], 1 otherwise).  One launch. */
size_t als_similar_workspace_bytes(int64_t n, int32_t n_q, int32_t top, int32_t slices);
int als_similar(const float* T, int64_t n, int32_t ld, int32_t k,
                const float* Q, int64_t n_q, int32_t ldq,
                const int32_t* self_rows, const uint32_t* allow_bits,
                int32_t top, int32_t slices,
                int32_t* idx_out, float* score_out,
                void* ws, size_t ws_bytes, void* stream);
int als_similar_unit_rows(const float* T, int64_t n, int32_t ld, int32_t k, float* out,
                          uint32_t* allow_bits, int32_t* valid_out, void* stream);

/* ---- K13: nonnegative rows (Spark's `nonnegative=true`: computeFactors with NNLSSolver
 *      in place of CholeskySolver, mllib/optimization/NNLS.scala) -------------------- */

/* Added under ABI 9 without a version bump: two new symbols, nothing existing changes.
 * als_nnls_rows: the factor row x >= 0 that minimises x^T A x / 2 - b^T x for each of the
 * n_rows ragged rows, with A and b EXACTLY als_fold_in's (above): the same input layout
 * (row_ptr int64, col int32 dense rows of Y_src, val fp32; a RatingBlock's CSR has this
 * shape, so the call serves a training half-sweep and a fold-in alike), the same skipping of
 * unknown columns (col < 0 or >= n_src: not counted), the same sums in fp64 over the fp32
 * factors in rating order, the same reg * n (explicit) / reg * n+ (implicit) diagonal and
 * the same yty_packed (required iff implicit).  Columns [k, ld) of Y_src are ignored
 * whatever they hold.
 * The solver is Spark's NNLS.solve in fp64: from x = 0, projected-gradient steps with
 * conjugate-gradient directions (dropped for one iteration after a coordinate hits the
 * wall), the exact line minimum clamped so that no coordinate goes negative, at most
 * max(400, 20 k) iterations, stopped when the step is NaN, below 1e-7 or above 1e40, or the
 * squared direction is below 1e-12 |x|^2 or 1e-32.  The step test also stops a row at x = 0
 * whose A has eigenvalues above ~1e7 (tens of millions of ratings, or factors of norm 1e4):
 * that is Spark's behaviour and is reproduced, not repaired.  No row fails: a row with
 * b = 0 (no used entry; implicit without a positive rating) is all zeros at the first test.
 * X_out[r*ld_out ..] gets the fp32 solution in columns [0, k), every value >= 0, and zeros
 * in [k, ld_out).  n_used_out (nullable): the used entries of row r.  iters_out (nullable,
 * int32 [n_rows]): the iteration count at return.  Two calls give bit-identical output.
 * A row with more than `chunk` ratings is cut into chunk-rating tasks, one workgroup each,
 * whose fp64 partial (A, b, n, n+) go to workspace slots and are summed in slot order before
 * the solve, so a long row never runs serially; rows are solved longest first (sorted by
 * degree on the device).  als_nnls_workspace_bytes(n_rows, nnz, k, chunk) sizes the
 * workspace for any rows with nnz entries in all (0 for arguments als_nnls_rows rejects);
 * with a smaller workspace that still holds the per-row arrays, the long rows its slots
 * cannot take are summed serially (same result up to the order of the fp64 sums).
 * 1 <= k <= 128 (ALS_EUNSUPPORTED outside); ld, ld_out >= k and multiples of 4; Y_src, X_out
 * and ws 16-byte aligned; n_rows < 2^31 - 1, n_src < 2^31, chunk >= 1.  Null pointers,
 * reg < 0, alpha < 0, implicit without yty_packed and n_rows < 0 are ALS_EINVAL, a workspace
 * too small for the per-row arrays ALS_EWORKSPACE, all checked on the host before any device
 * call; n_rows == 0 is a no-op returning 0.
 * Parity bar: 1e-4 relative per row against the fp64 restatement tests/nnls_ref.py; measured
 * maxima and the KKT residuals are in DESIGN.md section K13 and tests/test_gpu_nnls.py. */
size_t als_nnls_workspace_bytes(int64_t n_rows, int64_t nnz, int32_t k, int32_t chunk);
int als_nnls_rows(const int64_t* row_ptr, const int32_t* col, const float* val, int64_t n_rows,
                  const float* Y_src, int64_t n_src, int32_t ld, int32_t k,
                  float reg, int implicit, float alpha, const double* yty_packed,
                  int32_t chunk, float* X_out, int32_t ld_out, int32_t* n_used_out,
                  int32_t* iters_out, void* ws, size_t ws_bytes, void* stream);

/* ---- K14: diversified lists (maximal marginal relevance, Carbonell & Goldstein 1998;
 *      intra-list similarity, Ziegler et al. 2005) ------------------------------------- */

/* Added under ABI 9 without a version bump: two new symbols only, nothing existing changes.
 * als_diversify: re-ranks each query row's candidate pool.  Per row a pool of m slots
 * (1 <= m <= 256), idx int32 [n_q, m] and score f32 [n_q, m] as als_topk / als_topk_filtered
 * return them (dense rows of V, open slots -1 / -inf), against the other side's table
 * V [n_v, ld] of rank k; columns [k, ld) are ignored whatever they hold.
 *   live slot: 0 <= idx < n_v and a finite score; every other slot is dead and never
 *     picked.  Duplicate indices in a pool are separate candidates.
 *   rel_j = (s_j - s_min) / (s_max - s_min) in fp64 over the row's live slots, 1 for all
 *     when s_max == s_min.
 *   unit vector = v_j / |v_j|, the norm in fp64 over columns [0, k), stored in fp32; a row
 *     with zero norm or a non-finite entry has the zero vector, so its cosine with
 *     everything is 0 (it can still be picked).  cos(j, s) = <unit_j, unit_s>, summed in
 *     fp32 in ascending column order.
 *   greedy: step 0 picks the live slot with the largest rel; step t >= 1 the live unpicked
 *     slot with the largest lam * rel_j - (1 - lam) * max_{u < t} cos(j, s_u), in fp64 over
 *     the fp32 cosines; ties go to the lowest slot position at every step; it stops after
 *     `top` picks or when the live slots run out.
 * out_idx int32 [n_q, top] / out_score f32 [n_q, top]: the picked slots' idx and their
 * original scores bit for bit, in pick order (no longer score-descending); open slots
 * -1 / -inf.  out_ils f64 [n_q]: the mean of cos over the unordered pairs of the picked
 * list, NaN with fewer than two picks.  At lam = 1 the output is the live prefix of a
 * score-descending pool exactly.  lam is a float, as reg and alpha are everywhere in this
 * ABI, and is widened to fp64 in the kernel.  Two calls give bit-identical output.
 * als_list_similarity: out f64 [n_q] = the same mean over the slots of idx int32 [n_q, m]
 * with 0 <= idx < n_v (m <= 256), NaN with fewer than two: the intra-list similarity of
 * lists that came from anywhere.
 * 1 <= k <= 128 and 1 <= m <= 256 (ALS_EUNSUPPORTED outside); ld >= k and a multiple of 4,
 * V 16-byte aligned, 1 <= top <= m, lam in [0, 1] (a NaN is outside), n_v < 2^31,
 * 0 <= n_q < 2^31 - 1 and non-null pointers (ALS_EINVAL otherwise), all checked on the host
 * before any launch; n_q == 0 is a no-op.  No workspace. */
int als_diversify(const float* V, int64_t n_v, int32_t ld, int32_t k,
                  const int32_t* idx, const float* score, int64_t n_q, int32_t m,
                  int32_t top, float lam,
                  int32_t* out_idx, float* out_score, double* out_ils, void* stream);
int als_list_similarity(const float* V, int64_t n_v, int32_t ld, int32_t k,
                        const int32_t* idx, int64_t n_q, int32_t m,
                        double* out, void* stream);

/* ---- K15: the lists of all users together (catalogue coverage, Herlocker et al. 2004;
 *      novelty and personalisation, Zhou et al. 2010; average popularity and long-tail
 *      share, Abdollahpouri et al.).  Replaces nothing in Spark, which has none of these;
 *      the reference only filters by popularity, RecommenderSystem.py:245 ------------------ */

/* Added under ABI 9 without a version bump: six new symbols only, nothing existing changes.
 * Lists, for all three calls: idx int32 [n_q, idx_ld], the layout als_topk* / als_diversify
 * write; only the first `at` positions of a row count (1 <= at <= 256, idx_ld >= at; what
 * lies past them is never read).  An entry is VALID when 0 <= idx < n_v and, when allow_bits
 * is given (als_topk_filtered's mask: ceil(n_v / 32) words, bits past n_v ignored), its bit
 * is set; the catalogue is then the allowed rows only.  Every other entry is skipped: the -1
 * of an open slot, an id the model does not know, a row outside the catalogue.  Duplicates
 * inside one list each count (K5 never writes any; the overlap identity below assumes none).
 *
 * als_list_exposure: counts[j] (int32 [n_v]) = the valid entries naming row j.  accumulate
 * != 0 adds to what counts and *n_skipped_dev hold, so lists can be fed in chunks;
 * accumulate == 0 overwrites both in full, rows nobody lists included.  n_skipped_dev
 * (int64, nullable) = the skipped entries among the n_q * at.  Integer adds only: the counts
 * are exact and bit-identical run to run whatever order the adds land in.  Each workgroup
 * keeps als_list_exposure_window() int32 counters in LDS as a direct-mapped cache of the
 * catalogue (row j in slot j mod window, first row to arrive owns the slot; a row that finds
 * its slot taken is added in memory) and adds its non-zero slots to counts once at the end,
 * so with n_v <= window nothing but those final adds reaches memory, and in a larger skewed
 * catalogue the rows that take most entries are summed on chip.  No workspace.  The total
 * per row must fit int32.
 *
 * als_list_concentration: n = the catalogue rows (n_v, or the set bits below n_v), c_j their
 * counts (a negative count reads as 0), T = sum c_j.  out[7], fp64:
 *   out[0] n                           out[1] rows with c_j > 0 (coverage = out[1] / out[0])
 *   out[2] T                           out[5] sum_j c_j (c_j - 1) / 2
 *   out[3] Gini index of exposure, sum_{j=1..n} (2j - n - 1) c_(j) / (n T) over the ascending
 *          counts: 0 when every row is listed equally often, 1 - 1/n when one row takes
 *          everything; NaN when T = 0
 *   out[4] Shannon entropy in bits, -sum_{c_j > 0} (c_j / T) log2(c_j / T); NaN when T = 0
 *   out[6] max_j c_j
 * out[5] counts the (pair of lists, shared row) incidences of duplicate-free lists, so
 * personalisation = 1 - out[5] / (C(n_lists, 2) at), formed by the caller; n_lists and at
 * are only checked.  The counts are sorted by the library's radix sort with rows outside the
 * catalogue keyed 0: zeros add nothing to the Gini sum, and a non-zero count's catalogue rank
 * is its rank in the full sort minus n_v - n.  All sums are fp64 in a fixed order (per-block
 * partials in row order, then in sorted order, each folded by one block): two calls give
 * identical bits, and every value is exact while it stays below 2^53.  n_v == 0 writes
 * {0, 0, 0, NaN, NaN, 0, 0}.
 *
 * als_list_novelty: pop int32 [n_v] = how often each row was rated (a RatingBlock's
 * row-pointer differences), n_pop = the rows of the listing side, tail_bits (nullable, the
 * form of allow_bits) = the long-tail rows.  One wavefront per list; over the valid entries
 * of row r in position order, in fp64:
 *   novelty_r  mean of log2(n_pop / pop_j) over the entries with pop_j > 0 (mean
 *              self-information in bits); NaN without such an entry
 *   arp_r      mean of pop_j over all valid entries; NaN without a valid entry
 *   tail_r     share of the valid entries whose bit is set in tail_bits; NaN when tail_bits
 *              is NULL or the row has no valid entry
 * sums_out[7] = { sum novelty_r, rows with a novelty, sum arp_r, rows with a valid entry,
 * sum tail_r, valid entries, skipped entries }; a NaN row adds nothing and is not counted.
 * per_row_out: NULL or f64 [n_q, 3] = novelty_r, arp_r, tail_r.  Fixed summation order (rows
 * per wave in row order, waves in wave order, blocks by one final block): two calls give
 * bit-identical output.
 *
 * All three, checked on the host before any launch: at outside [1, 256] is
 * ALS_EUNSUPPORTED; negative sizes, idx_ld < at, n_v >= 2^31 - 1, n_pop < 1, null pointers
 * (when the sizes are non-zero) and a workspace that is not 16-byte aligned are ALS_EINVAL;
 * a short workspace is ALS_EWORKSPACE.  n_q == 0 is defined: the counts are zeroed unless
 * accumulating, the sums are zeroed.  The two workspaces (16-byte aligned) are sized by
 * als_list_concentration_scratch_bytes(n_v) (0 for an n_v the call rejects) and
 * als_list_novelty_scratch_bytes(n_q).  Costs beside K5 and beside torch.bincount: DESIGN.md
 * section K15. */
int32_t als_list_exposure_window(void);
int als_list_exposure(const int32_t* idx, int64_t n_q, int32_t idx_ld, int32_t at, int64_t n_v,
                      const uint32_t* allow_bits, int accumulate, int32_t* counts,
                      int64_t* n_skipped_dev, void* stream);
size_t als_list_concentration_scratch_bytes(int64_t n_v);
int als_list_concentration(const int32_t* counts, int64_t n_v, const uint32_t* allow_bits,
                           int64_t n_lists, int32_t at, double* out, void* ws, size_t ws_bytes,
                           void* stream);
size_t als_list_novelty_scratch_bytes(int64_t n_q);
int als_list_novelty(const int32_t* idx, int64_t n_q, int32_t idx_ld, int32_t at, int64_t n_v,
                     const uint32_t* allow_bits, const int32_t* pop, int64_t n_pop,
                     const uint32_t* tail_bits, double* sums_out, double* per_row_out,
                     void* ws, size_t ws_bytes, void* stream);

/* ---- K16: rating statistics and bias baselines.  Replaces the reference's
 *      getCountsAndAverages and "more than 500 reviews" filter (RecommenderSystem.py:49-86)
 *      and its training-mean baseline (RecommenderSystem.py:172-177); with a bias table it is
 *      the sweep of the damped baseline predictor mu + b_u + b_i (Koren 2010, section 2.1).
 *      Spark has neither -------------------------------------------------------------------- */

/* Added under ABI 9 without a version bump: six new symbols only, nothing existing changes.
 * A by-value double does not appear in this header; the three fp64 scalars below are passed
 * by address, *_host pointing to HOST memory that is read before the call returns (NULL = 0).
 *
 * als_row_moments: one CSR side as a RatingBlock holds it (row_ptr int64 [n_rows + 1], col
 * int32 [nnz], val fp32 [nnz]).  Over the terms
 *   e_j = (double)val_j - *offset_host - (other ? other[col_j] : 0)
 * of each row, `other` NULL or fp64 [n_cols] (a col_j outside [0, n_cols) takes 0 and is not
 * dereferenced; with other == NULL col is never read and may be NULL):
 *   moments  fp64 [n_rows, 5] = { n, sum e, M2 = sum (e - mean_row)^2, min e, max e }; n is
 *            exact, min and max are exact and NaN for a row without ratings (whose n, sum and
 *            M2 are 0)
 *   total    fp64 [5] = the same five over all ratings of the side (NaN min / max when
 *            nnz = 0); sum e^2 = M2 + sum^2 / n is a baseline's training SSE
 * All accumulation is fp64.  M2 is merged by Chan's rule (never sum e^2 - sum^2 / n).  No
 * atomics: the order of every addition is a function of row_ptr alone, so two calls give
 * identical bytes.  A row of more than als_rating_stats_task() ratings is cut into tasks of
 * that many, one workgroup each, merged in ascending task order; every other row is read by
 * a 16-lane group, als_rating_stats_group_rows() rows per workgroup.  col and val are read
 * with 16-byte loads when both are 16-byte aligned and with 4-byte loads otherwise, to the
 * same bits.  Row bounds are clamped to [0, nnz], so a row_ptr that does not describe nnz
 * ratings gives wrong numbers and no access outside col / val.
 * Scratch: als_rating_stats_scratch_bytes(nnz, n_rows) bytes, 16-byte aligned (0 for sizes
 * the call rejects); moments, total and other 8-byte aligned.
 *
 * als_bias_update: bias_out[row] (fp64 [n_rows]) = sum_row / (*damping_host + n_row) from a
 * moments table, 0 for a row with n = 0.  A separate call, not an output of the sweep: the
 * sweep stays a statistics pass and the update is one thread per row.
 *
 * als_baseline_predict: n pairs of dense rows (int32, -1 or anything outside [0, n_users) /
 * [0, n_items) = unknown id):
 *   pred[e]  (fp32) = *mu_host + (user known ? bu[urow] : 0) + (item known ? bi[irow] : 0),
 *            summed in fp64 and rounded once; bu / bi fp64, each may be NULL = all zero
 *   known[e] (uint8) = bit 0 user known, bit 1 item known
 *
 * Checked on the host before any device call: a negative size is ALS_EINVAL; nnz >= 2^40,
 * n_rows >= 2^31 - 1 or n >= 2^39 ALS_EUNSUPPORTED; a NULL row_ptr / moments / total /
 * bias_out / urow / irow / pred / known, a NULL val (or col, with other) when nnz > 0, a
 * misaligned table or scratch and a negative or non-finite damping ALS_EINVAL; a short
 * scratch ALS_EWORKSPACE.  n_rows == 0 and n == 0 are valid and do nothing (total is then
 * left as it is).  Costs beside torch and beside the byte floor: DESIGN.md section K16. */
int32_t als_rating_stats_task(void);
int32_t als_rating_stats_group_rows(void);
size_t als_rating_stats_scratch_bytes(int64_t nnz, int64_t n_rows);
int als_row_moments(const int64_t* row_ptr, const int32_t* col, const float* val, int64_t nnz,
                    int32_t n_rows, int32_t n_cols, const double* other,
                    const double* offset_host, double* moments, double* total, void* ws,
                    size_t ws_bytes, void* stream);
int als_bias_update(const double* moments, int32_t n_rows, const double* damping_host,
                    double* bias_out, void* stream);
int als_baseline_predict(const int32_t* urow, const int32_t* irow, int64_t n,
                         const double* mu_host, const double* bu, int32_t n_users,
                         const double* bi, int32_t n_items, float* pred, uint8_t* known,
                         void* stream);

/* ---- K17: add ratings to a built CSR side (the reference appends a new user's ratings to
 *      the training set and fits again, RecommenderSystem.py:207-247; Spark rebuilds its
 *      blocks from the union) -------------------------------------------------------------- */

/* Added under ABI 9 without a version bump: two new symbols only, nothing existing changes.
 * The CSR als_csr_build would make of concat(old ratings, batch), from the CSR of the
 * old ratings and the CSR of the batch, in one streaming pass with no sort.  K1's layout makes
 * that exact: dense rows are in ascending id order and a row keeps its ratings in input order,
 * duplicates included, so every row of the result is its old segment followed by its batch
 * segment.
 *   old side    row_ptr_old int64 [n_old + 1], col_old int32 [nnz_old], val_old f32 [nnz_old],
 *               nnz_old = row_ptr_old[n_old]; columns are dense rows of the other side as it
 *               was, n_cols_old of them
 *   new_of_old_row  int32 [n_old]: the dense row each old row has in the grown id map,
 *               STRICTLY increasing, values in [0, n_new).  NULL = identity: no new row ids,
 *               so n_new == n_old (or n_old == 0)
 *   new_of_old_col  int32 [n_cols_old]: the same for the other side; NULL = identity
 *   batch       row_ptr_add int64 [n_new + 1], col_add int32 [nnz_add], val_add f32 [nnz_add],
 *               nnz_add = row_ptr_add[n_new]: als_csr_build of the batch alone against the
 *               GROWN id maps, so rows and columns are already in the new dense spaces
 *   outputs     row_ptr_out int64 [n_new + 1], col_out int32 [nnz_old + nnz_add],
 *               val_out f32 [nnz_old + nnz_add]; they may not alias an input
 * For every new row r with j = the number of old rows placed before r:
 *   row_ptr_out[r] = row_ptr_old[j] + row_ptr_add[r]      (a lower bound in new_of_old_row
 *                                                          per row: no scan)
 *   the row holds the old segment of r (if new_of_old_row[j] == r), columns passed through
 *   new_of_old_col, in its old order, then col_add / val_add of [row_ptr_add[r],
 *   row_ptr_add[r + 1]).  Values are copied as bits.
 * Work is split over output ENTRIES, als_csr_merge_tile() of them per workgroup whichever rows
 * they fall in (one binary search in row_ptr_out per tile, then the rows in order), so an
 * item row of 10^5 ratings costs per rating what a short one does.  Integer and copy work
 * only, no atomics, every output word written once: two calls give identical bytes, and the
 * result equals als_csr_build on the concatenation bit for bit.  No scratch is used.  An
 * index that inconsistent row pointers would take outside col_old / col_add is not
 * dereferenced (the entry is written as col -1, val 0), and an old column outside
 * [0, n_cols_old) maps to -1.
 * Checked on the host before any launch: a negative size, n_new < n_old, n_new > n_old > 0
 * without new_of_old_row and null pointers (col / val of a side only when that side has
 * entries) are ALS_EINVAL; n_new >= 2^31 - 1 or
 * nnz_old + nnz_add >= 2^31 (K1's limit) ALS_EUNSUPPORTED.  nnz_add == 0 with NULL maps is a
 * plain copy.  Cost beside als_csr_build and beside the byte floor: DESIGN.md section K17. */
int32_t als_csr_merge_tile(void);
int als_csr_merge(const int64_t* row_ptr_old, const int32_t* col_old, const float* val_old,
                  int64_t nnz_old, int32_t n_old, int32_t n_cols_old,
                  const int32_t* new_of_old_row, const int32_t* new_of_old_col,
                  const int64_t* row_ptr_add, const int32_t* col_add, const float* val_add,
                  int64_t nnz_add, int32_t n_new,
                  int64_t* row_ptr_out, int32_t* col_out, float* val_out, void* stream);

/* ---- K18: remove ratings from a built CSR side (un-rate a pair, forget a user, withdraw an
 *      item; Spark rebuilds its blocks from the filtered set) ------------------------------- */

/* Added under ABI 9 without a version bump: four new symbols only, nothing existing changes.
 * The CSR als_csr_build would make of the old ratings with every copy of every listed
 * (row, column) pair filtered out and the order kept, from the CSR of the old ratings, as a
 * stream compaction in two calls with no sort.  K1's layout makes that exact: dense rows are in
 * ascending id order and a row keeps its ratings in input order, duplicates included, so every
 * row of the result is the stored row with the listed entries dropped.
 *   old side    row_ptr_old int64 [n_old + 1], col_old int32 [nnz_old], val_old f32 [nnz_old],
 *               nnz_old = row_ptr_old[n_old]; rows may be empty
 *   delete list a CSR over the same dense rows: row_ptr_del int64 [n_old + 1], col_del int32
 *               [nnz_del], each row's columns ASCENDING (a column listed twice is harmless);
 *               both may be NULL when nnz_del == 0
 *   tiles       = ceil(nnz_old / als_csr_remove_tile()); the tile is a multiple of 64
 * als_csr_remove_mark writes
 *   keep_bits   uint64 [ceil(nnz_old / 64)]: bit q % 64 of word q / 64 is 1 iff entry q stays,
 *               i.e. col_old[q] does not occur in its row's delete list (a binary search; a row
 *               with an empty list costs one comparison).  Every stored copy of a listed pair
 *               goes.  One wave ballot per word; the tail bits of the last word are 0
 *   tile_off    int64 [tiles + 1]: the exclusive scan of the tiles' kept counts, so
 *               tile_off[tiles] = nnz_out.  The counts go through `scratch` (int32 [tiles],
 *               als_csr_remove_scratch_bytes(nnz_old, n_old) bytes) and are scanned by one
 *               workgroup of the same call: no host read
 *   row_ptr_kept int64 [n_old + 1], in the OLD row numbering: the number of kept entries before
 *               row_ptr_old[r] (tile_off of its tile plus popcounts of that tile's words below
 *               it), so row r keeps row_ptr_kept[r + 1] - row_ptr_kept[r] entries — 0 for a row
 *               that lost everything or was empty — and row_ptr_kept[n_old] = nnz_out.  The row
 *               pointer of the result is row_ptr_kept restricted to the rows the caller keeps
 *   del_hits    int32 [nnz_del] or NULL: the stored copies dropped for each listed pair (0 = the
 *               pair was not stored); zeroed and then counted with integer atomic adds, the only
 *               atomics of K18
 * als_csr_remove_compact takes col_old, val_old, keep_bits and tile_off as mark left them, and
 *   new_of_old_col int32 [n_cols_old] or NULL: the dense row each old row of the OTHER side has
 *               after its rows left, -1 for a row that left; NULL = identity (the column is
 *               copied).  With a map, a column outside [0, n_cols_old) is written as -1
 *   outputs     col_out int32 [nnz_out], val_out f32 [nnz_out], nnz_out = tile_off[tiles] read
 *               by the caller (who needs row_ptr_kept on the host anyway to see which rows
 *               left).  Kept entry q goes to tile_off[q / tile] + its rank among the tile's kept
 *               entries; the value is copied as bits.  No output may alias an input
 * Work is split over stored ENTRIES, one tile per workgroup whichever rows they fall in (one
 * binary search in row_ptr_old per tile, then the rows in order through LDS), so an item row of
 * 10^5 ratings costs per rating what a short one does.  No sort, no floating-point arithmetic,
 * every output word written once (del_hits: zeroed, then added to): two calls give identical
 * bytes, and row pointer, columns and values equal als_csr_build on the filtered ratings bit for
 * bit.  An index that inconsistent row pointers or a foreign tile_off would take outside a buffer
 * is not dereferenced (delete ranges are clamped to [0, nnz_del], row positions to [0, nnz_old],
 * destinations outside [0, nnz_out) are skipped).
 * Checked on the host before any launch: a negative size and a null pointer (col / val /
 * keep_bits only when the side has entries, the delete list only when nnz_del > 0, outputs only
 * when nnz_out > 0) are ALS_EINVAL, as is nnz_out > nnz_old; nnz_old >= 2^31 or
 * n_old >= 2^31 - 1 (K1's limit) ALS_EUNSUPPORTED; a scratch below the stated size
 * ALS_EWORKSPACE.  nnz_del == 0 is a plain copy: every bit set, row_ptr_kept == row_ptr_old.
 * Cost beside als_csr_build and beside the byte floor: DESIGN.md section K18. */
int32_t als_csr_remove_tile(void);
size_t als_csr_remove_scratch_bytes(int64_t nnz_old, int32_t n_old);
int als_csr_remove_mark(const int64_t* row_ptr_old, const int32_t* col_old, int64_t nnz_old,
                        int32_t n_old, const int64_t* row_ptr_del, const int32_t* col_del,
                        int64_t nnz_del, uint64_t* keep_bits, int64_t* tile_off,
                        int64_t* row_ptr_kept, int32_t* del_hits, void* scratch,
                        size_t scratch_bytes, void* stream);
int als_csr_remove_compact(const int32_t* col_old, const float* val_old, int64_t nnz_old,
                           const uint64_t* keep_bits, const int64_t* tile_off,
                           const int32_t* new_of_old_col, int32_t n_cols_old, int32_t* col_out,
                           float* val_out, int64_t nnz_out, void* stream);

/* ---- K19: co-rated neighbours ("who rated X also rated Y": the item-based collaborative
 *      filtering neighbourhood of Sarwar et al. 2001, from the ratings and not the factors;
 *      the reference and Spark have no counterpart) ----------------------------------------- */

/* Added under ABI 9 without a version bump: four new symbols only, nothing existing changes.
 * For each of n_q query rows of one CSR side, the `top` other rows of the SAME side that share
 * the most raters with it: one row of the sparse product B^T B per query, never formed.
 *   queried side  row_ptr_q int64 [n + 1], col_q int32 (dense rows of the other side)
 *   other side    row_ptr_o int64 [n_o + 1], col_o int32 (dense rows of the queried side):
 *                 the two CSR sides K1 builds of one rating set; the values are never read
 *   q_rows        int32 [n_q] dense rows of the queried side; a row outside [0, n) and a row
 *                 without entries get an all-open list; a row given twice gets two lists
 * With n_a the entries of row a, the common count of a pair is
 *   c(a, b) = sum over rows u of the other side of (entries of a by u) x (entries of b by u),
 * duplicate entries counting with their multiplicity (without duplicates: the number of u that
 * rated both).  measure: 0 "count" (float)c; 1 "jaccard" (float)((double)c / (double)(n_a + n_b
 * - c)); 2 "cosine" (float)((double)c / sqrt((double)n_a * (double)n_b)) (set cosine): one fp64
 * expression of three integers, rounded once to fp32.  Row b is listed for query a when
 * b != a (by dense row), c(a, b) >= min_common (>= 1) and bit b of allow_bits is set
 * (als_topk_filtered's mask; NULL: every row).  Order: score descending, then row ascending
 * (the exact 64-bit key of als_topk).  Outputs idx int32, score f32 and common int32 (the
 * count c of each listed row), each [n_q, top]; open slots hold idx -1, score -inf, common 0.
 * Every sum is an integer add (c < 2^31 is the caller's to ensure), so the results are exact
 * and the same bits whatever the launch geometry, `pass`, `task`, or the order workgroups
 * finish in.
 * Queries go through in passes of `pass` (0 = 32; at most 64), each query in flight owning a
 * strip of n int32 counters in the scratch.  A query row is cut into tasks of `task` entries
 * (0 = als_co_rated_task(); at most 2^20), dealt over a fixed grid, so the most-rated row is
 * spread over the device; for each entry u of its task a wavefront walks u's row of the other
 * side and adds 1 per entry to the strip, through K15's direct-mapped LDS cache
 * (als_co_rated_window() slots: an LDS add on a hit, one global add on a miss).  One wavefront
 * per (slice of at least 512 rows, query) then ranks its counters, keeps its `top` best and
 * stores zeros over the counters it has read; a merge launch (two stages past 64 slices)
 * orders the lists.  Non-zero pass / task exist so that tests reach many passes and many
 * tasks at small shapes.
 * Scratch: als_co_rated_scratch_bytes(n, n_q, top, pass) bytes (sized for min(n_q, pass)
 * queries in flight), 16-byte aligned, and it need not be initialised: the call zeroes the
 * strips on entry and every pass leaves them zero, so the strips are zero after the call and
 * no result depends on what the scratch or the outputs held before.  The strips are the first
 * 4 min(n_q, pass) n bytes of the scratch.
 * Checked on the host before any launch: top outside [1, 256], measure outside [0, 3),
 * min_common < 1, pass outside [0, 64], task outside [0, 2^20], a negative size, n or
 * n_o >= 2^31 - 1 and (when n_q > 0) a null q_rows, row pointer, output or misaligned scratch
 * are ALS_EINVAL; a short scratch is ALS_EWORKSPACE; n_q == 0 is a no-op.
 * als_co_rated_scratch_bytes returns 0 for sizes als_co_rated rejects.
 * Cost per query and beside the other routes: DESIGN.md section K19. */
int32_t als_co_rated_task(void);
int32_t als_co_rated_window(void);
size_t als_co_rated_scratch_bytes(int64_t n, int32_t n_q, int32_t top, int32_t pass);
int als_co_rated(const int64_t* row_ptr_q, const int32_t* col_q, int64_t n,
                 const int64_t* row_ptr_o, const int32_t* col_o, int64_t n_o,
                 const int32_t* q_rows, int32_t n_q, int32_t measure, int32_t min_common,
                 const uint32_t* allow_bits, int32_t top, int32_t pass, int32_t task,
                 int32_t* idx, float* score, int32_t* common,
                 void* ws, size_t ws_bytes, void* stream);

/* ---- K20: per-user holdout and stratified folds (leave-k-out, the protocol HR@k, NDCG@k and
 *      MRR are reported under; Spark's randomSplit is a global row split) -------------------- */

/* Added under ABI 9 without a version bump: six new symbols only, nothing existing changes.
 * Which stored entries of a built rating set are held out, from (seed, user id, item id), the
 * rows' eligible sets and a rank window per row; the answer is keep bits in K18's format, so
 * als_csr_remove_compact makes the training side and, from the complement, the held-out triples.
 *   a side      row_ptr int64 [n_rows + 1], col int32 [nnz] (dense rows of the other side, n_cols
 *               of them), row_ids int32 [n_rows] and col_ids int32 [n_cols] the EXTERNAL ids of
 *               the dense rows of this and of the other side; rows_are_users != 0 when this
 *               side's rows are the users
 *   key         (seed: the 64 bits of the int64 argument, as uint64) splitmix64 of x =
 *               (uint64(uint32(user id)) << 32) | uint32(item id):
 *                 z = x + (seed + 1) * 0x9E3779B97F4A7C15
 *                 z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
 *                 z = (z ^ (z >> 27)) * 0x94D049BB133111EB,  key = z ^ (z >> 31)   (mod 2^64)
 *   composite   (key, column), compared lexicographically; "the end" is (2^64 - 1, 2^31 - 1),
 *               above every composite of a stored entry
 * One side SELECTS (its rows have the windows: the users, for a per-user holdout).
 * als_split_anchor runs on the OTHER side and writes
 *   anchor      int32 [n_rows]: the column (a dense row of the selecting side) of the row's
 *               smallest composite, -1 for a row without entries.  The entries (anchor[i], i) —
 *               every stored copy — are not eligible, so no row of the other side loses its last
 *               rating.  A wavefront per row; a row of more than 2048 entries is cut into tiles
 *               whose partial minima go through `scratch` and are merged by the row's wavefront
 * als_split_eligible runs on the selecting side and writes
 *   eligible    int32 [n_rows]: the row's entries that are no anchor (anchor int32 [n_cols], as
 *               als_split_anchor wrote it, or NULL: every entry is eligible).  The caller makes
 *               the windows from it
 * als_split_thresholds runs on the selecting side.  The rank of an eligible entry is the number
 * of eligible entries of its row with a strictly smaller composite, so stored copies of a pair
 * share a rank.  With win_lo, win_hi int32 [n_rows] (a negative rank counts as 0) it writes
 *   thr_lo_key uint64 [n_rows], thr_lo_col int32 [n_rows]: the smallest composite among the
 *               row's eligible entries of rank >= win_lo[r], the end when there is none (always
 *               when win_lo[r] >= eligible[r]); thr_hi_* the same for win_hi.  An eligible entry
 *               has win_lo <= rank < win_hi exactly when thr_lo <= its composite < thr_hi
 *   row_cap     rows of at most row_cap entries (0 = als_split_row_cap(), the largest allowed)
 *               are ranked by one wavefront with the row's composites in LDS, four rows per
 *               workgroup; longer rows are listed in `scratch` and a workgroup per listed row
 *               selects by radix on the key's bytes (eight histogram passes, both ranks at once)
 *               and resolves ties on (key, column) exactly.  No limit on the row length; a small
 *               row_cap exists so that tests reach the long-row path with short rows.  The
 *               outputs do not depend on row_cap
 * als_split_mark runs on EITHER side (selecting != 0: this side's rows have the thresholds and
 * `anchor` is indexed by its columns; selecting == 0: the thresholds are indexed by this side's
 * columns, `anchor` by its rows, and the composite's column is this side's row) and writes
 *   keep_bits, tile_off, row_ptr_kept   exactly as als_csr_remove_mark does, with "stays" =
 *               not (eligible and thr_lo <= composite < thr_hi), tiles of als_csr_remove_tile()
 *               entries.  Both sides mark by one predicate of the pair, so they keep the same
 *               ratings: no delete list, no sort, no host read
 * Scratch: als_split_scratch_bytes(nnz, n_rows) bytes for the side passed, 8-byte aligned; it
 * need not be initialised and no result depends on what it or the outputs held before.  Integer
 * work only; the atomics are integer adds and minima, so two calls give identical bytes.  A
 * column outside [0, n_cols) is never used as an index: the entry is no anchor, not eligible, and
 * stays.  Row positions are clamped to [0, nnz].
 * Checked on the host before any launch: a negative size and a null pointer that would be read
 * or written are ALS_EINVAL, as is row_cap outside [0, als_split_row_cap()]; nnz >= 2^31 or a
 * side of 2^31 - 1 rows (K1's limit) ALS_EUNSUPPORTED; a short scratch ALS_EWORKSPACE.
 * Cost beside the host split it replaces: DESIGN.md section K20. */
int32_t als_split_row_cap(void);
size_t als_split_scratch_bytes(int64_t nnz, int32_t n_rows);
int als_split_anchor(const int64_t* row_ptr, const int32_t* col, int64_t nnz, int32_t n_rows,
                     int32_t n_cols, const int32_t* row_ids, const int32_t* col_ids,
                     int32_t rows_are_users, int64_t seed, int32_t* anchor, void* scratch,
                     size_t scratch_bytes, void* stream);
int als_split_eligible(const int64_t* row_ptr, const int32_t* col, int64_t nnz, int32_t n_rows,
                       int32_t n_cols, const int32_t* anchor, int32_t* eligible, void* stream);
int als_split_thresholds(const int64_t* row_ptr, const int32_t* col, int64_t nnz, int32_t n_rows,
                         int32_t n_cols, const int32_t* row_ids, const int32_t* col_ids,
                         int32_t rows_are_users, int64_t seed, const int32_t* anchor,
                         const int32_t* win_lo, const int32_t* win_hi, int32_t row_cap,
                         uint64_t* thr_lo_key, int32_t* thr_lo_col, uint64_t* thr_hi_key,
                         int32_t* thr_hi_col, void* scratch, size_t scratch_bytes, void* stream);
int als_split_mark(const int64_t* row_ptr, const int32_t* col, int64_t nnz, int32_t n_rows,
                   int32_t n_cols, const int32_t* row_ids, const int32_t* col_ids,
                   int32_t rows_are_users, int64_t seed, int32_t selecting,
                   const uint64_t* thr_lo_key, const int32_t* thr_lo_col,
                   const uint64_t* thr_hi_key, const int32_t* thr_hi_col, const int32_t* anchor,
                   uint64_t* keep_bits, int64_t* tile_off, int64_t* row_ptr_kept, void* scratch,
                   size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ALS_HIP_H */
