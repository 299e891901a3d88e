/*
 * ltrx.h -- C ABI of libltrx.so: MI355X (gfx950) kernels for the listwise-LTR training hot path.
 *
 * This is the drop-in boundary of the engine.  allegro/allRank has no
 * FFI of its own: its plugin surface is Python name lookup (allrank/main.py:75,82-83).  Each entry
 * point below therefore cites the reference *Python* function it replaces; the Python side
 * (allrank_amd/) binds them with ctypes and mirrors the reference signatures one-to-one.
 *
 * Conventions
 *   - plain C types only: device pointers, sizes, scalars; no torch / HIP types in the signatures.
 *     `ltrx_stream_t` is a hipStream_t passed as void* (NULL = the null stream).
 *   - every tensor is caller-owned, dense row-major fp32 unless stated; kernels never allocate, never
 *     retain pointers, never synchronise the device, and enqueue on the given stream only.
 *   - y_true uses `pad_value` (-1 in allRank, allrank/data/dataset_loading.py:15) to mark padded slots.
 *   - re-entrant: no entry point reads or writes process-global mode switches; arithmetic / path / tile choices are
 *     arguments of the call that uses them.  (The only state kept is a per-device "kernel attributes already set" bit.)
 *   - return value: 0 = ok; LTRX_EINVAL bad argument; LTRX_EUNSUPPORTED shape outside the supported
 *     range (slate length above LTRX_MAX_SLATE_LEN for a loss, LTRX_MAX_METRIC_SLATE_LEN for a metric -- the
 *     Python wrappers name the limit in the exception; there is no silent fallback); LTRX_EHIP a HIP launch error (hipGetLastError code is returned as -(1000+code)).
 *   - `batch_divisor`: the number of slates the reference would have averaged over.  On one GPU it is B;
 *     under slate sharding it is the GLOBAL batch so that summing per-rank results reproduces the
 *     reference's loss on the gathered batch.
 *   - sort tie policy: stable descending (lower original index first), SURVEY.md §9.2.
 */
#ifndef LTRX_H
#define LTRX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LTRX_VERSION 130 /* 0.3.0 (round 6): ltrx_first_nonfinite; ltrx_fixlength_positions keys its draw by the slate id (not the batch row) */

#define LTRX_OK 0
#define LTRX_EINVAL (-1)
#define LTRX_EUNSUPPORTED (-2)
#define LTRX_EHIP (-1000)

#define LTRX_MAX_SLATE_LEN 2048        /* the loss kernels' tuned form: a slate and its per-item work arrays in LDS.  Every loss takes slates
                                          up to here; the four hot losses (listNet, listMLE, approxNDCG, lambdaLoss) go on: */
#define LTRX_MAX_LONG_SLATE_LEN 16384  /* ... their work arrays stay in LDS while they fit the CU's 160 KB (listNet: every length, listMLE
                                          6.7 k, approxNDCG 5.8 k, lambdaLoss 3.1 k items) and move to the call's workspace beyond that
                                          (same kernels through a global pointer; *_workspace_bytes(B, L) grows accordingly) -- the
                                          reference pads a validation set to its longest slate, allrank/data/dataset_loading.py:185-194 */
#define LTRX_MHA_DS_BUDGET_BYTES (2147483648ull) /* ltrx_mha_bwd, modes 1 / 2: the dS hand-over workspace is B h LK^2 floats (LK = L rounded
                                                    up to 64); a call that would need more than this runs the exact-fp32 kernels
                                                    (workspace B L h floats) instead -- ltrx_mha_bwd_workspace_bytes says which */
#define LTRX_MAX_METRIC_SLATE_LEN 8192 /* ltrx_ndcg_at / ltrx_mrr_at: validation sets are padded to their longest slate
                                          (allrank/data/dataset_loading.py:185-194); 16 B per item of the 160 KB LDS */

typedef void* ltrx_stream_t;

int ltrx_version(void);

/* ---------------------------------------------------------------------------------------------
 * Listwise losses.  All of them: inputs y_pred[B,L], y_true[B,L]; outputs loss_out[1] (scalar, as the
 * reference returns), optional per_slate_out[B] (the per-slate term before the batch reduction),
 * optional grad_out[B,L] = d loss / d y_pred (exactly 0 at padded slots).  `ws` is a scratch buffer
 * of at least the matching *_workspace_bytes(); it is write-only scratch, contents undefined after.
 * ------------------------------------------------------------------------------------------- */

/* allrank/models/losses/listNet.py:8-30   listNet(y_pred, y_true, eps, padded_value_indicator) */
size_t ltrx_listnet_workspace_bytes(int B, int L);
int ltrx_listnet_fwd_bwd(const float* y_pred, const float* y_true, int B, int L, float eps, float pad_value,
                         float batch_divisor, float* loss_out, float* per_slate_out, float* grad_out, void* ws,
                         ltrx_stream_t stream);

/* allrank/models/losses/listMLE.py:7-38   listMLE(y_pred, y_true, eps, padded_value_indicator)
 * `perm[L]` (int64, device) is the column shuffle the reference draws with torch.randperm (listMLE.py:17);
 * order_out[B,L] (int64, optional) receives the original item index at each sorted position. */
size_t ltrx_listmle_workspace_bytes(int B, int L);
int ltrx_listmle_fwd_bwd(const float* y_pred, const float* y_true, const int64_t* perm, int B, int L, float eps,
                         float pad_value, float batch_divisor, float* loss_out, float* per_slate_out,
                         float* grad_out, int64_t* order_out, void* ws, ltrx_stream_t stream);

/* allrank/models/losses/approxNDCG.py:7-53   approxNDCGLoss(y_pred, y_true, eps, padded_value_indicator, alpha) */
size_t ltrx_approxndcg_workspace_bytes(int B, int L);
int ltrx_approxndcg_fwd_bwd(const float* y_pred, const float* y_true, int B, int L, float eps, float pad_value,
                            float alpha, float batch_divisor, float* loss_out, float* per_slate_out,
                            float* grad_out, void* ws, ltrx_stream_t stream);

/* allrank/models/losses/lambdaLoss.py:7-114   lambdaLoss(y_pred, y_true, eps, padded_value_indicator,
 *                                              weighing_scheme, k, sigma, mu, reduction, reduction_log) */
enum ltrx_lambda_scheme {
  LTRX_SCHEME_NONE = 0,                 /* weighing_scheme=None            (lambdaLoss.py:58-59)  */
  LTRX_SCHEME_NDCGLOSS1 = 1,            /* ndcgLoss1_scheme                (:84-85)               */
  LTRX_SCHEME_NDCGLOSS2 = 2,            /* ndcgLoss2_scheme                (:88-94)               */
  LTRX_SCHEME_LAMBDARANK = 3,           /* lambdaRank_scheme               (:97-98)               */
  LTRX_SCHEME_NDCGLOSS2PP = 4,          /* ndcgLoss2PP_scheme              (:101-102)             */
  LTRX_SCHEME_RANKNET = 5,              /* rankNet_scheme                  (:105-106)             */
  LTRX_SCHEME_RANKNET_GTDIFF = 6,       /* rankNetWeightedByGTDiff_scheme  (:109-110)             */
  LTRX_SCHEME_RANKNET_GTDIFF_POWED = 7  /* rankNetWeightedByGTDiffPowed_scheme (:113-114)         */
};
enum ltrx_reduction { LTRX_REDUCE_SUM = 0, LTRX_REDUCE_MEAN = 1 };
enum ltrx_logbase { LTRX_LOG_BINARY = 0, LTRX_LOG_NATURAL = 1 };
/* k <= 0 means k=None (no truncation).  For LTRX_REDUCE_MEAN the divisor is the number of selected pairs
 * in THIS call's batch; pair_count_out[1] (optional) receives it.  When `ext_pair_count` (device, optional)
 * is given it is used as the divisor instead (global count under slate sharding). */
size_t ltrx_lambdaloss_workspace_bytes(int B, int L);
int ltrx_lambdaloss_fwd_bwd(const float* y_pred, const float* y_true, int B, int L, float eps, float pad_value,
                            int scheme, int k, float sigma, float mu, int reduction, int logbase,
                            const float* ext_pair_count, float* loss_out, float* pair_count_out, float* grad_out,
                            int64_t* order_out, void* ws, ltrx_stream_t stream);

/* allrank/models/losses/neuralNDCG.py:10-70 (neuralNDCG) and :73-136 (neuralNDCG_transposed), deterministic
 * NeuralSort (loss_utils.py:34-67) + Sinkhorn scaling (loss_utils.py:8-31).
 *   step 1  ltrx_neuralndcg_prepare: per-slate ideal DCG@k (metrics.py:41-77 on (y_true,y_true)) and
 *           nonzero_count_out[1] = number of slates with idcg != 0 (the loss normaliser, neuralNDCG.py:69).
 *           Under slate sharding the caller all-reduces nonzero_count between the two steps.
 *   step 2  ltrx_neuralndcg_fwd_bwd: loss and gradient; `nonzero_count` is read from DEVICE memory.
 * transposed != 0 selects the neuralNDCG_transposed conventions (same value; idcg stays "powered" when
 * powered_relevancies == 0, neuralNDCG.py:126).  k <= 0 means k=None.  The Sinkhorn early exit
 * (loss_utils.py:25) is batch-global as in the reference; iters_out[1] (int32, optional) = iterations used.
 * k_rows[B] (int32, device, optional): a per-slate cap on the ranks that carry a discount (min(k, k_rows[b])) -- the
 * stochastic variant (loss_utils.py:84-112) masks the permutation rows by the TRUE slate's padding (neuralNDCG.py:44)
 * while sorting each perturbed copy under another slate's mask (mask.repeat_interleave, :36/:41).
 * path: 0 = automatic (register-resident Sinkhorn kernels when L <= 240), 1 = always the general L2-streaming kernels (same
 * results; a per-call argument so that tests can pin either path without any process state). */
size_t ltrx_neuralndcg_workspace_bytes(int B, int L, int max_iter);
int ltrx_neuralndcg_prepare(const float* y_true, int B, int L, float pad_value, int k, int idcg_powered,
                            float* idcg_out, float* nonzero_count_out, void* ws, ltrx_stream_t stream);
int ltrx_neuralndcg_fwd_bwd(const float* y_pred, const float* y_true, const float* idcg, const float* nonzero_count,
                            int B, int L, float pad_value, float temperature, int powered_relevancies, int k,
                            const int32_t* k_rows, int transposed, int max_iter, float tol, float* loss_out, float* per_slate_out,
                            float* grad_out, int32_t* iters_out, int path, void* ws, ltrx_stream_t stream);

/* Stochastic NeuralSort around the two calls above (loss_utils.py:84-112, neuralNDCG.py:35-47,69): n_samples Gumbel-perturbed
 * copies of every slate run through ltrx_neuralndcg_fwd_bwd as ONE batch of n_samples * B pseudo slates, pseudo slate
 * i = sample * B + b holding the scores of slate b.
 *   ltrx_neuralsort_perturb (after ltrx_neuralndcg_prepare on the B slates): m = min over ALL B * L scores, padded slots included
 *           (:102); s_pos = s + |m|, log(s_pos + 1e-10) with log_scores (:104-105); s_pert[i] = s_pos[b] + beta * g[sample, b].
 *           smin_out[2] = (m, number of elements equal to m).  The reference sorts pseudo slate i under the padding mask of slate
 *           i / n_samples (mask.repeat_interleave, :108) and reads it out with the labels of slate i % B = b; y_ps carries that:
 *           plain: pad_value where slate i / n_samples pads, else the label of slate b where that is valid, else 0, and
 *           k_rows[i] = valid items of slate b; transposed (k_rows is not written): the raw label of slate b wherever slate
 *           i / n_samples is valid, LTRX_NEURALSORT_PAD (-1e30, the pad_value of the following ltrx_neuralndcg_fwd_bwd call) where
 *           it pads.  idcg_ps[i] = idcg[b]; cnt_ps[0] = nonzero_count[0] * n_samples (neuralNDCG.py:69).
 *           Noise: gumbel_in[n_samples,B,L] (optional) is used as given; without it g = -logf(-logf(U + 1e-10) + 1e-10)
 *           (loss_utils.py:70-81) with U = (hash >> 8) * 2^-24, hash = the dropout sites' counter hash of element
 *           (sample * B + b) * L + l under seed ^ (seed_step[0] * 0x9E3779B9) -- a replayed hipGraph draws fresh noise whenever
 *           the device word seed_step[0] (optional) has moved.  gumbel_out[n_samples,B,L] (optional) receives the noise used.
 *   ltrx_neuralsort_fold_grad (after ltrx_neuralndcg_fwd_bwd wrote grad_ps[n_samples*B,L]): gs[b,l] = w[b,l] sum_sample
 *           grad_ps[sample*B+b,l], w = 1 / (s + |m| + 1e-10) with log_scores, else 1; grad_out = gs, and every element with
 *           s == m also gets sign(m) * sum(gs) / smin[1] -- the path through |min(s)|, spread evenly over tied minima as
 *           torch's min() backward does; sign(0) = 0.
 * Both reductions (m with its tie count, sum(gs)) are two-stage and fixed-order: the same inputs and step word give the same
 * bits on every call.  L > LTRX_MAX_SLATE_LEN is unsupported, as for ltrx_neuralndcg_*. */
#define LTRX_NEURALSORT_PAD (-1.0e30f)
size_t ltrx_neuralsort_stoch_workspace_bytes(int B, int L, int n_samples);
int ltrx_neuralsort_perturb(const float* scores, const float* y_true, const float* idcg, const float* nonzero_count, int B, int L,
                            int n_samples, float pad_value, float beta, int log_scores, int transposed, uint32_t seed,
                            const uint32_t* seed_step, const float* gumbel_in, float* s_pert, float* y_ps, int32_t* k_rows,
                            float* idcg_ps, float* cnt_ps, float* smin_out, float* gumbel_out, void* ws, ltrx_stream_t stream);
int ltrx_neuralsort_fold_grad(const float* grad_ps, const float* scores, const float* smin, int B, int L, int n_samples,
                              int log_scores, float* grad_out, void* ws, ltrx_stream_t stream);

/* allrank/models/metrics.py:7-77   ndcg(y_pred, y_true, ats, gain=2^x-1, padding_indicator, filler_value)
 * ats[n_ats] is a HOST array.  ndcg_out[B,n_ats]; dcg_out[B,n_ats] optional; order_out[B,L] (int64, optional)
 * = stable descending argsort of the masked predictions (padded slots last, in original order). */
size_t ltrx_ndcg_workspace_bytes(int B, int L);
int ltrx_ndcg_at(const float* y_pred, const float* y_true, int B, int L, const int* ats, int n_ats,
                 float pad_value, float filler_value, float* ndcg_out, float* dcg_out, int64_t* order_out,
                 void* ws, ltrx_stream_t stream);
/* the same with a caller-supplied gain_function (metrics.py:7-8,41-42,67): gains[B,L] = gain_function evaluated per item on the
 * masked labels (padded items -> label 0 first, metrics.py:35; they then carry gain_function(0) at their tail positions).  Both
 * rankings -- by prediction and the ideal one, which sorts by LABEL (metrics.py:21) -- still come from y_pred / y_true. */
int ltrx_ndcg_at_gains(const float* y_pred, const float* y_true, const float* gains, int B, int L, const int* ats, int n_ats,
                       float pad_value, float filler_value, float* ndcg_out, float* dcg_out, int64_t* order_out,
                       void* ws, ltrx_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Pointwise / pairwise members of allrank.models.losses and MRR.
 * Count-normalised losses follow the lambdaLoss protocol: *_count_out[1] (optional) receives this call's
 * count, ext_*count (device, optional) replaces it as the divisor (global count under slate sharding).
 * ------------------------------------------------------------------------------------------- */

/* allrank/models/losses/rankNet.py:8-79  rankNet / rankNet_weightByGTDiff / rankNet_weightByGTDiff_pow:
 * BCEWithLogits(target 1) over the pairs y_i > y_j of valid items, mean over ALL pairs of the batch.
 * weight_mode 0: unweighted, 1: |y_i - y_j|, 2: |y_i^2 - y_j^2|.  No pair at all -> loss NaN, gradient 0 (torch). */
size_t ltrx_ranknet_workspace_bytes(int B, int L);
int ltrx_ranknet_fwd_bwd(const float* y_pred, const float* y_true, int B, int L, float pad_value, int weight_mode,
                         const float* ext_pair_count, float* loss_out, float* pair_count_out, float* grad_out, void* ws,
                         ltrx_stream_t stream);

/* allrank/models/losses/bce.py:8-32 (n == 0: y_pred[B,L] probabilities, divisor = slates with a valid item) and
 * ordinal.py:8-50 (n >= 1: y_pred[B,L,n], targets [y_true >= k+1], divisor = valid items); torch.nn.BCELoss arithmetic.
 * grad_out has the shape of y_pred. */
size_t ltrx_bce_workspace_bytes(int B, int L, int n);
int ltrx_bce_fwd_bwd(const float* y_pred, const float* y_true, int B, int L, int n, float pad_value, const float* ext_count,
                     float* loss_out, float* count_out, float* grad_out, void* ws, ltrx_stream_t stream);

/* allrank/models/losses/pointwise.py:6-32  pointwise_rmse(y_pred, y_true, no_of_levels) */
size_t ltrx_pointwise_rmse_workspace_bytes(int B, int L);
int ltrx_pointwise_rmse_fwd_bwd(const float* y_pred, const float* y_true, int B, int L, float no_of_levels, float pad_value,
                                float batch_divisor, float* loss_out, float* grad_out, void* ws, ltrx_stream_t stream);

/* allrank/models/losses/binary_listNet.py:8-33 */
size_t ltrx_binary_listnet_workspace_bytes(int B, int L);
int ltrx_binary_listnet_fwd_bwd(const float* y_pred, const float* y_true, int B, int L, float eps, float pad_value,
                                float batch_divisor, float* loss_out, float* grad_out, void* ws, ltrx_stream_t stream);

/* allrank/models/metrics.py:80-113  mrr(y_pred, y_true, ats, padding_indicator): mrr_out[B,n_ats]; ats is a HOST array.
 * Ties in the predictions are ranked by the stable descending order (padded slots last). */
size_t ltrx_mrr_workspace_bytes(int B, int L, int n_ats);
int ltrx_mrr_at(const float* y_pred, const float* y_true, int B, int L, const int* ats, int n_ats, float pad_value,
                float* mrr_out, void* ws, ltrx_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Ragged layout of the listwise losses and metrics (*_cu): a batch evaluated on its valid items only, as ltrx_mha_fwd takes it.
 *   - y_pred[n], y_true[n], grad_out[n] (and order_out[n]) hold only valid items; slate b is rows cu_seqlens[b] .. cu_seqlens[b+1]-1,
 *     cu_seqlens = i32[B+1] in device memory, n = cu_seqlens[B].  Every packed row is valid: there is no pad_value, and no label
 *     is compared with one.
 *   - slate_order (i32[B] in device memory, or NULL): the launch order of the slates -- longest first balances the CUs; results
 *     do not depend on it.
 *   - max_len (host): an upper bound of every slate's length in the call.  It sizes the work arrays (LDS, or the workspace beyond
 *     the CU's 160 KB), the workspace is the padded namesake's *_workspace_bytes(B, max_len), and the limits apply to it:
 *     LTRX_MAX_LONG_SLATE_LEN for the losses, LTRX_MAX_METRIC_SLATE_LEN for the metrics, LTRX_EUNSUPPORTED beyond.  A slate longer
 *     than max_len is the caller's error; it is evaluated as its first max_len items, so no access leaves the call's buffers.
 *   - a slate of length 0 is legal and gives what the padded call gives for a fully padded slate: loss contribution 0 (listNet,
 *     approxNDCG, lambdaLoss: no pair), ndcg = filler_value, dcg = 0, and for mrr the first maximum (label 0 at rank 0), i.e. the
 *     reciprocal rank 1 that metrics.py:100-107 gives a slate without relevant items, subject to the batch-wide rule below.
 *   - contract: each call returns what its padded namesake returns on the [B, L] grid that holds every slate's items first and
 *     pad_value after them, for any L >= max_len (same kernel bodies, loops bounded by the slate's length instead of L).
 *     per_slate_out[B], ndcg_out / dcg_out / mrr_out[B, n_ats] are indexed by slate; order_out[n] (int64) holds, at each sorted
 *     position of a slate's rows, the item's index INSIDE its slate.  Other arguments as in the padded call.
 * ------------------------------------------------------------------------------------------- */
int ltrx_listnet_fwd_bwd_cu(const float* y_pred, const float* y_true, const int32_t* cu_seqlens, const int32_t* slate_order, int B,
                            int max_len, float eps, float batch_divisor, float* loss_out, float* per_slate_out, float* grad_out,
                            void* ws, ltrx_stream_t stream);
int ltrx_approxndcg_fwd_bwd_cu(const float* y_pred, const float* y_true, const int32_t* cu_seqlens, const int32_t* slate_order, int B,
                               int max_len, float eps, float alpha, float batch_divisor, float* loss_out, float* per_slate_out,
                               float* grad_out, void* ws, ltrx_stream_t stream);
int ltrx_lambdaloss_fwd_bwd_cu(const float* y_pred, const float* y_true, const int32_t* cu_seqlens, const int32_t* slate_order, int B,
                               int max_len, float eps, int scheme, int k, float sigma, float mu, int reduction, int logbase,
                               const float* ext_pair_count, float* loss_out, float* pair_count_out, float* grad_out,
                               int64_t* order_out, void* ws, ltrx_stream_t stream);
/* default gain 2^y - 1 (a caller-supplied gain_function has no ragged form); ats[i] above a slate's length counts as its length */
int ltrx_ndcg_at_cu(const float* y_pred, const float* y_true, const int32_t* cu_seqlens, const int32_t* slate_order, int B,
                    int max_len, const int* ats, int n_ats, float filler_value, float* ndcg_out, float* dcg_out, int64_t* order_out,
                    void* ws, ltrx_stream_t stream);
/* the batch-wide rule of metrics.py:108-109 (sum of the slates' maximum labels == 0 -> all zeros) is kept; ws: ltrx_mrr_workspace_bytes */
int ltrx_mrr_at_cu(const float* y_pred, const float* y_true, const int32_t* cu_seqlens, const int32_t* slate_order, int B, int max_len,
                   const int* ats, int n_ats, float* mrr_out, void* ws, ltrx_stream_t stream);
/* allrank/inference/inference_utils.py:51-56 (padded scores to -inf, sort descending, gather X and y): the slates of a ragged batch in
 * ranked order, padded to L >= max_len items.  scores[n] = the packed scores of the valid items.  The item rows come from ONE of two
 * sources, chosen by which pointers are non-NULL:
 *   grid:      x[B, L, F], y[B, L] -- the padded batch the scores were computed from, valid items first in every slate;
 *   resident:  x_items, y_items, offsets of a CSR set resident in HBM (ltrx_assemble_batch's arrays) and ids[B] (int64, device), the
 *              slates of the batch: item i of slate b is row offsets[ids[b]] + i.  No padded copy of the features is read.
 * perm[n] (int32, optional): perm[cu[b] + r] = the index inside slate b of the item ranked r.  x_out[B, L, F]: row r < len_b of slate b
 * is source row perm[cu[b] + r], bit for bit, rows r >= len_b are 0.0f; y_out[B, L]: the labels in the same order, -1.0f behind them.
 * Order: the stable descending policy above -- rank of item i = #{ j : s_j > s_i, or s_j == s_i and j < i } (-0.0 == +0.0 ties, +-inf
 * order as floats).  The reference's torch.sort(descending=True) is NOT stable: its order on exact ties is undefined, this call defines
 * it.  NaN scores: the slate's order is unspecified, every output element is still written (tail values where no item landed), and
 * no access leaves the slate's rows.  Outputs must not overlap inputs.  16-byte accesses where F % 4 == 0 and the source and x_out
 * are 16-byte aligned, 4-byte accesses otherwise.  HBM per slate: len F floats read, L F written.
 * NULL scores / cu_seqlens / x_out / y_out, B, F, max_len <= 0, L < max_len, both source forms, none or an incomplete one:
 * LTRX_EINVAL; max_len > LTRX_MAX_METRIC_SLATE_LEN: LTRX_EUNSUPPORTED; a refused call writes nothing.  allrank_amd/csrc/ltrx_rank.hip. */
int ltrx_rank_slates_cu(const float* scores, const float* x, const float* y, const float* x_items, const float* y_items,
                        const int64_t* offsets, const int64_t* ids, const int32_t* cu_seqlens, const int32_t* slate_order, int B,
                        int max_len, int F, int L, int32_t* perm, float* x_out, float* y_out, ltrx_stream_t stream);

/* allrank/click_models (behind rank_and_click.py:88): clicks on ranked slates -- BaseCascadeModel / OnlyRelevantClickModel, optionally
 * inside MaxClicksModel, inside DiverseClicksModel, inside MaxClicksModel.  allrank_amd/csrc/ltrx_click.hip.
 *   x[B, L, F], y[B, L]: the padded ranked slates, valid items first (what ltrx_rank_slates_cu writes); cu_seqlens gives the item counts
 *   and the packed offsets of u; slate_order, max_len as in the ragged layout above.
 *   u[n] (fp64, device, or NULL): one uniform per valid item, in slate order; observe_p[max_len] (fp64, device, or NULL): the observation
 *   probability of each position.  Both or neither.
 *   q_host: a HOST pointer to the quantile (read before the launch; needed with `diverse` only).
 *   clicks_out[B, L]: 1.0f / 0.0f on valid items, -1.0f behind them.  margin_out[B] (fp64, or NULL): the slate's duplicate margin (0 without
 *   `diverse`).
 * Per slate of n items, in the reference's order of operations:
 *   1. item i is observed iff observe_p[i] >= u[cu[b] + i] (both NULL: every item is); a candidate is an item with
 *      (observed ? y_i : 0.0f) >= threshold -- an unobserved item is a candidate when threshold <= 0, as in the reference;
 *   2. max_candidates >= 0 keeps the first max_candidates candidates (MaxClicksModel inside the diverse model: cumsum <= max);
 *   3. diverse != 0: the margin is the q quantile of the n (n - 1) / 2 pairwise Euclidean distances of the valid rows by numpy's linear
 *      rule -- v = q (N - 1), lo = floor(v), hi = min(lo + 1, N - 1), t = v - lo, a + (b - a) t for t < 0.5, else b - (b - a)(1 - t), every
 *      operation rounded on its own; 0 for n <= 1.  Candidates are visited in rank order: one is clicked iff its distance to EVERY item
 *      clicked so far is > margin, any other is dropped;
 *   4. max_clicks >= 0 keeps the first max_clicks clicks (MaxClicksModel outside).
 * Distance arithmetic is part of the contract: sqrt(sum_k (double(a_k) - double(b_k))^2) in fp64, k ascending, no fused multiply-add,
 * a correctly rounded root, stated once in the kernel; the stored value serves the quantile and the comparisons alike; symmetric in
 * the pair.  For an odd pair count the margin IS one of the distances and that pair compares equal to it.  No floating-point atomics: the
 * same bits on every call.  With margin_out NULL a slate with fewer than two candidates skips its distance work (no comparison can
 * change its result).
 * Distances stay in LDS for slates of up to LTRX_CLICK_LDS_SLATE_LEN items; a longer slate uses its workgroup's slab of ws.  At most
 * LTRX_CLICK_SLAB_WORKGROUPS workgroups run such a call and the slates stride over them, so
 *   ltrx_click_workspace_bytes = min(B, LTRX_CLICK_SLAB_WORKGROUPS) * max_len (max_len - 1) / 2 * 8 bytes
 * for diverse calls with max_len > LTRX_CLICK_LDS_SLATE_LEN, 0 otherwise: bounded whatever B is (2.1 GB at LTRX_MAX_SLATE_LEN).
 * Refused before any HIP call, nothing written -- LTRX_EINVAL: NULL x / y / cu_seqlens / clicks_out; B, F or max_len <= 0; L < max_len;
 * exactly one of u / observe_p; diverse without q_host; q outside [0, 1]; ws NULL where the size query is non-zero.
 * LTRX_EUNSUPPORTED: max_len > LTRX_MAX_SLATE_LEN with diverse (a slab would be 16.8 MB per workgroup), > LTRX_MAX_METRIC_SLATE_LEN
 * without. */
#define LTRX_CLICK_LDS_SLATE_LEN 176
#define LTRX_CLICK_SLAB_WORKGROUPS 128
size_t ltrx_click_workspace_bytes(int B, int max_len, int diverse);
int ltrx_click_slates_cu(const float* x, const float* y, const int32_t* cu_seqlens, const int32_t* slate_order, int B, int max_len,
                         int F, int L, const double* u, const double* observe_p, float threshold, int max_candidates, int diverse,
                         const double* q_host, int max_clicks, float* clicks_out, double* margin_out, void* ws, ltrx_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Scoring model kernels (allrank/models/transformer.py).
 * ------------------------------------------------------------------------------------------- */

/* transformer.py:59-81  custom LayerNorm: y = a*(x-mean)/(std_unbiased+eps)+b over the last dim D, with an
 * optional fused residual input (transformer.py:105: the sum x + sublayer(...) that feeds the next norm):
 *   xsum = x (+ res);  y = LN(xsum).   xsum_out may be NULL when res is NULL.
 * Saves mean[rows], rstd[rows] (= 1/(std+eps)) for the backward.  res_drop_p > 0 applies the SublayerConnection dropout
 * (transformer.py:105) to the residual branch inside the add: xsum = x + drop(res), counter-based mask keyed by
 * drop_seed ^ hash(drop_step[0]) (drop_step may be NULL); the backward of the branch is ltrx_dropout_apply. */
int ltrx_layernorm_fwd(const float* x, const float* res, const float* a, const float* b, int rows, int D, float eps,
                       float* xsum_out, float* y_out, float* mean_out, float* rstd_out, float res_drop_p, uint32_t drop_seed,
                       const uint32_t* drop_step, ltrx_stream_t stream);
/* dx = LN backward of dy (+ dres_in if given: the gradient arriving through the residual branch);
 * da_out/db_out (fp32, length D) are written via a deterministic two-stage reduction through ws. */
size_t ltrx_layernorm_bwd_workspace_bytes(int rows, int D);
int ltrx_layernorm_bwd(const float* dy, const float* xsum, const float* a, const float* mean, const float* rstd,
                       const float* dres_in, int rows, int D, float eps, float* dx_out, float* da_out, float* db_out,
                       void* ws, ltrx_stream_t stream);
/* ltrx_layernorm_bwd without the parameter-gradient reduction: dx_out is final; ws holds *partial_rows_out rows of [da(D) | db(D)]
 * partials (row stride 2 D) that the caller sums, e.g. as two entries of ltrx_reduce_group. */
int ltrx_layernorm_bwd_partial(const float* dy, const float* xsum, const float* a, const float* mean, const float* rstd,
                               const float* dres_in, int rows, int D, float eps, float* dx_out, void* ws, int* partial_rows_out,
                               ltrx_stream_t stream);

/* The encoder's final norm and the d_output == 1 score head (model.py:111-117) without the normalised rows or their gradient ds * w
 * in memory.  D % 256 == 0, D <= 1024 and 16-byte aligned row / parameter pointers, else LTRX_EUNSUPPORTED (the caller keeps
 * ltrx_layernorm_* + ltrx_score_head_*).  Every output has the bits the two-kernel sequence gives it.
 * Forward: mean_out / rstd_out as ltrx_layernorm_fwd saves them, scores_out[r] = <LN(x[r]), w> + bias[0] as ltrx_score_head_fwd
 * computes it on ltrx_layernorm_fwd's output; y_out (may be NULL) receives LN(x).
 * Backward: dx_out = what ltrx_score_head_bwd followed by ltrx_layernorm_bwd_partial (dres_in NULL) writes; ws (at least
 * ltrx_norm_head_bwd_workspace_bytes) holds *partial_rows_out rows of [da(D) | db(D)] partials, row stride 2 D, as
 * ltrx_layernorm_bwd_partial leaves them for ltrx_reduce_group.
 * ltrx_norm_head_wgrad: the head's own gradients dw[D], db[1] of ltrx_score_head_bwd, with its input LN(xsum) recomputed from xsum
 * and the saved statistics in that call's row order; ws: ltrx_score_head_bwd_workspace_bytes(M, D). */
int ltrx_norm_head_fwd(const float* x, const float* a, const float* b, const float* w, const float* bias, int rows, int D, float eps,
                       float* scores_out, float* mean_out, float* rstd_out, float* y_out, ltrx_stream_t stream);
size_t ltrx_norm_head_bwd_workspace_bytes(int rows, int D);
int ltrx_norm_head_bwd_partial(const float* dscores, const float* xsum, const float* a, const float* w, const float* mean,
                               const float* rstd, int rows, int D, float eps, float* dx_out, void* ws, int* partial_rows_out,
                               ltrx_stream_t stream);
int ltrx_norm_head_wgrad(const float* dscores, const float* xsum, const float* a, const float* b, const float* mean, const float* rstd,
                         int M, int D, float* dw, float* db, void* ws, ltrx_stream_t stream);

/* transformer.py:137-156 attention() as used by MultiHeadedAttention.forward (:178-203), fused flash-style:
 * q,k,v,o are [B, L, h, d_k] views of the projection outputs (element (b,l,head,c) at ((b*L+l)*h+head)*d_k + c
 * scaled by the given row stride), key_pad_mask u8[B,L] (1 = padded key, filled with -inf, transformer.py:150-151);
 * softmax over keys; dropout on the probabilities (transformer.py:154-155) with rate p_drop (0 = off) from a counter-
 * based generator keyed by `seed` (the backward must be given the same p_drop and seed; the stream differs from torch's
 * Philox, equivalence is statistical).  lse_out[B,h,L] = log-sum-exp of the
 * scaled, masked scores (the only tensor saved for backward).  fp32 in/out; contractions on the fp32 MFMA
 * (v_mfma_f32_32x32x2_f32), exact fp32 products.  d_k % 4 == 0, d_k <= 128 (zero-padded to a multiple of 32).
 * cu_seqlens (i32[B+1] in device memory, or NULL): variable-length layout -- slate b occupies rows cu[b] .. cu[b+1]-1 of
 * q/k/v/o (its valid items packed: ltrx_gather_rows from a row index, ltrx_gather_rows_cu from cu_seqlens itself), L is then only the maximum slate length (grid size and the stride of
 * lse / delta); key_pad_mask may be NULL in that layout (every packed row is a valid key).
 * slate_order (i32[B] in device memory, or NULL): a permutation of the slates giving the order in which their workgroups are
 * launched -- longest first balances the CUs on ragged batches; results do not depend on it. */
/* `mode` = arithmetic of the attention contractions OF THIS CALL (the library keeps no mode; the backward must be given the
 * mode of its forward): 1 = split-bf16 on the bf16 MFMA (3 products per fp32 product, fp32-class,
 * like the dense projections) on the LDS-resident kernels, used wherever the shape fits (any slate length -- the forward streams
 * the keys through a ring in LDS; the backward up to LTRX_MAX_SLATE_LEN --, 32 < d_k <= 64; dropout and variable-length batches included); 0 = exact fp32 MFMA (bit-exact fp32 products) for every
 * shape -- the strict reference; 2 = the kernels of mode 1 with ONE bf16 product per contraction (plain-bf16 throughput mode,
 * about 2^-9 relative error per product: outside the parity contract, reported separately by bench.py).  Shapes that do not
 * fit always run the exact kernels. */
#define LTRX_MHA_EXACT_FP32 0
#define LTRX_MHA_SPLIT_BF16 1
#define LTRX_MHA_PLAIN_BF16 2
int ltrx_mha_fwd(const float* q, const float* k, const float* v, const uint8_t* key_pad_mask, int B, int L, int h,
                 int d_k, int row_stride, float* o, int o_row_stride, float* lse_out, float p_drop, uint32_t seed,
                 const uint32_t* seed_step, const int32_t* cu_seqlens, const int32_t* slate_order, int mode,
                 ltrx_stream_t stream);
/* backward: dq,dk,dv from do.  `ws` holds delta[B,h,L] (rowsum(do*o)) for the exact kernels, or -- in modes 1 / 2 where the
 * LDS-resident kernels run (32 < d_k <= 64, L <= LTRX_MAX_SLATE_LEN) -- the dS exchange between the two backward kernels,
 * B*h*LK*LK floats with LK = L rounded up to 64: S, P, dP and delta are computed once, by the dK/dV kernel, which hands dS to a
 * dQ = dS K kernel through HBM (deterministic, no atomics).  Size it with ltrx_mha_bwd_workspace_bytes for the SAME (d_k, mode)
 * the call will use. */
size_t ltrx_mha_bwd_workspace_bytes(int B, int L, int h, int d_k, int mode);
/* 1 when ltrx_mha_fwd / ltrx_mha_bwd take heads of d_k columns (d_k % 4 == 0, d_k <= 128), else 0: they return LTRX_EUNSUPPORTED.  Host only. */
int ltrx_mha_head_width_supported(int d_k);
int ltrx_mha_bwd(const float* q, const float* k, const float* v, const uint8_t* key_pad_mask, const float* o,
                 const float* dout, const float* lse, int B, int L, int h, int d_k, int row_stride, int o_row_stride,
                 float* dq, float* dk, float* dv, int d_row_stride, float p_drop, uint32_t seed,
                 const uint32_t* seed_step, const int32_t* cu_seqlens, const int32_t* slate_order, int mode, void* ws,
                 ltrx_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Training-step glue (allrank/training/train_utils.py:18-29 around the model): the pieces between the library
 * GEMMs that the explicit, graph-capturable step of allrank_amd/engine.py needs.
 * ------------------------------------------------------------------------------------------- */

/* The optimizers `getattr(torch.optim, config.optimizer.name)` (allrank/main.py:82) resolves to in practice, over one flat fp32
 * buffer of n elements.  ltrx_adam_step = torch.optim.Adam.step (Adam in every shipped config; weight_decay = the L2 term added to
 * the gradient) or, with decoupled != 0, torch.optim.AdamW.step (p *= 1 - lr * weight_decay first): step_count[1] (device, float) is
 * incremented first and used for the bias corrections.  ltrx_sgd_step = torch.optim.SGD.step with dampening 0 (momentum_buf may be
 * NULL when momentum == 0).  Gradients are multiplied by grad_scale (1.0 normally) and, when given, by grad_scale_dev[0] (device; the
 * clipping coefficient) on the fly.  (amsgrad / maximize / foreach variants: not implemented -- the Python layer keeps those jobs
 * on torch's optimizer.)
 * lr, the betas, eps and weight_decay arrive as fp32 and the bias corrections 1 - beta^t are computed in fp32 (powf) from the device
 * step count: against the same rule in fp64 one update is off by the usual few roundings plus about
 * 2 u (beta1^t / (1 - beta1^t) + beta2^t / (2 (1 - beta2^t))) of the update, u = 2^-24 -- about 1000 u at t = 1 and 500 u at t = 2 for
 * beta2 = 0.999, under 2 u from t = 693 on (tests/step_ref.py derives and tests/test_gpu_step_kernels.py holds that bound).
 * torch keeps the same hyperparameters as doubles; MEASURED, typical, not a bound: with the default betas and random gradients the
 * largest relative difference of one parameter update between the two over 1,000 steps is 1.6e-5 (it is float(0.999f) != 0.999 in
 * 1 - beta2; tests/test_step_ref_cpu.py prints the figure and does not assert it). */
int ltrx_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, size_t n, float lr, float beta1,
                   float beta2, float eps, float weight_decay, int decoupled, float* step_count, float grad_scale,
                   const float* grad_scale_dev, ltrx_stream_t stream);
int ltrx_sgd_step(float* params, const float* grads, float* momentum_buf, size_t n, float lr, float momentum, int nesterov,
                  float weight_decay, float grad_scale, const float* grad_scale_dev, ltrx_stream_t stream);

/* torch.nn.utils.clip_grad_norm_ (allrank/training/train_utils.py:24-25) over the flat gradient buffer:
 * scale_out[0] = min(1, max_norm / (||grads||_2 + 1e-6)), norm_out[0] (optional) = the norm; deterministic two-stage sum. */
size_t ltrx_clip_workspace_bytes(size_t n);
int ltrx_clip_grad_norm_scale(const float* grads, size_t n, float max_norm, float* scale_out, float* norm_out, void* ws,
                              ltrx_stream_t stream);

/* nn.Linear bias gradient: out[n] (+)= sum_m a[m*ld + n] for a row-major [M,N] matrix; deterministic two-stage. */
size_t ltrx_colsum_workspace_bytes(int M, int N);
int ltrx_colsum(const float* a, int M, int N, int ld, float* out, int accumulate, void* ws, ltrx_stream_t stream);

/* ReLU backward in place (transformer.py:227, FCModel activation): dr[i] = r[i] > 0 ? dr[i] * scale : 0; n % 4 == 0. */
int ltrx_relu_bwd(float* dr_inout, const float* r_post_act, size_t n, float scale, ltrx_stream_t stream);

/* dropout plumbing of the explicit step: dst[i] = src[i] * keep_scale(i) with the same counter-based mask the forward
 * kernels use (seed ^ hash(step[0])); ltrx_bump_u32 advances the per-step word (so a replayed hipGraph re-keys). */
int ltrx_dropout_apply(const float* src, float* dst, size_t n, float p, uint32_t seed, const uint32_t* drop_step,
                       ltrx_stream_t stream);
int ltrx_bump_u32(uint32_t* word, ltrx_stream_t stream);

/* Finiteness check of the explicit step -- the replacement of torch.autograd.detect_anomaly() (allrank/main.py:89,
 * config.detect_anomaly, config.py:77) for a step that has no autograd graph: scans buf[0..n) (the flat gradient buffer; 16-byte
 * aligned) once and writes out[0] = index of the first segment that holds a NaN / Inf (segment s = [seg_start[s], seg_start[s+1]),
 * seg_start sorted ascending, seg_start[0] = 0: the parameter tensors in flat-buffer order), 0x7fffffff if every element is finite;
 * out[1] = number of non-finite elements.  HBM-bound, 4 B per element.  allrank_amd/csrc/ltrx_train.hip. */
int ltrx_first_nonfinite(const float* buf, size_t n, const int64_t* seg_start, int n_seg, int* out, ltrx_stream_t stream);

/* all transposed weight copies of the explicit step in one launch: matrix m = rows x cols floats at src_base + desc[4m],
 * written transposed (cols x rows) at dst_base + desc[4m+1]; desc[4m+2..3] = rows, cols; tile_start[n+1] = prefix sums of
 * ceil(rows/32)*ceil(cols/32) (all arrays in DEVICE memory except the scalars). */
int ltrx_transpose_batch(const float* src_base, float* dst_base, const int64_t* desc, const int32_t* tile_start, int n,
                         int total_tiles, ltrx_stream_t stream);

/* Compacted (variable-length) batches: pack the valid items of a padded [B, L] batch (dataset.py:28-38 pads with -1 rows)
 * into consecutive rows and back.  gather: dst[i,:] = src[idx[i],:] for i < n, zero rows for n <= i < n_pad;
 * scatter: dst[idx[i],:] = src[i,:] for i < n.  idx in DEVICE memory. */
int ltrx_gather_rows(const float* src, int ld_src, const int32_t* idx, int n, int n_pad, int cols, float* dst, int ld_dst,
                     ltrx_stream_t stream);
/* idx[r] = b*L + (r - cu[b]) for packed row r of slate b (valid items first in every slate); n = cu[B]. */
int ltrx_packed_row_index(const int32_t* cu_seqlens, int B, int L, int n, int32_t* idx, ltrx_stream_t stream);
int ltrx_scatter_rows(const float* src, int ld_src, const int32_t* idx, int n, int cols, float* dst, int ld_dst,
                      ltrx_stream_t stream);

/* Packed batches whose row count lives in DEVICE memory (graph-replayable: no launch argument depends on the batch).
 * n = cu_seqlens[B] (i32[B+1], device memory; slate b = packed rows cu[b] .. cu[b+1]-1, cu[b+1]-cu[b] <= L); `rows` >= n is the
 * host row bucket the outputs hold.  Rows move as 32-bit words, 16 bytes per access when cols / strides / addresses allow.
 *   ltrx_assemble_packed: from a CSR set resident in HBM (ltrx_assemble_batch's arrays) and B slate ids: x_out[r, :F] = the
 *       features of item j of slate b for r = cu[b] + j < n, zero rows for n <= r < rows (columns F .. ld_x-1 untouched);
 *       y_out[B, L] = labels, -1 on padding; idx_out[r] = b*L + j and pos_out[r] = j (both -1 for r >= n; either may be NULL).
 *       The padding branch of FixLength followed by packing.
 *   ltrx_gather_rows_cu: the same packing of a padded batch src[B', L, ld_src] (valid items first in every slate; slates past
 *       B' must have length 0): dst[r] = src[b*L + j] for r < n, zero for n <= r < rows; idx_out (or NULL) as above.
 *   ltrx_scatter_rows_cu: dst[b*L + j] = src[cu[b] + j] for j < cu[b+1]-cu[b] (and cu[b] + j < rows), 0 in every other slot
 *       of dst[B, L, ld_dst].
 *   ltrx_zero_rows_cu: x[r, 0 .. cols-1] = 0 for the alignment rows n <= r < rows of a row-major buffer with row stride ld
 *       (columns cols .. ld-1 and the rows below n untouched; nothing when n >= rows).  16-byte stores where x, ld and cols
 *       allow, 4-byte stores otherwise.  NULL pointers, B, rows, cols <= 0 or ld < cols: LTRX_EINVAL, nothing is written. */
int ltrx_assemble_packed(const float* x_items, const float* y_items, const int64_t* offsets, const int64_t* slates,
                         const int32_t* cu_seqlens, int B, int L, int F, int rows, float* x_out, int ld_x, float* y_out,
                         int32_t* idx_out, int64_t* pos_out, ltrx_stream_t stream);
int ltrx_gather_rows_cu(const float* src, int ld_src, const int32_t* cu_seqlens, int B, int L, int cols, int rows, float* dst,
                        int ld_dst, int32_t* idx_out, ltrx_stream_t stream);
int ltrx_scatter_rows_cu(const float* src, int ld_src, const int32_t* cu_seqlens, int B, int L, int cols, int rows, float* dst,
                         int ld_dst, ltrx_stream_t stream);
int ltrx_zero_rows_cu(float* x, int ld, int cols, const int32_t* cu_seqlens, int B, int rows, ltrx_stream_t stream);

/* OutputLayer with d_output == 1 (model.py:111-117): scores[m] = <x[m,:], w> + b, and its backward
 * (dx[m,:] = dscores[m] * w; dw = sum_m dscores[m] x[m,:]; db = sum_m dscores[m]). */
int ltrx_score_head_fwd(const float* x, const float* w, const float* b, int M, int D, float* scores, ltrx_stream_t stream);
size_t ltrx_score_head_bwd_workspace_bytes(int M, int D);
int ltrx_score_head_bwd(const float* dscores, const float* x, const float* w, int M, int D, float* dx, float* dw,
                        float* db, void* ws, ltrx_stream_t stream);

/* fp32-accurate dense projections on the bf16 matrix cores ("split-bf16": each fp32 operand is split into bf16 hi + lo
 * while staged into LDS; A B^T ~= Ahi Bhi^T + Ahi Blo^T + Alo Bhi^T with fp32 accumulation).  `strict` is the precision
 * code of a call: 0 = the three products above (parity arithmetic, default); 1 = a 3-term split and 6 products (true-fp32
 * error); 2 = ONE product Ahi Bhi^T (plain bf16 operands, fp32 accumulate: the throughput mode, about 2^-9 relative error
 * per product -- outside the parity contract, reported separately by bench.py).
 * Error of the split itself, per product and hence per entry relative to sum_k |a||b| (bf16: 8 significand bits, unit round-off 2^-8;
 * derived and proved on operands spanning 2^+-46 in tests/test_split_bf16_cpu.py), on top of the fp32 accumulation:
 *   code 0: BOUND 3 * 2^-16 (1 + 2^-7) = 4.6e-5, typical 3 * 2^-18;   code 1: BOUND 4 * 2^-24 (1 + 2^-7) = 2.4e-7, typical 2^-26;
 *   code 2: BOUND 2 * 2^-8 (1 + 2^-8) = 7.8e-3, typical 2^-9.
 * Replaces the nn.Linear GEMMs of model.py:35-44 and transformer.py:193-203,221-227.
 *   ltrx_gemm_nt: C[M,N] (ld ldc) = epi( A[M,K] (ld lda) * B[N,K]^T (ld ldb) + bias[N] )
 *                 -- forward (B = weight) and input gradient (B = weight^T);  K, lda, ldb multiples of 4.
 *                 epilogue `act`: 0 none, 1 ReLU (transformer.py:227 fused), 2 multiply by (aux[m,n] > 0): the ReLU
 *                 backward fused into the input-gradient GEMM (aux = the saved post-activation tensor, ld ldaux);
 *                 3 add aux[m,n] AFTER the dropout: C = aux + drop_p(A B^T + bias), the residual connection of
 *                 SublayerConnection (transformer.py:98-106) written by the projection that closes the sublayer.
 *                 4 / 5: the ReLU and its backward with the mask carried as ONE BIT per element: act 4 = act 1 that also writes
 *                 the mask (of the post-dropout activation) to aux, act 5 = act 2 reading that mask instead of the fp32 activation
 *                 (aux = a 16-byte aligned buffer of ltrx_gemm_nt_relu_bits_bytes(M, N, K) bytes, ldaux ignored; both launches must
 *                 have the same M and N, and the function must be non-zero for the K of EACH launch: N % 256 == 0, K % 32 == 0 and a
 *                 tile count the large-tile kernel takes; LTRX_EUNSUPPORTED where it returns 0 -- use acts 1 / 2 there).  Same results as acts 1 / 2.
 *                 drop_p > 0: nn.Dropout after the activation (model.py:43, transformer.py:227) fused in the epilogue
 *                 (act 0/1: counter-based mask over the [M,N] output; act 2: the mask is carried by aux, only 1/(1-p)).
 *   ltrx_gemm_tn: C[NP,KP] (dense) = A[M,NP]^T * B[M,KP]  -- weight gradient dW = dY^T X (split over M, deterministic);
 *                 bias_out[NP] (optional) = column sums of A = the bias gradient, produced in the same pass. */
size_t ltrx_gemm_nt_relu_bits_bytes(int M, int N, int K);
int ltrx_gemm_nt(const float* A, int lda, const float* B, int ldb, const void* B_image, float* C, int ldc, int M, int N, int K, const float* bias,
                 int act, const float* aux, int ldaux, float drop_p, uint32_t drop_seed, const uint32_t* drop_step, int strict,
                 int tile, ltrx_stream_t stream);
/* B_image (optional, NULL = none): the operand B pre-split by ltrx_split_image -- every 4 consecutive floats of B replaced, at the
 * same address offset, by the 16 bytes {hi0..hi3, lo0..lo3} of their bf16 hi / lo split.  The large-tile kernels then copy B into LDS
 * instead of splitting it on the fly (identical bits, identical results, less VALU work); other kernels ignore it and read B.  What it
 * is for: nn.Linear weights (model.py:35-44, transformer.py:193-227) change once per optimizer step but are staged by every tile of
 * every GEMM of the step.  ltrx_split_image: n floats (multiple of 4), src and dst 16-byte aligned. */
int ltrx_split_image(const float* src, void* dst, size_t n, ltrx_stream_t stream);
/* The engine's whole per-step weight refresh in one launch: the image of the flat parameter buffer (src_base[0..nflat) -> src_image,
 * as ltrx_split_image) and, for the n matrices of desc / tile_start (as ltrx_transpose_batch), the transposed fp32 copy in dst_base
 * AND its image in dst_image (same offsets).  Requires nflat % 4 == 0, 16-byte aligned buffers, 4-float aligned dst offsets and
 * rows % 4 == 0 for every matrix.  Bit-identical to ltrx_transpose_batch + 2 x ltrx_split_image.
 * ENGINE-INTERNAL: desc / tile_start are DEVICE tables, so the call can check the host-visible preconditions only (pointers, nflat % 4,
 * 16-byte alignment of the five buffers); the per-matrix ones -- rows % 4 == 0, dst offset % 4 == 0 -- are the caller's contract
 * (allrank_amd/engine.py `_fused_images` verifies them when it builds the table, and uses ltrx_transpose_batch + ltrx_split_image
 * otherwise).  A table that violates them yields float4 stores that straddle rows: silent corruption of the copies, never a fault
 * outside the buffers.  Other callers should use the two public calls it fuses. */
int ltrx_weight_images(const float* src_base, size_t nflat, void* src_image, float* dst_base, void* dst_image, const int64_t* desc,
                       const int32_t* tile_start, int n, int total_tiles, const float* pad_src, int pad_rows, int pad_cols, int pad_ld,
                       float* pad_dst, void* pad_dst_image, ltrx_stream_t stream);
/*   pad_src (optional, NULL = none): one more matrix [pad_rows][pad_cols] copied to pad_dst[pad_rows][pad_ld] (fp32) and
 *   pad_dst_image (its image) in the same launch -- the engine keeps the first FC weight [H, F] with rows of ld = F rounded up to 32
 *   so that the input projection runs the large-tile GEMM (padding columns: whatever the buffers hold, zeros in the engine).
 *   pad_ld % 4 == 0 and pad_ld >= pad_cols rounded up to 4; the three pointers 16-byte aligned.  pad_cols % 4 != 0 (a feature count
 *   the data set dictates: 46, 137, ...) is read with scalar loads, and the columns from pad_cols up to the next multiple of 4 are
 *   then WRITTEN, with zeros (fp32 copy and image); the columns beyond stay untouched as above. */
/* A batch into the step's static input buffers in one launch: x (nx floats = rows of F) into rows of ld_dst >= F floats of x_dst
 * (padding columns untouched; nx may be 0), y_dst = y (ny floats),
 * mask_dst[i] = (y[i] == pad_value) -- the padding mask the reference derives per batch (allrank/training/train_utils.py:19,
 * allrank/data/dataset_loading.py:15 PADDED_Y_VALUE). */
int ltrx_ingest_batch(const float* x, const float* y, size_t nx, size_t ny, int F, int ld_dst, float pad_value, float* x_dst,
                      float* y_dst, unsigned char* mask_dst, ltrx_stream_t stream);
/* `tile` (both GEMMs) is a per-call tuning argument: 0 = automatic choice per shape (what every product call passes);
 * ltrx_gemm_nt: the 128-column kernel 1 128x128x32, 2 128x128x64, 3 256x128x32, 4 256x128x64 (precision codes 1 and 2 have the
 * 128x128x32 form only: every code runs it); the 256-column (large-tile) kernel 6 256x256x32, 7 128x256x32, 8 64x256x32 with two
 * workgroups per CU (these need N % 256 == 0, K % 32 == 0, 16-byte aligned C / bias / aux and a precision code other than 1:
 * LTRX_EUNSUPPORTED otherwise); any other code runs as 1.  ltrx_gemm_tn: 1 = the 128x128 kernel even where the 256x256 one applies;
 * 9 = the caller states that every row of B (the last one included) is READABLE up to column KP rounded up to 256 (ldb >= that): the
 * 256x256 kernel then also serves a KP that is no multiple of 256 -- it reads the padding, drops its products, C stays dense [NP, KP]
 * (the engine's input buffer keeps F = 136 features in rows of 256 floats).  Results do not depend on the tile beyond fp32 summation
 * order. */
/* test hook, no GPU needed: the launch plan of an ltrx_gemm_nt call with these shapes, leading dimensions, act, bias / dropout present
 * (0 / 1), precision code (`strict`) and `tile`, given the two alignment facts the call derives from its pointers -- vec_epi: C, bias
 * and aux allow 16-byte accesses; b_image: a 16-byte aligned B_image was passed.  Returns the number of launches (1, or 2 in the
 * row-split window of the automatic choice) and writes 7 ints per launch to out (14 ints): first row, rows, tile code (1-4, 6, 7, 8 as
 * above), bf16 terms per operand (1, 2, 3), and for the large-tile kernel: partial last row tile (0 / 1), B read from its image
 * (0 / 1), epilogue kind (0 generic, 1 plain, 2 bias, 3 ReLU + one-bit mask, 4 mask read, 5 residual).  Returns 0 where the call is
 * refused, and then out[0] = its return code. */
int ltrx_debug_gemm_nt_plan(int M, int N, int K, int lda, int ldb, int ldc, int act, int has_bias, int drop_on, int strict, int tile,
                            int vec_epi, int b_image, int* out);
/* test hook, no GPU needed: the launch plan of an ltrx_gemm_tn call.  Returns 1 when it runs the 256x256 kernel, 0 for the 128x128
 * one, -1 for arguments the call refuses; *splits_out = row splits, *rows_per_split_out = rows of each, *kv_out = columns of B that
 * exist (KP; the 256x256 kernel over padded rows, tile 9, computes KP rounded up to 256 of them). */
int ltrx_debug_gemm_tn_plan(int M, int NP, int KP, int lda, int ldb, int strict, int tile, int* splits_out, int* rows_per_split_out,
                            int* kv_out);
/* workspace for ltrx_gemm_tn sized for M rows: sufficient for EVERY call with the same NP, KP and any row count <= M
 * (variable-length batches re-use one workspace); ltrx_gemm_tn_splits = the split count a call with exactly M rows uses
 * (each split owns an [NP,KP] slab + 2 bias rows of the workspace). */
size_t ltrx_gemm_tn_workspace_bytes(int M, int NP, int KP);
int ltrx_gemm_tn_splits(int M, int NP, int KP);
int ltrx_gemm_tn(const float* A, int lda, const float* B, int ldb, float* C, float* bias_out, int M, int NP, int KP, int strict,
                 int tile, void* ws, ltrx_stream_t stream);
/* Up to LTRX_GEMM_TN_GROUP_MAX weight gradients over the SAME M rows in one launch (the four nn.Linear projections of an encoder
 * layer: allrank/models/transformer.py:174, 217-218 -- loss.backward() computes each dW = dY^T X separately, allrank/training/
 * train_utils.py:23): C[p][NP[p], KP[p]] = A[p][M, NP[p]]^T * B[p][M, KP[p]], bias_out[p] (may be NULL per problem) = column
 * sums of A[p].  The tiles of all problems share one grid, so the row split is chosen for the SUM of the tiles: 4x fewer partial
 * slabs than four ltrx_gemm_tn calls.  Each result is BIT-IDENTICAL run to run (fixed split and reduction order) but not to the
 * single-problem call's (different split count).  Shapes outside the 256x256-tile kernel fall back to one ltrx_gemm_tn per problem.
 * The pointer / int tables are HOST arrays, read before the call returns.  ws: ltrx_gemm_tn_group_workspace_bytes (sufficient for
 * every row count <= M). */
#define LTRX_GEMM_TN_GROUP_MAX 4
size_t ltrx_gemm_tn_group_workspace_bytes(int nprob, int M, const int* NP, const int* KP);
/* slabs_out / bias_slabs_out / splits_out: all NULL = the call reduces its partial slabs itself (one launch per problem); all given =
 * the reduction is left to the caller: problem p's dW is the fixed-order sum of *splits_out slabs of NP[p]*KP[p] floats at slabs_out[p],
 * its bias gradient the column sums of *splits_out rows of NP[p] floats at bias_slabs_out[p] (NULL where bias_out[p] is NULL) -- entries
 * for ltrx_reduce_group, which sums them together with other partials of the same layer in one launch.  *splits_out == 0: the call took
 * the per-problem path and C / bias_out are already final. */
int ltrx_gemm_tn_group(int nprob, const float* const* A, const int* lda, const float* const* B, const int* ldb, float* const* C,
                       float* const* bias_out, int M, const int* NP, const int* KP, int strict, void* ws, size_t ws_bytes,
                       const float** slabs_out, const float** bias_slabs_out, int* splits_out, ltrx_stream_t stream);
/* n <= LTRX_REDUCE_GROUP_MAX independent reductions in one launch: dst[i][c] = sum_{s < splits[i]} src[i][s * row_stride[i] + c] for
 * c < cols[i], each in a fixed order (deterministic).  Entries with splits[i] <= 0 are skipped.  (The engine sums the weight-gradient
 * slabs of an encoder layer and the parameter-gradient partials of its LayerNorms with it: 11 launches -> 1; autograd's per-tensor
 * accumulation in loss.backward(), allrank/training/train_utils.py:23.) */
/* test hook, no GPU needed: the workgroup -> (tile, split) table ltrx_gemm_tn_group launches with for these shapes (the tiles of one
 * (problem, split) group on one XCD where they fit); tile_out / split_out: 256 bytes each; returns the workgroup count, 0 when the shapes
 * take the per-problem path. */
int ltrx_debug_tn_group_map(int nprob, int M, const int* NP, const int* KP, unsigned char* tile_out, unsigned char* split_out);
/* test hook, no GPU needed: the decision of an ltrx_gemm_tn_group / ltrx_gemm_tn_group_ln call with these shapes, leading dimensions
 * (lda / ldb may be NULL: dense), precision code and ws_bytes -- the library's own predicate, not a copy of it.  Returns 1 when the
 * call runs the grouped kernel, 0 when it falls back to one ltrx_gemm_tn per problem (a shape outside the 256x256 kernel, more than
 * 256 tiles, or ws_bytes below the need).  *splits_out = row splits of the grouped launch (0 on the per-problem path);
 * *need_bytes_out = workspace bytes the grouped launch writes at that split count, exactly (0 where the shapes alone rule it out). */
int ltrx_debug_tn_group_plan(int nprob, int M, const int* NP, const int* KP, const int* lda, const int* ldb, int strict, size_t ws_bytes,
                             int* splits_out, size_t* need_bytes_out);
/* ltrx_gemm_tn_group followed by ltrx_layernorm_bwd_partial(dy .. partial_rows_out) in ONE call, every output with the bits that pair
 * gives it.  The grouped launch keeps one workgroup per CU and plans tiles x splits <= 256 of them; when CUs are left over (the four
 * projections of an encoder layer: 48 tiles x 5 splits = 240) and D is a register-resident row width (D % 256 == 0, D <= 1024, aligned
 * pointers), the LayerNorm backward runs as 256 - tiles x splits extra workgroups of the SAME launch instead of a launch of its own
 * behind it.  side_wgs: 0 = the library decides (taken only when its measured streaming rate puts the side job well inside the GEMM
 * part's duration); > 0 = that many side workgroups, clamped to the free CUs (tests).  *side_taken_out = the side workgroups used, 0
 * when the call ran the grouped GEMM (or its per-problem fall-back) and then the LayerNorm kernel: the caller handles one case.
 * LTRX_EINVAL, and nothing launched, when dx_out or ln_ws overlaps an A[p] or B[p]: side workgroups write while the others read. */
int ltrx_gemm_tn_group_ln(int nprob, const float* const* A, const int* lda, const float* const* B, const int* ldb, float* const* C,
                          float* const* bias_out, int M, const int* NP, const int* KP, int strict, void* ws, size_t ws_bytes,
                          const float** slabs_out, const float** bias_slabs_out, int* splits_out, const float* dy, const float* xsum,
                          const float* a, const float* mean, const float* rstd, const float* dres_in, int rows, int D, float eps,
                          float* dx_out, void* ln_ws, int* partial_rows_out, int side_wgs, int* side_taken_out, ltrx_stream_t stream);
/* test hook, no GPU needed: the side-job plan of ltrx_gemm_tn_group_ln (aligned pointers, sufficient workspace, strict 0).  Returns the
 * side workgroup count (0: not taken); *gemm_wgs_out: workgroups of the GEMM path (0: per-problem path); *vblocks_out: workgroups of
 * the stand-alone LayerNorm backward launch, whose work the side workgroups divide; owner_out[vb], 320 ints: the id of the workgroup
 * that takes block vb of that launch, -1 where none does. */
int ltrx_debug_tn_group_side_plan(int nprob, int M, const int* NP, const int* KP, int rows, int D, int has_dres, int side_wgs,
                                  int* gemm_wgs_out, int* vblocks_out, int* owner_out);
#define LTRX_REDUCE_GROUP_MAX 16
int ltrx_reduce_group(int n, const float* const* src, const int* splits, const size_t* row_stride, const size_t* cols, float* const* dst,
                      ltrx_stream_t stream);

/* Model options around the encoder on the explicit step (allrank_amd/csrc/ltrx_extras.hip):
 *   ltrx_layernorm_torch_fwd: FCModel.input_norm = nn.LayerNorm(n_features) (model.py:27,39): biased variance, eps inside the
 *       sqrt; saves mean and rstd.  Its parameter gradients come from ltrx_layernorm_bwd called with these statistics (D >= 2
 *       there: ltrx_layernorm_bwd refuses D == 1, which this forward accepts).
 *   ltrx_layernorm_torch_fwd_strided: the same rows (same bits) read with row stride ldx >= D and written with row stride ldy >= D;
 *       columns D .. ldy of y are not touched.  The engine normalises dense input rows into the padded operand rows of the first
 *       projection when the feature count is no multiple of 4.  A stride below D: LTRX_EINVAL, nothing launched.
 *   ltrx_posenc_fwd: positional encoding (positional.py:15-77, transformer.py:51-52): y = scale * x + table[row(m)],
 *       row = padding_idx for masked items and ranks outside [0, padding_idx), else indices[m]; mask may be NULL.
 *   ltrx_posenc_table_bwd: gradient of a LEARNED table: dtable[r] = sum of dx[m] over the rows m with row(m) == r; the padding
 *       row gets 0 (nn.Embedding(padding_idx)); deterministic.      ltrx_scale_inplace: x *= s (the sqrt(d_model) factor).
 *   ltrx_out_act_fwd / _bwd: OutputLayer activation (model.py:106-117), kind 1 = Sigmoid, 2 = Tanh; bwd: dz = dy * act'(y). */
int ltrx_layernorm_torch_fwd(const float* x, const float* w, const float* b, int rows, int D, float eps, float* y, float* mean_out,
                             float* rstd_out, ltrx_stream_t stream);
int ltrx_layernorm_torch_fwd_strided(const float* x, int ldx, const float* w, const float* b, int rows, int D, float eps, float* y, int ldy,
                                     float* mean_out, float* rstd_out, ltrx_stream_t stream);
int ltrx_posenc_fwd(const float* x, const float* table, const int64_t* indices, const uint8_t* mask, int M, int D, int padding_idx,
                    float scale, float* y, ltrx_stream_t stream);
int ltrx_posenc_table_bwd(const float* dx, const int64_t* indices, const uint8_t* mask, int M, int D, int padding_idx, float* dtable,
                          ltrx_stream_t stream);
int ltrx_scale_inplace(float* x, size_t n, float s, ltrx_stream_t stream);
int ltrx_out_act_fwd(const float* z, size_t n, int kind, float* y, ltrx_stream_t stream);
int ltrx_out_act_bwd(const float* dy, const float* y, size_t n, int kind, float* dz, ltrx_stream_t stream);

/* Slate-resident training step of an FCModel([H]) -> OutputLayer(H, 1) -> listNet model (BASELINE configs[1]): forward, loss,
 * backward and -- optionally -- the Adam update in TWO launches that read the features from HBM once
 * (allrank_amd/csrc/ltrx_fcstep.hip).  Replaces, for this model family, the call sequence of loss_batch
 * (allrank/training/train_utils.py:18-29): FCModel.forward (allrank/models/model.py:35-44, one Linear + activation `act`:
 * 0 = None, 1 = ReLU, no dropout, no input_norm), OutputLayer.forward (model.py:111-117, d_output 1, no activation),
 * listNet (allrank/models/losses/listNet.py:8-30), autograd's backward of the three, and torch.optim.Adam / AdamW.step.
 *   x[B,L,F], y[B,L] (pad_value marks padded slots); `params` = ONE flat fp32 buffer holding W1[H,F] at off_w1 (= 0), b1[H] at
 *   off_b1, w_out[H] at off_wout, b_out[1] at off_bout: adjacent segments, each padded to a multiple of 4 floats, nflat in total;
 *   `grads` has the same layout and receives d loss / d params; scores[B,L] = model.score(x); dscores (optional) = d loss / d scores;
 *   hidden_out (optional, tests) = the FC activations [B,L,H]; loss_out[1] = sum of the per-slate losses / batch_divisor.
 *   exp_avg != NULL: the Adam update is applied to `params` in the reducing launch (step_count: device float, bumped by the
 *   call; decoupled != 0: AdamW) -- same update rule as ltrx_adam_step; NULL: gradients only (sharded runs all-reduce them first).
 * Arithmetic: the two contractions (x W1^T and x^T dh) are three bf16 MFMA products per fp32 product with fp32 accumulation, as
 * in ltrx_gemm_nt / ltrx_gemm_tn; everything else fp32.  Partial gradients are summed in a fixed order (deterministic).
 * ltrx_fc_listnet_supported: 1 when (L, F, H) fit the kernel (L <= 256, F <= 144 and F % 4 == 0, H <= 96), else 0 and the step
 * call returns LTRX_EUNSUPPORTED (the caller then runs the GEMM launch sequence). */
int ltrx_fc_listnet_supported(int L, int F, int H);
size_t ltrx_fc_listnet_workspace_bytes(int B, int L, int F, int H, size_t nflat);
int ltrx_fc_listnet_step(const float* x, const float* y, int B, int L, int F, int H, int act, float* params, size_t off_w1,
                         size_t off_b1, size_t off_wout, size_t off_bout, size_t nflat, float eps, float pad_value,
                         float batch_divisor, float* scores, float* dscores, float* hidden_out, float* loss_out, float* grads,
                         float* exp_avg, float* exp_avg_sq, float* step_count, float lr, float beta1, float beta2, float adam_eps,
                         float weight_decay, int decoupled, void* ws, ltrx_stream_t stream);

/* The same step for a LINEAR scorer (FC activation None), opt-in: score = w_out . (W1 x + b1) + b_out = x . v + c with v = W1^T w_out --
 * two consecutive linear maps evaluated as one, exactly -- and dW1 = w_out (x) u, db1 = D w_out, dw_out = W1 u + D b1, db_out = D with
 * u = sum dscore_l x_l, D = sum dscore_l.  Per slate two matrix-vector products in fp32 FMAs (no matrix cores, no operand split); the
 * slate is held in registers, the next one is in flight while it is processed; a workgroup's partial gradient is F + 2 floats.  Same
 * arguments, layout of `params` / `grads`, outputs and optimizer semantics as ltrx_fc_listnet_step (without `act` / hidden_out).
 * Two launches (slates; partials -> gradients + optimizer).  allrank_amd/csrc/ltrx_fcstep.hip. */
size_t ltrx_fc_linear_listnet_workspace_bytes(int B, int F);
int ltrx_fc_linear_listnet_step(const float* x, const float* y, int B, int L, int F, int H, float* params, size_t off_w1, size_t off_b1,
                                size_t off_wout, size_t off_bout, size_t nflat, float eps, float pad_value, float batch_divisor,
                                float* scores, float* dscores, float* loss_out, float* grads, float* exp_avg, float* exp_avg_sq,
                                float* step_count, float lr, float beta1, float beta2, float adam_eps, float weight_decay,
                                int decoupled, void* ws, ltrx_stream_t stream);

/* On-device batch assembly for a CSR training set resident in HBM (allrank_amd/csrc/ltrx_data.hip):
 *   ltrx_fixlength_positions: FixLength (dataset_loading.py:32-93) for the B slates `slates` of a batch: positions[b][l] = the
 *       position inside slate b that fills slot l, -1 = padding.  Short slates are padded (:81-93); slates of >= L items are
 *       sampled without replacement in random order (:70) with the reference's relevance rule (:72-76).  Counter-based
 *       randomness keyed by (`seed`, the slate's id in the dataset): the same seed draws the same sample for a slate whichever
 *       batch or batch row it arrives in (a rank assembling only its block of a global batch == the one-rank run);
 *       max_slate_len <= 12288.
 *   ltrx_assemble_batch: xb[B,L,F], yb[B,L] (-1 on padding), indices[B,L] (= positions) from the CSR arrays (ToTensor +
 *       collate, :19-29).
 *   ltrx_assemble_batch_picked: the same outputs in ONE launch from positions chosen on the host (the reference's own
 *       np.random.choice draws; no [B,L] positions tensor in HBM).  Row b with pick_row[b] >= 0 takes position
 *       picks[pick_row[b]][l] for slot l; a row with pick_row[b] < 0 keeps its stored order, l < len ? l : -1 (the first L items of
 *       a slate of >= L items).  A position outside [0, len), or a pick_row >= n_pick_rows, is padding (features 0, label -1,
 *       index -1): nothing outside the slate is read.  picks may be NULL only with n_pick_rows == 0.  Slates of any length. */
int ltrx_fixlength_positions(const int64_t* offsets, const float* y_items, const int64_t* slates, int B, int L, int max_slate_len,
                             uint64_t seed, int64_t* positions, ltrx_stream_t stream);
int ltrx_assemble_batch(const float* x_items, const float* y_items, const int64_t* offsets, const int64_t* slates,
                        const int64_t* positions, int B, int L, int F, float* xb, float* yb, int64_t* indices, ltrx_stream_t stream);
int ltrx_assemble_batch_picked(const float* x_items, const float* y_items, const int64_t* offsets, const int64_t* slates,
                               const int32_t* pick_row, const int32_t* picks, int n_pick_rows, int B, int L, int F, float* xb, float* yb,
                               int64_t* indices, ltrx_stream_t stream);

/* libsvm / SVMlight text parsed on the device (the reference: sklearn's load_svmlight_file on the host, dataset_loading.py:130).
 * text = the file's bytes in device memory, line_start[n_lines] = byte offset of every line.  One thread per line.
 * Pass 1 (X NULL): y[line], qid[line], minmax_index = {smallest, largest} feature index (initialise to {INT_MAX, -1}).
 * Pass 2: X[line][index - index_base] = value (X zero-initialised by the caller, dense [n_lines, n_features]).
 * bad_lines (device int, zero-initialised) counts malformed lines. */
int ltrx_libsvm_parse(const uint8_t* text, const int64_t* line_start, int64_t n_lines, int64_t n_bytes, float* y, int64_t* qid, float* X,
                      int n_features, int index_base, int* minmax_index, int* bad_lines, ltrx_stream_t stream);

/* Feature normalisation of a resident item array (the reference: reproducibility/normalize_features.py, a host script over three
 * libsvm files).  allrank_amd/csrc/ltrx_featnorm.hip.
 *   x[n, F]: fp32 rows, `ld` floats apart (ld >= F; the ld - F floats behind a row are never read and never written).
 *   negate[F], take_log[F]: device uint8 flags per column.  With s = -1 where negate[f] is set, else 1:
 *       t(x) = s x,  and  t(x) = log(s x + eps_log)  where take_log[f] is set -- evaluated in fp64 from the fp32 value.
 *   eps_log_host, eps_host: HOST pointers to the two fp64 constants (read before the launch).
 *   ltrx_feature_min:       min_out[f] = min over the rows of s x (fp32, exact).  -0.0 and +0.0 compare equal, so a column of zeros
 *                           of either sign has a minimum that is >= 0.  Called once per role; the caller takes the minimum over roles.
 *   ltrx_feature_moments:   mean_out[f] = (sum of t) / n, then std_out[f] = sqrt((sum of (t - mean_out[f])^2) / n): TWO passes over
 *                           x, as np.mean / np.std take them, never E[t^2] - E[t]^2.
 *   ltrx_feature_normalize: x = (float)((t(x) - mean[f]) / (std[f] + eps)), in place.
 * A workgroup owns a block of rows and a thread a fixed set of columns: its partial results stay in registers, the threads of a
 * workgroup that share columns are combined by a tree of fixed shape in LDS, every workgroup leaves one row of F fp64 partials in
 * `ws`, and a second small launch combines those rows in a fixed order.  No floating-point atomics: the same bits on every call with
 * the same arguments.  Rows are read (and written) in 16-byte pieces where ld % 4 == 0 and x is 16-byte aligned, in 4-byte pieces
 * otherwise; any F.  HBM: 4 n F bytes read per pass (one pass for the minimum, two for the moments), as many written by normalize.
 * The calls allocate nothing and synchronise nothing.  *_workspace_bytes: one row of F doubles per workgroup, never fewer for a
 * larger n; 0 for n <= 0 or F <= 0.
 * NULL x / negate / take_log / an output / ws / a host pointer, n <= 0, F <= 0 or ld < F: LTRX_EINVAL, nothing launched. */
size_t ltrx_feature_min_workspace_bytes(int n, int F);
int ltrx_feature_min(const float* x, int n, int F, int ld, const uint8_t* negate, float* min_out, void* ws, ltrx_stream_t stream);
size_t ltrx_feature_moments_workspace_bytes(int n, int F);
int ltrx_feature_moments(const float* x, int n, int F, int ld, const uint8_t* negate, const uint8_t* take_log,
                         const double* eps_log_host, double* mean_out, double* std_out, void* ws, ltrx_stream_t stream);
int ltrx_feature_normalize(float* x, int n, int F, int ld, const uint8_t* negate, const uint8_t* take_log, const double* eps_log_host,
                           const double* mean, const double* std, const double* eps_host, ltrx_stream_t stream);

/* libsvm text written on the device: the inverse of ltrx_libsvm_parse (the reference: dataset_saving.py:32, scikit-learn's
 * dump_svmlight_file on the host, 22 bytes of text per value).  allrank_amd/csrc/ltrx_svmwrite.hip, ltrx_fmt.h.
 *   X[n_rows, F]: fp32 rows, `ldx` floats apart (ldx >= F);  y[n_rows] fp32 labels;  qid[n_rows] int64;  all in device memory.
 *   A row is KEPT unless y[r] == pad_value (a NaN pad_value keeps every row).  The line of a kept row:
 *       <%.16g of y[r]> qid:<%d of qid[r]>   then   " <f + index_base>:<%.16g of X[r][f]>"   for each f with X[r][f] != 0, rising f,
 *       then "\n";  a row without a non-zero value ends "qid:N \n", with the space.  -0.0 counts as zero and is left out.
 *   "%.16g" is the text Python's '%.16g' % float(numpy.float32(v)) gives, for EVERY fp32 bit pattern: the correctly rounded sixteen
 *   significant digits of the exact binary value (half-even on exact ties), trailing zeros stripped, fixed notation for decimal
 *   exponents -4 .. 15 and d.ddde+XX otherwise, "-0", "nan", "inf", "-inf".  Integer arithmetic only (multi-word division and
 *   multiplication by 10^9); the host and the device run the same function.
 *   ltrx_libsvm_line_bytes (pass A): line_bytes[r] = the byte length of row r's line, 0 for a row that is not kept;  *bad (device int,
 *       zero-initialised by the caller) += the number of kept rows that hold a non-finite label or value.
 *   ltrx_libsvm_format (pass B): row r's line at text + line_start[r], where line_start = the exclusive prefix sum of line_bytes (the
 *       caller's, e.g. torch.cumsum) and n_bytes = its total.  Offsets are int64.  Nothing outside [0, n_bytes) is written, whatever
 *       line_start holds.  Placement is deterministic: one wave per row, a wave scan of the token lengths, no atomics.
 *   Both passes format every value (a token's length is known only once it is rounded); neither allocates or synchronises.
 *   NULL X / y / qid / an output, n_rows <= 0, F <= 0, ldx < F, index_base < 0, F + index_base > INT_MAX, n_bytes <= 0: LTRX_EINVAL,
 *   nothing launched.  Not covered by the test suite: a text above 2 GiB in one call.
 *   ltrx_debug_format_g16: HOST-ONLY test hook, no launch -- v[n], text[24 n] and len[n] are host pointers; len[i] bytes (at most 22)
 *       of the text of v[i] start at text + 24 i.  It runs the function the kernels run, compiled for the host. */
int ltrx_libsvm_line_bytes(const float* X, int64_t ldx, const float* y, const int64_t* qid, int64_t n_rows, int F, float pad_value,
                           int index_base, int64_t* line_bytes, int* bad, ltrx_stream_t stream);
int ltrx_libsvm_format(const float* X, int64_t ldx, const float* y, const int64_t* qid, int64_t n_rows, int F, float pad_value,
                       int index_base, const int64_t* line_start, int64_t n_bytes, uint8_t* text, ltrx_stream_t stream);
int ltrx_debug_format_g16(const float* v, int64_t n, uint8_t* text, int32_t* len);

/* Test hook: D[32x32] = A[32x2] * B[2x32] with ONE v_mfma_f32_32x32x2_f32, written through the operand / result
 * lane layout the attention kernels assume.  Lets the parity suite tell a layout bug from a logic bug. */
int ltrx_selftest_mfma32x32x2(const float* A, const float* B, float* D, ltrx_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LTRX_H */
