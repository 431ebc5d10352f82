/* ocffm_fold.h — folding new users in from an interaction history: the fold
 * entries of an ocffm_model.  Included by ocffm.h (after the saved-models
 * section, whose types it uses); do not include it alone. */
#ifndef OCFFM_FOLD_H
#define OCFFM_FOLD_H

#ifdef __cplusplus
extern "C" {
#endif

/* Folding in a row from an interaction history (no reference counterpart):
 * serving a user the model was not trained on, given the items that user has
 * touched.  Row i of `hist` (a labelled data set with hist.m == X.m, which may
 * be X itself; only its labels are read) holds the history of row i of X: H_i,
 * its sorted distinct labels < n (a repeated label counts once, labels >= n
 * are ignored).  A row with H_i non-empty is folded: with d = fv k, q_j in R^d
 * the first k entries of Q_{field fv + g}[j] over g < fv, and z_ij = a_i + b_j
 * + sum_c <P_c[i], Q_c[j]> from the projected tables (also for a row without a
 * kept node: then z_ij = b_j, never the popularity), its correction delta_i
 * minimises the training objective's per-row terms
 *   sum_{j in H_i} (1 - z_ij - <delta,q_j>)^2
 *   + omega sum_{j < n, j not in H_i} (r - z_ij - <delta,q_j>)^2 + lambda |delta|^2,
 * the rows of a new value-1 feature of user field `field` towards the item
 * fields (the classic ALS fold-in; a_i stays as projected).  It is solved in
 * closed form on the device in fp64 (an FP32 model's values are widened), from
 * catalogue aggregates that are built on the first fold call after a catalogue
 * is set and kept with the model.  Applying it adds delta_i[g k + t] to
 * P_{field fv + g}[i][t] (sum in fp64, rounded to the model's precision),
 * after which the plain serving call runs: a folded row's scores have the same
 * bits in every fold entry, and a folded row is never cold.  A row with H_i
 * empty is not folded: delta_i = 0 and every result is the plain entry's, bit
 * for bit, the cold-row rule included.  delta_i has the same bits between
 * calls and does not depend on the row's place, on the other rows or on
 * OCFFM_REC_ROWS: every sum has a fixed order and there are no floating-point
 * atomics.
 *
 * ocffm_model_fold_in writes delta (X.m x d, row-major, g-major then t < k)
 * and, when nhist is given, |H_i|.  The _fold entries are the plain entries of
 * the same name on the folded rows: recommend_fold keeps the meaning of
 * OCFFM_REC_EXCLUDE_LABELS (X's own labels); for a hold-out protocol pass the
 * held-out labels in X and the history as both hist and seen; evaluate_fold is
 * label_ranks_fold followed by ocffm_eval_from_ranks.
 * Errors, on top of the plain entry's: OCFFM_E_ARG for a NULL fo, hist or
 * delta, field >= fu, lambda <= 0, omega < 0 or a non-finite parameter, hist
 * without labels or with another row count than X, fv k > OCFFM_FOLD_MAX_D;
 * OCFFM_E_STATE before ocffm_model_set_items; OCFFM_E_DATA if a pivot of the
 * normal equations is not positive and finite (impossible for valid
 * parameters and finite tables).  An empty catalogue gives delta = 0, nhist =
 * 0 and the plain entry's results.
 * Counters: "fold_stats_builds", aggregate builds since the model was created;
 * "fold_stats_us", the last build; "fold_us", the last call's build-solve and
 * apply launches between HIP events; "fold_rows", the rows the last call
 * folded. */
#define OCFFM_FOLD_MAX_D 128
typedef struct ocffm_fold {
  uint32_t field;          /* the user field of the new feature, < fu */
  double omega, lambda, r; /* as trained: weight and target of the unobserved pairs, regulariser */
} ocffm_fold;

int ocffm_model_fold_in(ocffm_model *m, const ocffm_data *X, const ocffm_data *hist, const ocffm_fold *fo,
                        double *delta /* X.m x d, row-major, g-major then t < k */, uint32_t *nhist /* may be NULL: |H_i| */);
int ocffm_model_recommend_fold(ocffm_model *m, const ocffm_data *X, const ocffm_data *hist, const ocffm_fold *fo,
                               uint64_t row0, uint64_t rows, uint32_t topn, uint32_t flags, uint32_t *items, double *scores);
int ocffm_model_label_ranks_fold(ocffm_model *m, const ocffm_data *X, const ocffm_data *hist, const ocffm_fold *fo,
                                 const ocffm_data *seen, uint32_t *ranks, double *scores, uint32_t *ncand);
int ocffm_model_evaluate_fold(ocffm_model *m, const ocffm_data *X, const ocffm_data *hist, const ocffm_fold *fo,
                              const ocffm_data *seen, const uint32_t *cuts, uint32_t ncut, ocffm_eval *out);

#ifdef __cplusplus
}
#endif

#endif /* OCFFM_FOLD_H */
