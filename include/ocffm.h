/*
 * ocffm.h — C ABI of the MI355X-native one-class FFM trainer.
 *
 * This is the drop-in boundary for the reference's hot path (one training
 * epoch of block Newton-CG, johncreed/one-class-ffm ffm.cpp:852-870).  The
 * reference exposes it only as C++ classes (ffm.h:42-154: Parameter, ImpData,
 * ImpProblem, save_model) driven by train.cpp:169-207.  Each entry point
 * below names the reference interface it replaces.  Plain pointers and
 * sizes only: no C++ types, no exceptions, no torch types cross this ABI.
 *
 * All functions return an int status (OCFFM_OK == 0).  On failure,
 * ocffm_last_error() returns a thread-local message.  A problem object is
 * not re-entrant; one host thread drives it.  Device memory is owned by the
 * problem object; host arrays passed in are copied (the caller keeps them).
 */
#ifndef OCFFM_H
#define OCFFM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OCFFM_OK 0
#define OCFFM_E_ARG 1   /* invalid argument   (reference: std::invalid_argument, train.cpp:201-205) */
#define OCFFM_E_IO 2    /* file not readable / not writable                                         */
#define OCFFM_E_DATA 3  /* malformed input (reference: UB, e.g. label >= #items, ffm.cpp:267,382)   */
#define OCFFM_E_HIP 4   /* HIP runtime error, or no GPU                                             */
#define OCFFM_E_COMM 5  /* RCCL error                                                               */
#define OCFFM_E_STATE 6 /* call out of order (e.g. epoch before init)                               */

/* Precision of the device path. */
#define OCFFM_FP64 64 /* parity mode: same arithmetic type as the reference (ffm.h:34-35) */
#define OCFFM_FP32 32 /* perf mode: fp32 tables, fp64 CG scalars and reductions           */

/* Replaces class Parameter (ffm.h:42-49).  Defaults (ocffm_param_default)
 * are the reference's *code* defaults: omega 0.1, lambda 1e-5, r -1,
 * nr_pass 20, k 4, nr_threads 1, self_side 1, freq 0. */
typedef struct ocffm_param {
  double omega;        /* -w : weight of the implicit negatives          */
  double lambda;       /* -l : L2 regularisation                          */
  double r;            /* -r : target value of the negatives              */
  uint32_t nr_pass;    /* -t : epochs                                     */
  uint32_t k;          /* -k : latent dimension (any k in 1..128)         */
  uint32_t nr_threads; /* -c : host threads (parsing); device path ignores */
  int32_t self_side;   /* !--ns : include same-side field-pair blocks     */
  int32_t freq;        /* --freq : lambda scaled by feature frequency     */
  int32_t precision;   /* OCFFM_FP64 or OCFFM_FP32                        */
  int32_t device;      /* HIP device ordinal                              */
} ocffm_param;

void ocffm_param_default(ocffm_param *p);

const char *ocffm_last_error(void);
int ocffm_device_count(int *count);

/* ------------------------------------------------------------------ data
 * Replaces class ImpData (ffm.h:51-79).  A data set is rows of
 * (fid, idx, val) feature nodes plus, for train/test files, a label list of
 * positive item ids per row. */
typedef struct ocffm_data ocffm_data;

typedef struct ocffm_data_info {
  uint64_t m;     /* rows (lines)                                  */
  uint64_t n;     /* max label + 1 (0 for item files)              */
  uint64_t f;     /* fields: max fid + 1 over every token          */
  uint64_t nnz_x; /* kept feature nodes                            */
  uint64_t nnz_y; /* labels                                        */
} ocffm_data_info;

/* ImpData::read + ImpData::split_fields (ffm.cpp:80-257).  With ds != NULL
 * (the train set's per-field Ds, as for test files, train.cpp:191) a node
 * with idx >= ds[fid] is dropped. */
int ocffm_data_read(const char *path, int has_label, const uint64_t *ds, uint32_t nds, ocffm_data **out);

/* The same from in-memory rows: xptr[m+1] row pointers into fid/idx/val,
 * yptr[m+1]/ycol labels (both NULL for an item file). */
int ocffm_data_from_rows(uint64_t m, const uint64_t *xptr, const uint32_t *fid, const uint64_t *idx,
                         const double *val, const uint64_t *yptr, const uint64_t *ycol, const uint64_t *ds,
                         uint32_t nds, ocffm_data **out);

/* ImpData::transY (ffm.cpp:259-294): item-major positives of V from the
 * user-major labels of U. */
int ocffm_data_trans_y(ocffm_data *V, const ocffm_data *U);

int ocffm_data_get_info(const ocffm_data *d, ocffm_data_info *out);
/* Per-field Ds (ffm.cpp:221); out must hold info.f values. */
int ocffm_data_get_ds(const ocffm_data *d, uint64_t *out);
/* The parsed labels (ffm.cpp:93-101: U->Y before transY): yptr holds info.m+1
 * offsets, ycol info.nnz_y item indices.  Either pointer may be NULL. */
int ocffm_data_get_labels(const ocffm_data *d, uint64_t *yptr, uint64_t *ycol);
/* One field's CSR after split_fields (ffm.cpp:185-257): xptr info.m+1
 * offsets, then that field's node indices and values.  Pointers may be NULL;
 * *nnz receives the field's node count. */
int ocffm_data_get_field(const ocffm_data *d, uint32_t field, int64_t *xptr, uint32_t *xidx, double *xval,
                         uint64_t *nnz);
void ocffm_data_free(ocffm_data *d);

/* --------------------------------------------------------------- problem
 * Replaces class ImpProblem (ffm.h:82-151). */
typedef struct ocffm_problem ocffm_problem;

/* ImpProblem(U, Uva, V, param) (ffm.h:84-86).  Ut may be NULL (no -p).  The
 * data sets are copied to the device; V must have been through
 * ocffm_data_trans_y.  Single process, one GPU. */
int ocffm_problem_create(const ocffm_data *U, const ocffm_data *Ut, const ocffm_data *V, const ocffm_param *p,
                         ocffm_problem **out);

/* Data-parallel variant (no reference counterpart: the reference is one
 * process).  One process per GPU; training rows (users) are split into
 * nranks contiguous shards and this rank keeps shard `rank`.  Gradient and
 * Hessian-vector partial sums are all-reduced with RCCL.
 * comm_id: OCFFM_COMM_ID_BYTES bytes from ocffm_comm_id() on rank 0,
 * broadcast by the caller (with nranks == 1 the RCCL path still runs: a
 * one-rank communicator, used by the tests).  Test rows (Ut) are sharded
 * the same way. */
#define OCFFM_COMM_ID_BYTES 128
int ocffm_comm_id(void *out);
int ocffm_problem_create_dist(const ocffm_data *U, const ocffm_data *Ut, const ocffm_data *V,
                              const ocffm_param *p, int rank, int nranks, const void *comm_id,
                              ocffm_problem **out);

/* Host-side all-reduce hook (tests and environments without RCCL).  When
 * set, every sum-all-reduce is staged through host memory and handed to
 * fn(buf, count, is_double, user).  Must be set before ocffm_problem_init. */
typedef int (*ocffm_allreduce_fn)(void *buf, uint64_t count, int is_double, void *user);
int ocffm_problem_create_dist_host(const ocffm_data *U, const ocffm_data *Ut, const ocffm_data *V,
                                   const ocffm_param *p, int rank, int nranks, ocffm_allreduce_fn fn,
                                   void *user, ocffm_problem **out);

/* ImpProblem::init (ffm.cpp:467-512).  W/H are drawn on the host from the
 * C library rand() stream exactly as the reference does (ffm.cpp:71-78).
 * The reference's init is the first rand() consumer of its process (implicit
 * seed 1); HIP runtime start-up in ocffm_problem_create may draw from the
 * stream, so call srand(1) right before this for reference-identical W/H. */
int ocffm_problem_init(ocffm_problem *p);

/* ImpProblem::one_epoch (ffm.cpp:852-870). */
int ocffm_problem_one_epoch(ocffm_problem *p);

/* ImpProblem::solve_side / solve_cross for one block (ffm.cpp:815-850). */
int ocffm_problem_solve_block(ocffm_problem *p, uint32_t f1, uint32_t f2);

/* ImpProblem::cache_sasb (ffm.cpp:514-535). */
int ocffm_problem_cache_sasb(ocffm_problem *p);

/* ImpProblem::solve (ffm.cpp:1147-1161): nr_pass epochs, validation and the
 * stdout table every 10th epoch when a test set is present. */
int ocffm_problem_solve(ocffm_problem *p);

/* The training objective (the reference's func(), ffm.cpp:1321-1351, which
 * its train never calls), in closed form from the state resident on the
 * device; no m x n pass.  With yhat_ij = a_i + b_j + sum_c <P_c[i], Q_c[j]>:
 *   value  = 0.5 (pos + omega (all - on_pos) + reg)
 *   pos    = sum over the label entries (i,j) of the training rows of
 *            (1 - yhat_ij)^2 (an entry listed twice counts twice)
 *   on_pos = the same sum of (r - yhat_ij)^2
 *   all    = sum_{i<m} sum_{j<n} (r - yhat_ij)^2
 *   reg    = sum over W and H of the used blocks of lambda_d |row_d|^2
 * lambda_d = lambda, or under freq lambda times the frequency of feature d
 * in the row's own field (W of block (f1,f2): field f1; H: field f2).
 * func() ignores freq while the gradient and CG use it (ffm.cpp:561-570):
 * under freq the value is the function the solver descends, not func()'s.
 *  - Arithmetic: every sum across row ranges, blocks and tiles is fp64 in a
 *    fixed order (no floating-point atomics): two calls on the same state
 *    return equal bits.  An OCFFM_FP32 problem accumulates at most 1024 rows
 *    of a Gram tile in fp32 before widening.  OCFFM_OBJ_BLOCKS /
 *    OCFFM_OBJ_GROUP (read at create) change the value by fp64 reassociation
 *    only.
 *  - Does not change the solver state (tables, projections, y~, biases, the
 *    CG log).
 *  - Sharded problems: collective; every rank returns the global value (m,
 *    labels: global counts).
 *  - Errors: OCFFM_E_ARG for a NULL problem or out; OCFFM_E_STATE before
 *    init / load_binary.
 * The launches are the kernel family "objective" of the statistics below;
 * the counter "obj_us" holds the last call's wall time. */
typedef struct ocffm_objective {
  double value, pos, on_pos, all, reg;
  uint64_t m, n, labels; /* global rows, item rows, label entries */
} ocffm_objective;
int ocffm_problem_objective(ocffm_problem *p, ocffm_objective *out);

/* ocffm_problem_solve with the objective reported and, optionally, a stop on
 * its relative decrease.  With o == NULL or objective_every == 0 and
 * tol <= 0 it is ocffm_problem_solve, byte for byte on stdout.  Otherwise
 * rank 0 prints one line per evaluation,
 *   objective iter=<init|epoch> value=<%.17g> decrease=<%.6g>
 * (decrease: (F_prev - F) / |F_prev|, absent on the init line), after that
 * epoch's validation row if there is one.  On an early stop with a test set
 * the last epoch is validated and its row printed unless it already was.
 * rep (may be NULL): epochs run, whether the tolerance stopped the solve, the
 * objective at init and at the last evaluation (0 when never evaluated). */
typedef struct ocffm_solve_opts {
  uint32_t objective_every; /* 0: never; e: before the first epoch and after every e-th */
  double tol;               /* <= 0: none; else stop after epoch t when (F_prev - F_t) <= tol |F_prev|,
                               F_prev the previous evaluation (F_0 at init); implies objective_every >= 1 */
  uint32_t min_pass;        /* never stop before this many epochs */
} ocffm_solve_opts;
typedef struct ocffm_solve_report {
  uint32_t epochs;
  int32_t converged;
  double objective0, objective;
} ocffm_solve_report;
int ocffm_problem_solve_ex(ocffm_problem *p, const ocffm_solve_opts *o, ocffm_solve_report *rep);

/* ImpProblem::validate (ffm.cpp:925-1016): loss = sqrt(ploss/m_te), p@k and
 * nDCG@k at k = 5,10,20,40,80. */
typedef struct ocffm_metrics {
  double loss;
  double prec[5];
  double ndcg[5];
  uint32_t top_k[5];
} ocffm_metrics;
int ocffm_problem_validate(ocffm_problem *p, ocffm_metrics *out);
/* The reference's nDCG known-answer build (-DEBUG_nDCG -DSHOW_SCORE_ONLY,
 * script/nDCG_degub_tool/readme:1-4): validate() with every test row's
 * scores forced to z_j = n - j after its ploss term (ffm.cpp:988-993).
 * per_row_ndcg (optional, room for cap doubles): nDCG@5,10,20,40,80 of each
 * of this rank's test rows, row-major (ffm.cpp:1059-1128; the build prints
 * the @10 value per row, ffm.cpp:1126).  OCFFM_E_ARG when cap < 5 x
 * ocffm_problem_test_rows(). */
int ocffm_problem_validate_forced(ocffm_problem *p, ocffm_metrics *out, double *per_row_ndcg, uint64_t cap);
/* Test rows of this rank (Uva->m of the reference, ffm.cpp:925; 0 without a
 * test set). */
int ocffm_problem_test_rows(ocffm_problem *p, uint64_t *m);

/* Top-N recommendation (no reference counterpart: the reference only scores
 * inside validate).  Top-N items for rows [row0, row0+rows) of X under the
 * current model.
 * X: user rows in the train set's field space (read with the train Ds, as a
 * test file is).  items: rows x topn, row-major.  scores (may be NULL): the
 * same shape, the model's prediction  a_i + b_j + sum_c <P_c[i], Q_c[j]>
 * (pred_z, ffm.cpp:915-923, plus the row's own side term a_i, which is added
 * before the selection so that the order below is the order of the returned
 * values).  Order: score descending, equal scores by ascending item index.
 * Does not change the solver state.
 *  - Candidates: every item row j < n of V.  With OCFFM_REC_EXCLUDE_LABELS in
 *    flags, the row's own labels in X are excluded (labels >= n are ignored,
 *    and so is the flag when X has no labels).
 *  - Cold rows: a row with no kept feature node is scored as validate scores
 *    it (ffm.cpp:975-977): its candidates are j < npop (the train set's
 *    max label + 1), its scores the train popularity values; the same
 *    ordering and exclusion rules hold.
 *  - Short rows: a row with fewer than topn candidates has OCFFM_REC_NONE and
 *    a score of -inf in the remaining slots.
 *  - Arithmetic: the problem's precision (fp32 tables and accumulation in
 *    OCFFM_FP32, fp64 in OCFFM_FP64), returned as fp64.
 *  - Reproducibility: a row's result is the same bit for bit between calls
 *    and does not depend on its position in the call nor on how the call was
 *    chunked or the items sliced (OCFFM_REC_ROWS, OCFFM_REC_SLICES): the
 *    selection is on the total order (score, item index).
 *  - Errors: OCFFM_E_STATE before init / load_binary; OCFFM_E_ARG for
 *    topn == 0, topn > OCFFM_REC_MAX_TOPN, row0 + rows > X.m, NULL items, or
 *    an X with more fields than the train set's user side; OCFFM_E_DATA for
 *    a node of X with idx >= Ds[fid].  rows == 0 is OCFFM_OK.
 *  - Sharded problems: the owned tables are made whole first, as in
 *    validate; X is not sharded, each rank scores the rows it passes.  This
 *    has only been run on one rank.
 * The launches are the kernel family "recommend" of the statistics below;
 * the counter "rec_setup_us" holds the last call's host-side set-up time. */
#define OCFFM_REC_MAX_TOPN 128
#define OCFFM_REC_EXCLUDE_LABELS 1u /* flags bit: drop each row's own labels from its candidates */
#define OCFFM_REC_NONE 0xffffffffu  /* item id of an unfilled slot */
int ocffm_problem_recommend(ocffm_problem *p, const ocffm_data *X, uint64_t row0, uint64_t rows, uint32_t topn,
                            uint32_t flags, uint32_t *items, double *scores);

/* Exact label ranks (no reference counterpart).  For every label of X, its
 * rank among the candidates of its row under the current model: the 0-based
 * number of candidates that come before it in the order of
 * ocffm_problem_recommend (score descending, equal scores by ascending item
 * index; ties are thus broken by item index).  The other labels of the row
 * count as candidates too.
 * X: labelled user rows in the train set's field space (read with the train
 * Ds).  ranks, scores (may be NULL): one entry per label of X in
 * ocffm_data_get_labels order (info.nnz_y entries); a score is the value
 * ocffm_problem_recommend returns for that (row, item), bit for bit.
 * ncand (may be NULL): the candidate count of each of the X.m rows.
 * Does not change the solver state.
 *  - Candidates of row i: every item j < n of V; for a cold row (no kept
 *    feature node) j < npop, scored by train popularity as in recommend.
 *    With seen != NULL the labels of seen's row i are removed (seen.m must
 *    equal X.m; its labels >= n are ignored).
 *  - Labels that are not candidates (>= n, >= npop on a cold row, or present
 *    in seen) get OCFFM_RANK_NONE and a score of -inf.
 *  - Duplicate labels: every copy gets the same rank and score.
 *  - Arithmetic and reproducibility: as ocffm_problem_recommend.  A label's
 *    rank and score are the same bit for bit between calls and do not depend
 *    on the row's position in X nor on OCFFM_REC_ROWS / OCFFM_REC_SLICES,
 *    which chunk and slice this call as well.  No rows x n array is built.
 *  - Errors: OCFFM_E_STATE before init / load_binary; OCFFM_E_ARG for NULL
 *    ranks, an X without labels, seen.m != X.m, or an X with more fields than
 *    the train set's user side; OCFFM_E_DATA for a node of X with
 *    idx >= Ds[fid].  X.m == 0 is OCFFM_OK.
 *  - Sharded problems: the owned tables are made whole first, as in
 *    validate; X is not sharded, each rank ranks the rows it passes.  This
 *    has only been run on one rank.
 * The launches are the kernel family "evaluate" of the statistics below; the
 * counter "eval_setup_us" holds the last call's host-side set-up time. */
#define OCFFM_RANK_NONE 0xffffffffu
int ocffm_problem_label_ranks(ocffm_problem *p, const ocffm_data *X, const ocffm_data *seen, uint32_t *ranks,
                              double *scores, uint32_t *ncand);

/* Scores of given pairs (no reference counterpart).  out[e] is the score of
 * row prow[e] of X and item pitem[e] under the current model, e < npairs: the
 * value ocffm_problem_recommend and ocffm_problem_label_ranks return for that
 * (row, item), bit for bit, in either precision (the same chain: chunks of 16
 * depth elements in order, then (acc + b_j) + a_i, widened to fp64).
 * X: user rows in the train set's field space (read with the train Ds); its
 * labels, if any, play no part.  Does not change the solver state.
 *  - Cold rows: a row with no kept feature node scores popular[j], the train
 *    popularity value, as in recommend.
 *  - Pairs that are no candidates: pitem[e] >= n, or >= npop on a cold row,
 *    score -inf.  Repeated pairs are scored each.
 *  - Reproducibility: a pair's score does not depend on its place in the call
 *    nor on the other pairs.
 *  - Errors: OCFFM_E_STATE before init / load_binary; OCFFM_E_ARG for
 *    prow[e] >= X.m, a NULL prow / pitem / out with npairs > 0, or an X with
 *    more fields than the train set's user side; OCFFM_E_DATA for a node of X
 *    with idx >= Ds[fid] (every row of X is checked and laid out, also those
 *    no pair names).  npairs == 0 is OCFFM_OK.
 *  - Sharded problems: as ocffm_problem_recommend.
 * The launch belongs to the kernel family "rerank" of the statistics below;
 * the counter "rec_setup_us" holds the last call's host-side set-up time. */
int ocffm_problem_score(ocffm_problem *p, const ocffm_data *X, uint64_t npairs, const uint32_t *prow,
                        const uint32_t *pitem, double *out);

/* Top-N of each row's own candidate list (no reference counterpart): what a
 * retrieval stage, a stock filter or a sampled-negatives harness asks of a
 * trained model.  For rows [row0, row0 + rows) of X; the list of row
 * row0 + i is ccol[cptr[i] .. cptr[i + 1]), in any order: cptr holds
 * rows + 1 non-decreasing offsets with cptr[0] == 0.
 * items, scores (may be NULL): rows x topn, row-major, with exactly
 * ocffm_problem_recommend's shape, order and values: score descending, equal
 * scores by ascending item index, every score the value recommend returns for
 * that (row, item) bit for bit.  Does not change the solver state.
 *  - Candidates of a row: the distinct entries of its list that are
 *    candidates in recommend's sense: < n (every item row of V), or < npop on
 *    a cold row (scored by train popularity), minus the row's own labels in X
 *    when OCFFM_REC_EXCLUDE_LABELS is set in flags.  Other entries are
 *    ignored; a duplicate counts once.
 *  - Short rows: a row with fewer than topn candidates has OCFFM_REC_NONE and
 *    a score of -inf in the remaining slots; an empty list gives a row of
 *    those.
 *  - Cost: the item rows of the list entries are gathered; no sweep over the
 *    n items takes place and scratch is (list segments) x topn entries.
 *  - Reproducibility: a row's result is the same bit for bit between calls
 *    and does not depend on its position in the call, on the order of its
 *    list, on OCFFM_REC_ROWS (rows per chunk) nor on how the list was cut
 *    into segments (OCFFM_REC_SEG): the selection is on the total order
 *    (score, item index) over distinct items.
 *  - Errors: those of ocffm_problem_recommend (OCFFM_E_STATE before init /
 *    load_binary; OCFFM_E_ARG for topn == 0, topn > OCFFM_REC_MAX_TOPN,
 *    row0 + rows > X.m, NULL items, or an X with more fields than the train
 *    set's user side; OCFFM_E_DATA for a node of X with idx >= Ds[fid]), and
 *    OCFFM_E_ARG for a NULL cptr, cptr[0] != 0, a decreasing cptr, or a NULL
 *    ccol with cptr[rows] > 0.  rows == 0 is OCFFM_OK.
 *  - Sharded problems: the owned tables are made whole first, as in
 *    validate; X is not sharded, each rank scores the rows it passes.  This
 *    has only been run on one rank.
 * The launches are the kernel family "rerank" of the statistics below; the
 * counter "rec_setup_us" holds the last call's host-side set-up time. */
int ocffm_problem_recommend_among(ocffm_problem *p, const ocffm_data *X, uint64_t row0, uint64_t rows,
                                  const uint64_t *cptr, const uint32_t *ccol, uint32_t topn, uint32_t flags,
                                  uint32_t *items, double *scores);

/* Ranking metrics from label ranks.  ocffm_eval_from_ranks is pure host code
 * (no GPU, no problem): yptr holds the m + 1 label offsets of the rows,
 * ranks / scores (may be NULL: loss 0) / ncand the outputs of
 * ocffm_problem_label_ranks.  Sums are taken in fp64 in row order.
 * A row's ranked labels are its distinct labels with a rank other than
 * OCFFM_RANK_NONE: P of them, ranks r_1 < ... < r_P (copies of a label share
 * a rank and count once).  rows_used counts the rows with P >= 1; every mean
 * below is over those rows, the others are skipped; with rows_used == 0
 * every metric is 0.  labels = yptr[m], labels_ranked = the sum of P.
 * For a cut c the hits are the labels with r < c:
 *   prec   = hits / c  (the divisor is c even with fewer candidates, as in
 *            the reference's prec_k)
 *   recall = hits / P
 *   ndcg   = sum_hits 1/log2(r + 2)  /  sum_{t < min(c, P)} 1/log2(t + 2)
 *   map    = (1 / min(c, P)) sum_{hits t} t / (r_t + 1), t the label's
 *            1-based index among the row's ranked labels
 *   hit    = 1 if hits > 0, else 0
 * and without a cut:
 *   mrr    = 1 / (r_1 + 1)
 *   auc    = 1 - sum_t (r_t - (t - 1)) / (P (ncand - P)): the fraction of
 *            (label, other candidate) pairs the model orders correctly, ties
 *            broken by item index; a row with ncand == P is left out of this
 *            mean (which is over the remaining rows)
 *   loss   = sqrt(sum over ranked labels of (1 - s)^2 / rows_used), the
 *            ploss of validate.
 * cuts: 1 <= ncut <= OCFFM_EVAL_MAX_CUTS values >= 1, strictly increasing;
 * otherwise OCFFM_E_ARG, as for a NULL yptr / ranks / ncand / cuts / out.
 * ocffm_problem_evaluate is ocffm_problem_label_ranks followed by
 * ocffm_eval_from_ranks, with the errors of both. */
#define OCFFM_EVAL_MAX_CUTS 8
typedef struct ocffm_eval {
  uint64_t rows, rows_used, labels, labels_ranked;
  uint32_t ncut, cuts[8];
  double loss, mrr, auc, prec[8], recall[8], ndcg[8], map[8], hit[8];
} ocffm_eval;
int ocffm_eval_from_ranks(uint64_t m, const uint64_t *yptr, const uint32_t *ranks, const double *scores,
                          const uint32_t *ncand, const uint32_t *cuts, uint32_t ncut, ocffm_eval *out);
int ocffm_problem_evaluate(ocffm_problem *p, const ocffm_data *X, const ocffm_data *seen, const uint32_t *cuts,
                           uint32_t ncut, ocffm_eval *out);

/* Label ranks among per-row candidate lists (no reference counterpart): the
 * sampled-negatives protocol ("1 positive + 99 / 999 sampled negatives") and
 * the short-list of a retrieval stage.  ocffm_problem_label_ranks with each
 * row ranked among its own list instead of among every item.  Covers all X.m
 * rows; the list of row i is ccol[cptr[i] .. cptr[i + 1]), in any order and
 * with repeats: cptr holds X.m + 1 non-decreasing offsets with cptr[0] == 0.
 * ranks, scores (may be NULL), ncand (may be NULL): as in
 * ocffm_problem_label_ranks.  Does not change the solver state.
 *  - Candidate set K_i of row i.  A candidate is defined as in
 *    ocffm_problem_label_ranks: < n, or < npop on a cold row, and not among
 *    seen's labels of row i.  K_i is the distinct entries of the list that are
 *    candidates, united with the row's own labels that are candidates: the
 *    positive is ranked whether or not the caller put it in the list.  A
 *    duplicate counts once; other entries are ignored.
 *  - Rank of a label: the 0-based number of members of K_i before it in
 *    ocffm_problem_recommend's total order (score descending, equal scores by
 *    ascending item index).  The other labels of the row count, as in
 *    label_ranks.  ncand[i] = |K_i| for every row; an empty list gives the
 *    number of the row's candidate labels.  Labels that are no candidates get
 *    OCFFM_RANK_NONE and -inf; copies of a label share a rank.
 *  - Scores: the value ocffm_problem_score returns for that pair, bit for bit.
 *  - Reproducibility: ranks, scores and ncand do not depend on the order of
 *    the list, on OCFFM_REC_ROWS, on OCFFM_REC_SEG nor on scheduling: K_i is a
 *    set, built on the host, and all cross-wave accumulation is integer adds.
 *  - Consequence: when every list holds all of 0..n-1, the three outputs
 *    equal ocffm_problem_label_ranks's.
 *  - Cost: the item rows of K_i are gathered, for the rows that have a
 *    candidate label; a row without one is only counted.  No sweep over the n
 *    items takes place.  There is no cap on a row's list.
 *  - Errors: those of ocffm_problem_label_ranks, and OCFFM_E_ARG for a NULL
 *    cptr, cptr[0] != 0, a decreasing cptr, or a NULL ccol with cptr[m] > 0.
 *    X.m == 0 is OCFFM_OK.
 *  - Sharded problems: as ocffm_problem_recommend_among.
 * ocffm_problem_evaluate_among is this followed by ocffm_eval_from_ranks,
 * with the errors of both.  The launches belong to the kernel family
 * "evaluate"; the counter "eval_setup_us" holds the last call's host-side
 * set-up time (the construction of the K_i included). */
int ocffm_problem_label_ranks_among(ocffm_problem *p, const ocffm_data *X, const ocffm_data *seen,
                                    const uint64_t *cptr, const uint32_t *ccol, uint32_t *ranks, double *scores,
                                    uint32_t *ncand);
int ocffm_problem_evaluate_among(ocffm_problem *p, const ocffm_data *X, const ocffm_data *seen,
                                 const uint64_t *cptr, const uint32_t *ccol, const uint32_t *cuts, uint32_t ncut,
                                 ocffm_eval *out);

/* print_epoch_info (ffm.cpp:1130-1145) of the last validation, and the
 * header of init_va (ffm.cpp:901-912), to stdout. */
int ocffm_print_header(void);
int ocffm_print_epoch(const ocffm_metrics *m, uint32_t iter);

/* State access (copies to host as fp64).  what: 'W','H','P','Q' (block
 * b12 = index_vec(f1,f2,f), ffm.cpp:53-55), 'a','b' (biases), 's','t'
 * (sa, sb), 'u' (user-major y-tilde), 'v' (item-major y-tilde).  Returns
 * the element count in *len; copies min(cap, count) values when out != 0.
 * Under sharding, row-indexed user-side arrays are this rank's rows. */
int ocffm_problem_get(ocffm_problem *p, char what, uint32_t b12, double *out, uint64_t cap, uint64_t *len);
/* Overwrite W or H of block b12 (P/Q are recomputed); for tests. */
int ocffm_problem_set(ocffm_problem *p, char what, uint32_t b12, const double *in, uint64_t len);

/* Kernel-level entry points for parity tests.  Gradient of one half
 * (gd_side / gd_cross, ffm.cpp:537-592, 630-703) and lam*v + H(v) of one
 * half (the product inside cg(), ffm.cpp:783-801).  half 0 = W of block
 * (f1,f2), half 1 = H.  Neither changes the solver state. */
int ocffm_problem_grad(ocffm_problem *p, uint32_t f1, uint32_t f2, int half, double *out);
int ocffm_problem_hv(ocffm_problem *p, uint32_t f1, uint32_t f2, int half, const double *v, double *out);

/* save_model (ffm.cpp:1163-1237): the reference's text model format. */
int ocffm_problem_save_model(ocffm_problem *p, const char *path);

/* ImpProblem::save_binary_model (ffm.cpp:1239-1267): W and H of every used
 * block in the reference's binary layout (uint32 f, fu, fv, k; uint64 Ds;
 * per block uint32 index_vec, uint64 |W|, uint64 |H|, doubles). */
int ocffm_problem_save_binary(ocffm_problem *p, const char *path);
/* ImpProblem::load_binary_model (ffm.cpp:1269-1301) as it was meant to work
 * (the reference's opens an ofstream and writes): reads that layout, checks
 * f/fu/fv/k/Ds against this problem, restores W/H and re-derives P, Q, the
 * biases, sa/sb and y-tilde as ocffm_problem_init does.  May replace init. */
int ocffm_problem_load_binary(ocffm_problem *p, const char *path);

/* Statistics.  cg: CG iteration count of every half solved since the last
 * reset (solve order).  Kernel timing is recorded with HIP events on the
 * solver's stream when profiling is on. */
typedef struct ocffm_kernel_stat {
  char name[32];
  uint64_t launches;
  double total_ms;     /* summed event-measured duration        */
  double alg_bytes;    /* summed algorithmic bytes  */
  double alg_flops;    /* summed floating-point ops (MFMA kernels; else 0) */
} ocffm_kernel_stat;
int ocffm_problem_cg_log(ocffm_problem *p, int32_t *out, int cap, int *count);
int ocffm_problem_set_profiling(ocffm_problem *p, int on);
/* Restrict event timing to the kernel family `name` (NULL or "" = all). */
int ocffm_problem_set_profile_filter(ocffm_problem *p, const char *name);
int ocffm_problem_kernel_stats(ocffm_problem *p, ocffm_kernel_stat *out, int cap, int *count);
int ocffm_problem_reset_stats(ocffm_problem *p);
/* Algorithmic HBM bytes of the epochs run since the last reset
 * (SURVEY §8d formula with the actual CG counts). */
int ocffm_problem_alg_bytes(ocffm_problem *p, double *bytes);
/* Diagnostic event counters since create (no reference counterpart):
 * "cgp_launches" (persistent CG launches: column-Gram and id-like side
 * halves), "cgp_side_launches" (the latter), "cgp_side_full" (side halves
 * whose gradient and update ran inside the launch), "cgp_recovered"
 * (launches whose grid gave up on its barrier and whose solve was finished
 * per step), "cgp_refused" (cooperative launches the runtime refused),
 * "cgp_side_sm1" / "_sm2" / "_sm4" (id-like side launches by rows per
 * subgroup) and "cgp_side_res_sm1" / "_sm2" / "_sm4" (the resident grid last
 * found for that variant, in blocks), "xfuse_steps" (fused id-field cross
 * steps) and "xfuse_strided" (those on fewer blocks than their rows fill),
 * "ccg_halves" (cross halves solved on per-column Grams), "hot_halves"
 * (cross halves whose steps read hot rows' Grams), "capped_launches"
 * (launches whose grid a residency or *_BLOCKS cap cut below its work, so
 * that its blocks loop), "pcol_gd" / "pcol_hs" (cross gradient / Hessian-
 * vector row passes that gathered a partner field's own table through
 * partner columns, OCFFM_PCOL) and "pcol_bytes" (bytes of those column
 * arrays), "obj_us" (wall time of the last ocffm_problem_objective call, in
 * microseconds).  An unknown name reads 0. */
int ocffm_problem_counter(ocffm_problem *p, const char *name, int64_t *value);
int ocffm_problem_sync(ocffm_problem *p);
/* Digests (FNV-1a over the bytes) of every array of the device data layout
 * the problem built from its ImpData (per-field CSR of split_fields,
 * ffm.cpp:185-257; the item-major positives of transY, ffm.cpp:259-294; the
 * popularity, ffm.cpp:143,172-176; the CSCs, jobs and segments), in a fixed
 * order.  The layout is built on the device unless OCFFM_HOST_BUILD=1 was
 * set at create; both builds give the same digests.  names: cap x 48 chars
 * (may be NULL); *count receives the number of entries. */
int ocffm_problem_layout_digest(ocffm_problem *p, char *names, uint64_t *digests, int cap, int *count);
void ocffm_problem_destroy(ocffm_problem *p);

/* ------------------------------------------------------------ SGD mode
 * BASELINE.json north_star extras, NO reference counterpart (the reference
 * trains only by block Newton-CG): field-aware FM trained per instance by
 * SGD / AdaGrad with lock-free (HOGWILD) writes to W, each positive
 * (user row, item row) of U drawing `nneg` negatives on the device from an
 * alias table over item popularity^neg_power; log-loss.  Instance nodes =
 * the user row's nodes then the item row's (global feature id = field
 * offset + idx).  Parity against oracle/sgd_oracle.cpp (a serial CPU
 * statement), not against the reference ("parity unpinned"). */
typedef struct ocffm_sgd ocffm_sgd;
typedef struct ocffm_sgd_param {
  uint32_t k;          /* latent dimension (1..128)                         */
  float eta;           /* learning rate (libffm default 0.2)                */
  float lambda;        /* L2 (libffm default 2e-5)                          */
  uint32_t nneg;       /* sampled negatives per positive                    */
  double neg_power;    /* alias weights = item label count ^ neg_power      */
  int32_t adagrad;     /* 1: AdaGrad (G starts at 1), 0: plain SGD          */
  int32_t norm;        /* 1: instance-wise 1/|x|^2 normalisation            */
  int32_t serial;      /* 1: one wave, instances in order (parity tests)    */
  uint64_t seed;       /* W init, instance order, negative draws            */
  int32_t device;
} ocffm_sgd_param;
typedef struct ocffm_sgd_info {
  uint64_t n_features; /* NF: rows of W (all fields)      */
  uint32_t n_fields;   /* F                               */
  uint32_t kp;         /* padded row length               */
  uint64_t positives;  /* this rank's positives           */
  uint64_t instances;  /* per epoch: positives (1 + nneg) */
} ocffm_sgd_info;
void ocffm_sgd_param_default(ocffm_sgd_param *p);
int ocffm_sgd_create(const ocffm_data *U, const ocffm_data *V, const ocffm_sgd_param *p, ocffm_sgd **out);
/* One process per GPU: this rank trains on its contiguous user shard's
 * positives; ocffm_sgd_average() makes W and G the mean over the ranks
 * (RCCL all-reduce over xGMI) — periodic model averaging. */
int ocffm_sgd_create_dist(const ocffm_data *U, const ocffm_data *V, const ocffm_sgd_param *p, int rank, int nranks,
                          const void *comm_id, ocffm_sgd **out);
/* The same with ocffm_sgd_average's sums staged through host memory and
 * handed to fn (float arrays: W, then G) — tests of the sharding on one GPU. */
int ocffm_sgd_create_dist_host(const ocffm_data *U, const ocffm_data *V, const ocffm_sgd_param *p, int rank,
                               int nranks, ocffm_allreduce_fn fn, void *user, ocffm_sgd **out);
int ocffm_sgd_epoch(ocffm_sgd *s, double *mean_loss);
int ocffm_sgd_average(ocffm_sgd *s);
/* phi for n (user row, item row) pairs with the current W. */
int ocffm_sgd_phi(ocffm_sgd *s, uint64_t n, const uint32_t *users, const uint32_t *items, float *out);
/* what: 'W' / 'G' (float, NF x F x kp), 'p' alias probabilities (float),
 * 'a' alias targets (uint32), 'o' last epoch's order (uint64 A, B, T). */
int ocffm_sgd_get(ocffm_sgd *s, char what, void *out, uint64_t cap, uint64_t *len);
int ocffm_sgd_set_w(ocffm_sgd *s, const float *w, uint64_t n);
int ocffm_sgd_get_info(ocffm_sgd *s, ocffm_sgd_info *out);
int ocffm_sgd_sync(ocffm_sgd *s);

/* Top-N recommendation under the trainer's current W: the shape, order and
 * rules of ocffm_problem_recommend on the SGD model.  Top-N items for rows
 * [row0, row0+rows) of X; items: rows x topn, row-major; scores (may be NULL):
 * the same shape.  Order: score descending, equal scores by ascending item
 * index.  Does not change W or G.
 * X: user rows in the train set's field space (read with the train Ds, as a
 * test file is); their nodes are laid out as the train rows' are (global
 * feature id = field offset + idx; field-major within a row, file order
 * within a field).
 *  - Scores: phi of ocffm_sgd_phi, decomposed so that no rows x n array is
 *    built.  A node a of a row has feature j_a, field f_a, value x_a; user
 *    fields are 0..fu-1, item fields fu..F-1; U_i the nodes of user row i,
 *    V_j those of item row j; W[j][f] the kp-long row of feature j towards
 *    field f.  Cross block c = f fv + (g - fu) for f < fu, g >= fu (the Newton
 *    problem's order), C = fu fv:
 *      P_c[i] = sum_{a in U_i, f_a = f} x_a W[j_a][g]
 *      Q_c[j] = sum_{b in V_j, f_b = g} x_b W[j_b][f]
 *      A_i    = sum_{a < a' in U_i} x_a x_a' <W[j_a][f_a'], W[j_a'][f_a]>
 *      B_j    = the same sum over V_j
 *      su_i   = sum_{a in U_i} x_a^2,   sv_j = sum_{b in V_j} x_b^2
 *      s(i,j) = ((acc + B_j) + A_i) rn
 *    acc: sum_c <P_c[i], Q_c[j]> in ocffm_problem_recommend's chain (chunks of
 *    16 depth elements in order over the depth C kp); rn = 1 for a trainer
 *    with norm = 0, else 1 / (su_i + sv_j) where that sum is > 0 and 1 where
 *    it is 0.  All sums are fp32 in node order; the result is returned as
 *    fp64.  In exact arithmetic this is phi: pairs of user nodes give A_i,
 *    pairs of item nodes B_j, a user node in field f and an item node in
 *    field g one term of <P_c[i], Q_c[j]>.  A feature that appears twice in
 *    a row counts as two nodes, as in phi.
 *  - Agreement with ocffm_sgd_phi: to fp32 rounding only, because phi sums
 *    the same products in another order.
 *  - Candidates: every item row j < V.m of every row.  With
 *    OCFFM_REC_EXCLUDE_LABELS in flags, the row's own labels in X are excluded
 *    (labels >= V.m are ignored, and so is the flag when X has no labels).
 *  - No cold rows and no popularity fallback: a row without nodes has P = 0,
 *    A = 0, su = 0 and is scored by B_j rn; an item row without nodes scores
 *    A_i rn.
 *  - Short rows: a row with fewer than topn candidates has OCFFM_REC_NONE and
 *    a score of -inf in the remaining slots.
 *  - Reproducibility: a (row, item) score has the same bits in this call, in
 *    ocffm_sgd_label_ranks and between calls on an unchanged W, and does not
 *    depend on the row's position in the call nor on how the call was chunked
 *    or the items sliced (OCFFM_REC_ROWS, OCFFM_REC_SLICES, read at create):
 *    the selection is on the total order (score, item index).
 *  - The item side (Q_c, B, sv) is projected on the first serving call and
 *    again only after W changed (ocffm_sgd_epoch, ocffm_sgd_average,
 *    ocffm_sgd_set_w); the rows of X are projected per call.
 *  - Errors: OCFFM_E_ARG for topn == 0, topn > OCFFM_REC_MAX_TOPN,
 *    row0 + rows > X.m, NULL items, and for a trainer with no user field or no
 *    item field (no cross block); OCFFM_E_DATA for a node of the call's rows
 *    with fid >= fu or idx >= Ds[fid].  There is no OCFFM_E_STATE case: a
 *    trainer always has a W.  rows == 0 is OCFFM_OK.
 *  - Sharded trainers: every rank holds a whole W, so each rank serves the
 *    rows it is given from its own current W; X is not sharded.  This has
 *    only been run on one rank.
 * Out of this path: fp64. */
int ocffm_sgd_recommend(ocffm_sgd *s, const ocffm_data *X, uint64_t row0, uint64_t rows, uint32_t topn,
                        uint32_t flags, uint32_t *items, double *scores);
/* Exact label ranks under the current W: ocffm_problem_label_ranks on the SGD
 * model.  For every label of X its 0-based rank among the candidates of its
 * row in ocffm_sgd_recommend's order, and (scores, may be NULL) the value
 * ocffm_sgd_recommend returns for that (row, item), bit for bit; one entry per
 * label in ocffm_data_get_labels order.  ncand (may be NULL): the candidate
 * count of each of the X.m rows.
 *  - Candidates of row i: every item j < V.m; with seen != NULL the labels of
 *    seen's row i are removed (seen.m must equal X.m; its labels >= V.m are
 *    ignored).  The other labels of the row count as candidates.
 *  - Labels that are not candidates (>= V.m, or present in seen) get
 *    OCFFM_RANK_NONE and a score of -inf.  Every copy of a duplicate label
 *    gets the same rank and score.
 *  - Arithmetic, reproducibility, the item-side cache and sharded trainers:
 *    as ocffm_sgd_recommend.
 *  - Errors: OCFFM_E_ARG for NULL ranks, an X without labels, seen.m != X.m,
 *    or a trainer without a cross block; OCFFM_E_DATA for a node of X with
 *    fid >= fu or idx >= Ds[fid].  X.m == 0 is OCFFM_OK. */
int ocffm_sgd_label_ranks(ocffm_sgd *s, const ocffm_data *X, const ocffm_data *seen, uint32_t *ranks,
                          double *scores, uint32_t *ncand);
/* ocffm_sgd_label_ranks followed by ocffm_eval_from_ranks (whose argument
 * errors it shares: the cuts, NULL out). */
int ocffm_sgd_evaluate(ocffm_sgd *s, const ocffm_data *X, const ocffm_data *seen, const uint32_t *cuts,
                       uint32_t ncut, ocffm_eval *out);
/* Pair scores and candidate lists on the SGD model: the Newton entries
 * (ocffm_problem_score, ocffm_problem_recommend_among,
 * ocffm_problem_label_ranks_among, ocffm_problem_evaluate_among) with their
 * shape, order, short-row and duplicate rules, on ocffm_sgd_recommend's
 * scores: a (row, item) pair has the bits ocffm_sgd_recommend and
 * ocffm_sgd_label_ranks give it.
 *  - There are no cold rows: candidates are the items < V.m (minus the row's
 *    own labels under OCFFM_REC_EXCLUDE_LABELS, or seen's labels of the row).
 *    ocffm_sgd_score gives -inf for pitem[e] >= V.m.
 *  - The item side comes from the same cache that follows the model version
 *    ("rank_item_builds" rises once per model change, not per call).
 *  - ocffm_sgd_label_ranks_among: when every list holds all of 0..V.m-1 the
 *    three outputs equal ocffm_sgd_label_ranks's.
 *  - Reproducibility: as the Newton entries (OCFFM_REC_ROWS and OCFFM_REC_SEG
 *    are read at create).
 *  - Errors: those of ocffm_sgd_recommend (label ranks: ocffm_sgd_label_ranks;
 *    evaluate: ocffm_sgd_evaluate), OCFFM_E_ARG for a NULL cptr, cptr[0] != 0,
 *    a decreasing cptr, or a NULL ccol with cptr[rows] > 0; for the pairs
 *    OCFFM_E_ARG for prow[e] >= X.m or a NULL prow / pitem / out with
 *    npairs > 0 (every row of X is checked and laid out).  npairs == 0,
 *    rows == 0 and X.m == 0 are OCFFM_OK.
 * The counters are ocffm_sgd_counter's: "rank_setup_us", "rank_kernel_us". */
int ocffm_sgd_score(ocffm_sgd *s, const ocffm_data *X, uint64_t npairs, const uint32_t *prow, const uint32_t *pitem,
                    double *out);
int ocffm_sgd_recommend_among(ocffm_sgd *s, const ocffm_data *X, uint64_t row0, uint64_t rows, const uint64_t *cptr,
                              const uint32_t *ccol, uint32_t topn, uint32_t flags, uint32_t *items, double *scores);
int ocffm_sgd_label_ranks_among(ocffm_sgd *s, const ocffm_data *X, const ocffm_data *seen, const uint64_t *cptr,
                                const uint32_t *ccol, uint32_t *ranks, double *scores, uint32_t *ncand);
int ocffm_sgd_evaluate_among(ocffm_sgd *s, const ocffm_data *X, const ocffm_data *seen, const uint64_t *cptr,
                             const uint32_t *ccol, const uint32_t *cuts, uint32_t ncut, ocffm_eval *out);
/* Serving counters; an unknown name reads 0 (as ocffm_problem_counter).
 *  rank_item_builds    item-side projections since create
 *  rank_setup_us       the last serving call's host set-up (the item-side
 *                      projection included when it ran)
 *  rank_item_build_us  the last item-side projection
 *  rank_kernel_us      the last call's sweep, list, merge and pair-score launches,
 *                      between HIP events on the trainer's stream */
int ocffm_sgd_counter(ocffm_sgd *s, const char *name, int64_t *value);
void ocffm_sgd_destroy(ocffm_sgd *s);

/* ------------------------------------------------------- saved models
 * Serving from a saved model (no reference counterpart: the reference writes
 * its model files and reads none).  An ocffm_model holds, on one device, the
 * field space (f, fu, fv, k, Ds), W and H of every used block padded as the
 * problem pads them, the current item catalogue in the serving sweeps' form
 * (the item-side cross tables Q_c, n x kp, and b_j) and an optional popularity
 * vector.  It holds no training rows.  Single GPU only: a model is neither
 * sharded nor replicated; one host thread drives it. */
typedef struct ocffm_model ocffm_model;

typedef struct ocffm_model_info {
  uint32_t f, fu, fv, k, kp; /* fields (all, user, item); latent dimension and its padded length */
  uint32_t nblocks, nused;   /* f (f + 1) / 2 field-pair blocks; those with tables                */
  int32_t self_side;         /* 1: the side blocks are used (0: a model trained with --ns)        */
  int32_t precision, device; /* of a model; 0 and -1 from ocffm_model_file_info                   */
  int32_t has_items;         /* a catalogue is set                                                */
  uint64_t n, npop;          /* catalogue items; popularity entries                               */
  /* in: NULL, or room for ds_cap / used_cap values; out: Ds of the f fields
   * (user fields first) and one flag per block b12 = index_vec(f1, f2, f). */
  uint64_t *Ds;
  uint8_t *used;
  uint32_t ds_cap, used_cap;
} ocffm_model_info;

/* Reads and fully validates a model file on the host; no device is touched.
 * binary == 0: the text model ocffm_problem_save_model writes (header lines
 * f, fu, fv, k, then the Ds; table lines "W|H,f1,f2,row v1 ... vk", blocks in
 * (f1, f2) order, W before H, rows in order).  binary != 0: the layout
 * documented at ocffm_problem_save_binary.  The side blocks are either all
 * present or all absent (--ns: unused blocks).
 * OCFFM_E_IO for a path that cannot be read.  OCFFM_E_DATA for a text file
 * with an absent cross block, a block with only one of W / H, a missing,
 * repeated or out-of-order row, a wrong value count, a non-numeric token or
 * trailing text; for a binary file that is truncated, has a wrong block
 * index or table size, or trailing bytes; for either with f != fu + fv,
 * k outside 1..128 or only some of the side blocks. */
int ocffm_model_file_info(const char *path, int binary, ocffm_model_info *out);

/* A model from a file (the checks of ocffm_model_file_info; a bad file leaves
 * no object behind), with its tables in `precision` (OCFFM_FP64 / OCFFM_FP32)
 * on `device`.  The text model holds six significant digits per value. */
int ocffm_model_load_text(const char *path, int precision, int device, ocffm_model **out);
int ocffm_model_load_binary(const char *path, int precision, int device, ocffm_model **out);
/* A model from a problem's current state, copied device to device: W / H, and
 * as its catalogue the problem's resident item side (Q and b, which training
 * updates incrementally) and its popularity, so that every serving result on
 * the training catalogue has the problem's own bits.  Precision and device are
 * the problem's.  OCFFM_E_STATE before init / load_binary; OCFFM_E_ARG for a
 * sharded problem. */
int ocffm_model_from_problem(ocffm_problem *p, ocffm_model **out);

/* Replaces the catalogue by the rows of V, any item rows in the model's item
 * field space: read them with the model's item Ds (ocffm_model_get_ds, the
 * last fv values), as a test file is read with the train Ds.  The rows are
 * laid out per field and projected on the device through W / H (Q_c[j] and
 * b_j in the arithmetic of the problem's own projection, bit for bit).  The
 * popularity is cleared.  V.m == 0 gives an empty catalogue: every serving
 * call then returns OCFFM_REC_NONE / -inf / OCFFM_RANK_NONE.
 * OCFFM_E_ARG for more fields than fv; OCFFM_E_DATA for a node with
 * idx >= Ds[fid].  The counter "project_us" holds the projection's time. */
int ocffm_model_set_items(ocffm_model *m, const ocffm_data *V);
/* The cold rows' scores: pop[j] for the catalogue items j < min(npop, n); the
 * indices are catalogue indices (rows of the last ocffm_model_set_items), not
 * the labels of any training set.  Without it (npop == 0 clears it) a cold
 * row, one with no kept feature node, has no candidates.  OCFFM_E_STATE
 * before ocffm_model_set_items; OCFFM_E_ARG for a NULL pop with npop > 0. */
int ocffm_model_set_popularity(ocffm_model *m, const double *pop, uint64_t npop);

/* Serving: the signatures, order, exclusion, short-row, duplicate and
 * reproducibility rules (OCFFM_REC_ROWS, OCFFM_REC_SLICES, OCFFM_REC_SEG, read
 * when the model is created) and the error codes of the ocffm_problem_ entry
 * of the same name, on the model's catalogue: n is its item count, npop the
 * popularity entries, X rows in the model's user field space (read with the
 * first fu values of ocffm_model_get_ds).  OCFFM_E_STATE before
 * ocffm_model_set_items (a model from a problem has a catalogue).  The query
 * rows are projected by one launch per call (the kernel family of
 * ocffm_model_set_items).  Counters (ocffm_model_counter; an unknown name reads
 * 0): "rec_setup_us" / "eval_setup_us", the last call's host set-up as for the
 * problem; "project_us", the last ocffm_model_set_items' projection;
 * "rank_kernel_us", the last call's serving launches between HIP events. */
int ocffm_model_recommend(ocffm_model *m, const ocffm_data *X, uint64_t row0, uint64_t rows, uint32_t topn,
                          uint32_t flags, uint32_t *items, double *scores);
int ocffm_model_score(ocffm_model *m, const ocffm_data *X, uint64_t npairs, const uint32_t *prow,
                      const uint32_t *pitem, double *out);
int ocffm_model_recommend_among(ocffm_model *m, const ocffm_data *X, uint64_t row0, uint64_t rows,
                                const uint64_t *cptr, const uint32_t *ccol, uint32_t topn, uint32_t flags,
                                uint32_t *items, double *scores);
int ocffm_model_label_ranks(ocffm_model *m, const ocffm_data *X, const ocffm_data *seen, uint32_t *ranks,
                            double *scores, uint32_t *ncand);
int ocffm_model_label_ranks_among(ocffm_model *m, const ocffm_data *X, const ocffm_data *seen, const uint64_t *cptr,
                                  const uint32_t *ccol, uint32_t *ranks, double *scores, uint32_t *ncand);
int ocffm_model_evaluate(ocffm_model *m, const ocffm_data *X, const ocffm_data *seen, const uint32_t *cuts,
                         uint32_t ncut, ocffm_eval *out);
int ocffm_model_evaluate_among(ocffm_model *m, const ocffm_data *X, const ocffm_data *seen, const uint64_t *cptr,
                               const uint32_t *ccol, const uint32_t *cuts, uint32_t ncut, ocffm_eval *out);
int ocffm_model_counter(ocffm_model *m, const char *name, int64_t *value);

/* Folding new users in from an interaction history, on a model: the fold
 * entries (fold_in and the _fold forms of recommend, label_ranks and evaluate)
 * are declared in ocffm_fold.h, included at the end of this header. */

/* Items like this one: cosine / inner-product top-N between catalogue items,
 * pair similarities, and queries by item rows that are not in the catalogue
 * are declared in ocffm_similar.h, included at the end of this header. */

/* Diversified top-N (greedy MMR re-ranking of a row's pool by those
 * similarities) is declared in ocffm_diverse.h, included after it. */

/* Access.  ocffm_model_get_info fills Ds / used when the caller gave room;
 * ocffm_model_get_ds writes the f field sizes (user fields first).
 * ocffm_model_get copies to the host as fp64 like ocffm_problem_get: what 'W',
 * 'H' (block b12), 'Q' (the catalogue's cross table of cross block b12,
 * n x k), 'b' (b_j, n values). */
int ocffm_model_get_info(ocffm_model *m, ocffm_model_info *out);
int ocffm_model_get_ds(ocffm_model *m, uint64_t *out);
int ocffm_model_get(ocffm_model *m, char what, uint32_t b12, double *out, uint64_t cap, uint64_t *len);
void ocffm_model_destroy(ocffm_model *m);

#ifdef __cplusplus
}
#endif

#include "ocffm_fold.h"
#include "ocffm_similar.h"
#include "ocffm_diverse.h"

#endif /* OCFFM_H */
