/* ocffm_similar.h — items like this one: cosine / inner-product top-N between
 * catalogue items on an ocffm_model.  Included by ocffm.h (after the
 * saved-models section, whose types it uses); do not include it alone. */
#ifndef OCFFM_SIMILAR_H
#define OCFFM_SIMILAR_H

#ifdef __cplusplus
extern "C" {
#endif

/* Similar items (no reference counterpart).  The catalogue's item-side cross
 * tables are an item's whole interaction with any user: score(i, j) - a_i - b_j
 * = <p_i, e_j>.  On a model with a catalogue of n items, C = fu fv cross
 * tables and depth C kp (entries past k are zero):
 *   embedding   e_j is the concatenation over c < C of Q_c[j][0..kp).
 *   chain       acc(x, y) is the serving sweep's own chain: chunks of 16 depth
 *               elements in order on v_mfma_{f32,f64}_16x16x4, as in
 *               ocffm_problem_recommend.  The operands commute within each MFMA
 *               and the chain order is fixed: acc(x, y) and acc(y, x) have the
 *               same bits.
 *   norms       nn_j = <e_j, e_j> is summed in fp64 from the widened table
 *               values in one fixed association (16 lane
 *               chains s = fma(x, x, s) over the depth elements 64 t + 4 l ..
 *               + 3 of lane l in depth order, then a fixed butterfly over the
 *               lanes); no floating-point atomics.  inv_j = 1 / sqrt(nn_j) in
 *               fp64, rounded once to the model's precision; inv_j = 0 where
 *               nn_j == 0.
 *   similarity  cosine (default): sim = acc (inv_x inv_y) in the model's
 *               precision; the product of the two inverse norms comes first,
 *               so sim is symmetric bit for bit.  OCFFM_SIM_DOT: sim = acc.
 *               The cosine with a zero vector is 0, and such an item stays a
 *               candidate.  a, b, the popularity and cold rows play no part:
 *               no row is cold.
 *   values      are returned as fp64 (exact for either precision).
 *   order       recommend's strict total order: similarity descending, equal
 *               values by ascending item index.  A row's result therefore does
 *               not depend on its place in the call, on OCFFM_REC_ROWS, on
 *               OCFFM_REC_SLICES or on the other queries.
 *   exclusions  a query given by its catalogue index q leaves q itself out
 *               unless OCFFM_SIM_KEEP_SELF is set.  Optional per-query lists
 *               (xptr: nq + 1 non-decreasing offsets from 0 into xcol, the
 *               shape of the _among lists; both NULL: none) are united with
 *               it; entries >= n are ignored and repeats count once.
 *   short rows  slots without a candidate hold OCFFM_REC_NONE and -inf.
 *
 * ocffm_model_similar_items: the queries are the catalogue items qitem[0..nq),
 * in any order, repeats allowed; items / scores are nq x topn, row-major
 * (scores may be NULL).
 * ocffm_model_similar_to: the queries are rows [row0, row0 + rows) of Vq, item
 * rows in the model's item field space (read with the model's item Ds, as for
 * set_items), e.g. an item that is not in the catalogue; they are projected
 * as the catalogue is and their norms are summed by the catalogue's kernel, so
 * a copy of catalogue row q gives similar_items' bits for q with
 * OCFFM_SIM_KEEP_SELF.  Nothing is excluded but the lists.
 * ocffm_model_item_similarity: sim of the catalogue pairs (pa[e], pb[e]), the
 * value the two entries above return for that pair, bit for bit; -inf when
 * either index is >= n.
 * Errors: OCFFM_E_STATE before ocffm_model_set_items; OCFFM_E_ARG for topn ==
 * 0 or > OCFFM_REC_MAX_TOPN, NULL items, NULL qitem, pa, pb or out with a
 * non-zero count, qitem[e] >= n, row0 + rows > Vq.m, a Vq with more fields
 * than fv, unknown flag bits, an xcol without xptr, an xptr that does not
 * start at 0 or decreases, or has entries without xcol; OCFFM_E_DATA for a
 * node of Vq with idx >= Ds[fid].  Zero queries or pairs return OCFFM_OK; an
 * empty catalogue gives rows of OCFFM_REC_NONE / -inf.
 * Counters (ocffm_model_counter): "sim_norm_builds", builds of the
 * catalogue's inverse norms since the model was created (they are built on
 * the first similarity call after a catalogue is set, kept with the model and
 * dropped by set_items); "sim_norm_us", the last build; "sim_setup_us", the
 * last call's host set-up; "rank_kernel_us", the last call's launches between
 * HIP events; "sim_gather_us", the share of similar_items' query gathers. */
#define OCFFM_SIM_DOT 1u       /* flags: inner product instead of cosine */
#define OCFFM_SIM_KEEP_SELF 2u /* flags: a query item stays among its own candidates */

int ocffm_model_similar_items(ocffm_model *m, uint64_t nq, const uint32_t *qitem, const uint64_t *xptr,
                              const uint32_t *xcol, uint32_t topn, uint32_t flags, uint32_t *items, double *scores);
int ocffm_model_similar_to(ocffm_model *m, const ocffm_data *Vq, uint64_t row0, uint64_t rows, const uint64_t *xptr,
                           const uint32_t *xcol, uint32_t topn, uint32_t flags, uint32_t *items, double *scores);
int ocffm_model_item_similarity(ocffm_model *m, uint64_t npairs, const uint32_t *pa, const uint32_t *pb,
                                uint32_t flags, double *out);

#ifdef __cplusplus
}
#endif

#endif /* OCFFM_SIMILAR_H */
