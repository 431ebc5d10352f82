/* ocffm_diverse.h — diversified top-N: greedy maximal-marginal-relevance (MMR)
 * re-ranking of a row's top-`pool` list on an ocffm_model.  Included by ocffm.h
 * (after ocffm_similar.h, whose similarity it uses); do not include it alone. */
#ifndef OCFFM_DIVERSE_H
#define OCFFM_DIVERSE_H

#ifdef __cplusplus
extern "C" {
#endif

/* Diversified recommendation (no reference counterpart).  A model that has
 * learnt an artist or a genre field fills the head of a top-N list with near
 * duplicates; this entry re-ranks a row's pool on the device, trading model
 * score against the cosine similarity (ocffm_similar.h) to what is already
 * taken.  No rows x n and no n x n array exists.
 *   pool        the row's top-`pool` list: with cptr == ccol == NULL exactly
 *               what ocffm_model_recommend(topn = pool, flags) returns for the
 *               row, otherwise what ocffm_model_recommend_among(..., topn =
 *               pool, flags) returns: items, scores, order, cold rows,
 *               OCFFM_REC_EXCLUDE_LABELS and short rows as in those calls.  c
 *               is the number of filled slots and s_0 >= ... >= s_{c-1} are
 *               the pool scores as fp64 (recommend's bits).
 *   relevance   in fp64: range = s_0 - s_{c-1}, rel_p = (s_p - s_{c-1}) /
 *               range, and rel_p = 0 for every p when range == 0.
 *   similarity  sim(p, t) is ocffm_model_item_similarity's cosine of the two
 *               pool items, bit for bit (the sweep's chain, then acc (inv_x
 *               inv_y) in the model's precision), widened to fp64.  An item
 *               with a zero norm has similarity 0 to everything.
 *   selection   step 0 takes pool position 0.  At step t >= 1 every position p
 *               not yet taken has ms_p, the maximum of sim(p, u) over the taken
 *               u (a true maximum: it may be negative), and v_p = w rel_p -
 *               theta ms_p with w = 1 - theta computed once on the host: two
 *               products and one difference, each rounded to fp64 on its own
 *               (nothing is contracted into an FMA; the division of rel is
 *               correctly rounded).  The position with the largest v is taken;
 *               equal v goes to the lower pool position.  Selection stops
 *               after min(topn, c) picks.
 *   outputs     rows x topn, row-major.  items: the taken items in the order
 *               they were taken; scores (may be NULL): their model scores,
 *               recommend's bits; mmr (may be NULL): v when taken (step 0:
 *               w rel_0); pos (may be NULL): the pool position.  Slots past
 *               the picks hold OCFFM_REC_NONE, -inf, -inf and OCFFM_REC_NONE.
 * Hence theta == 0 returns recommend(topn) / recommend_among(topn) bit for bit
 * for any pool >= topn, and a row's result does not depend on its place in the
 * call, on OCFFM_REC_ROWS, OCFFM_REC_SLICES, OCFFM_REC_SEG or the other rows.
 * Errors: those of ocffm_model_recommend / ocffm_model_recommend_among (topn
 * checked as there); OCFFM_E_ARG for pool < topn, pool > OCFFM_DIV_MAX_POOL,
 * theta outside [0, 1] or NaN, unknown flag bits, a ccol without cptr (and
 * what _among rejects of its lists); OCFFM_E_STATE before
 * ocffm_model_set_items.  rows == 0 returns OCFFM_OK; an empty catalogue gives
 * rows of OCFFM_REC_NONE / -inf.
 * Counters (ocffm_model_counter): "div_setup_us", the last call's host set-up;
 * "div_kernel_us", the share of the MMR launches between HIP events;
 * "rank_kernel_us", all of the call's launches; the inverse norms are those of
 * ocffm_similar.h ("sim_norm_builds", "sim_norm_us"). */
#define OCFFM_DIV_MAX_POOL OCFFM_REC_MAX_TOPN /* 128 */

int ocffm_model_recommend_diverse(ocffm_model *m, const ocffm_data *X, uint64_t row0, uint64_t rows,
                                  const uint64_t *cptr, const uint32_t *ccol, /* both NULL: the whole catalogue */
                                  uint32_t topn, uint32_t pool, double theta, uint32_t flags,
                                  uint32_t *items, double *scores, double *mmr, uint32_t *pos);

#ifdef __cplusplus
}
#endif

#endif /* OCFFM_DIVERSE_H */
