/* vus_closure.h -- long loop closures as a low-rank correction of the band solve (part of the C ABI of include/vus.h,
 * which includes this file; it can also be included on its own).  A between factor whose two nodes lie further apart than
 * the band adds U U^T to the reduced camera system, U being 6 columns with two non-zero row blocks.  With the band system
 * B = L L^T factored as it is today,
 *     Z = B^-1 U,   C = I + U^T Z,   x = x0 - Z C^-1 (U^T x0)
 * solves (B + U U^T) x = b exactly from the band solution x0 = B^-1 b: the band need not widen to hold the closure.
 * The hot step is Z: the substitution of up to 6 * 64 further right-hand sides against the factor the band solve has left
 * behind (vus_ba_band_resolve); the rest are small kernels over the long factors.  A trial runs
 *     vus_closure_linearize (once per linearisation), vus_ba_schur, vus_closure_gradient, the one-sided band solve,
 *     vus_closure_scatter, vus_ba_band_resolve, vus_closure_capacitance, vus_closure_diag_max, vus_closure_correct.
 * All pointers are device pointers, every call is asynchronous on `stream`, allocates nothing and returns 0 or a negative
 * VUS_E_* code, as in vus.h.  The arguments are checked on the host before anything is launched.
 */
#ifndef VUS_CLOSURE_H
#define VUS_CLOSURE_H
#include "vus.h"
#include "vus_between.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VUS_CLOSURE_MAX_COLS 384 /* 64 closures of 6 columns */

/* X <- B^-1 X against the stored factor.  L: what vus_ba_band_solve / vus_ba_band_solve_multi leave in Sband (the
 * ONE-SIDED solves), in the layout vus_marginals.h describes; every band mode leaves that layout.  L is not modified.
 * X [n_cols, 6 * n_nodes]: one right-hand side per row, as in vus_ba_band_solve_multi, solved in place, no sign change;
 * 1 <= n_cols <= VUS_CLOSURE_MAX_COLS.  X must not overlap L.
 * One workgroup owns 16 columns and walks the forward sweep over all panels and then the backward sweep on its own: no
 * workgroup waits for another, no flags, no atomics; two calls on the same L and X give the same bits.  A panel step is
 * a 48 x (6 band) by (6 band) x 16 product on v_mfma_f64_16x16x4_f64 and the panel's 48 x 48 inverse applied as a product
 * (bands under 7 nodes keep the factor in the diagonal panels: those substitute).
 * work / work_doubles: scratch for the call.  This implementation needs none (work may be NULL with work_doubles 0); a
 * negative work_doubles, or a NULL work with a positive one, is refused. */
int vus_ba_band_resolve(const double* L, int n_nodes, int band, double* X, int n_cols, double* work,
                        long long work_doubles, void* stream);

/* ---- the long set: k <= VUS_CLOSURE_MAX between factors whose nodes lie MORE than the band apart -----------------------
 * A vus_between_factors (include/vus_between.h) holds them; its target CSR is used by vus_between_eval_step /
 * vus_between_error only, which serve the long set unchanged (they check sizes and pointers only).  The arithmetic of a
 * factor -- residual, H1 = -Ad(hx^-1), H2 = I, whitening, Block reweighting -- is that of the in-band path.  fp64, fixed
 * summation orders, no atomics: two runs give the same bits.  No stage reads anything back to the host. */
#define VUS_CLOSURE_MAX 64
#define VUS_CLOSURE_ROW 78 /* doubles per factor in `rows` */
#define VUS_CLOSURE_MAX_RHS 8

/* Host-side validation, once per factor set (reads the index arrays back): 1 <= n <= VUS_CLOSURE_MAX, every node a pose
 * node in [0, n_nodes), every loss known, and |node1 - node2| > band for every factor: one inside the band belongs to
 * vus_between_assemble; with `sqrt_info` (full-covariance models, include/vus_between.h), its entries as vus_between_check
 * checks them. */
int vus_closure_check(const vus_between_factors* B, int band, void* stream);
long long vus_closure_work_doubles(const vus_between_factors* B);

/* rows [n, 78] at `poses` [n_poses, 12]: J1 (36, row-major: residual row x tangent column of node1), J2 (36), r (6), whitened
 * and scaled by sqrt(w(|W r|)) -- W = diag(1/sigma), or the factor's R under sqrt_info: J2 is then sqrt(w) R, upper-triangular,
 * all 36 entries written;  err[0] = 0.5 sum |r|^2, the linear error at delta = 0.  work: vus_closure_work_doubles. */
int vus_closure_linearize(const vus_between_factors* B, const double* poses, double* rows, double* err, double* work,
                          void* stream);

/* gs [n_nodes, 6] += J1^T r at node1 and J2^T r at node2 of every factor, in factor order.  Call where
 * vus_between_assemble stands: after vus_ba_schur, before vus_nav_assemble / vus_navb_assemble. */
int vus_closure_gradient(const vus_between_factors* B, const double* rows, double* gs, void* stream);

/* U [6 n, 6 n_nodes] (the layout of X above): row 6 f + q = row q of [J1 J2] of factor f at the columns of its two nodes,
 * zero elsewhere (the whole buffer is written). */
int vus_closure_scatter(const vus_between_factors* B, const double* rows, double* U, void* stream);

/* C [6 n, 6 n] = I + U^T Z from rows and Z = vus_ba_band_resolve(U) (each entry a 12-term dot product), then its Cholesky
 * factor in place (lower triangle, row-major; the strict upper triangle keeps I + U^T Z), by one workgroup. */
int vus_closure_capacitance(const vus_between_factors* B, const double* rows, const double* Z, double* C, void* stream);

/* X [n_rhs, 6 n_nodes] <- X - Z C^-1 (U^T X), row by row, in place: solutions of the band system become solutions of
 * the system with the long closures.  1 <= n_rhs <= VUS_CLOSURE_MAX_RHS.  work: vus_closure_work_doubles. */
int vus_closure_correct(const vus_between_factors* B, const double* rows, const double* Z, const double* C, double* X,
                        int n_rhs, double* work, void* stream);

/* out[0] = max_i C_ii = max_i sum_{c <= i} L_ic^2 from the factor vus_closure_capacitance has left in C: 1 + the largest
 * weight of a closure row against the band system.  The correction cancels x0 = B^-1 b down to x by about that factor,
 * so the low-rank path loses that many digits more than a band widened to the closure would (profiles/closure_conditioning.md);
 * the caller decides what is too large.  NaN if any L_ic^2 on or below the diagonal is NaN.  One workgroup, no read-back. */
int vus_closure_diag_max(const vus_between_factors* B, const double* C, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VUS_CLOSURE_H */
