/* vus_marginals.h -- marginal covariances of the bundle adjustment (part of the C ABI of include/vus.h, which includes
 * this file; it can also be included on its own).  What gtsam.Marginals(graph, values).marginalCovariance(key) computes,
 * from the reduced camera system S = L L^T that vus_ba_schur (at lambda = 0) and the one-sided band solve leave behind.
 * All pointers are device pointers, every call is asynchronous on `stream`, allocates nothing and returns 0 or a negative
 * VUS_E_* code, as in vus.h.  The arguments are checked on the host before anything is launched.
 *
 * Sigma = S^-1 is delivered in S's own band storage [n_nodes, band + 1, 36]: entry (i, s) is the full 6 x 6 block
 * Sigma(i, i - s), row-major; the slots left of column 0 (i < s) are zero.  The band of Sigma is all any marginal of the
 * graph needs: a landmark's observing poses lie within the band of each other, and the shared-bias border of inertial
 * graphs adds a rank-6 correction.
 */
#ifndef VUS_MARGINALS_H
#define VUS_MARGINALS_H
#include "vus.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Block-band selected inversion.  L: the factor vus_ba_band_solve / vus_ba_band_solve_multi leave in Sband (the
 * ONE-SIDED solves: the split solves leave Sband unspecified), in the solver's layout -- blocks left of the 8-node diagonal
 * panels hold their transposes, and for bands of 7 nodes and more the diagonal panels hold the inverse of their 48 x 48
 * factor block; every band mode of the factorisation leaves that layout.  L is not modified.  Bottom-up over the panels P
 * with the rows R (the band nodes) below them, X = L_RP L_PP^-1:
 *     Sigma_RP = -Sigma_RR X                      (v_mfma_f64_16x16x4_f64; Sigma_RR is always inside the band)
 *     Sigma_PP = L_PP^-T L_PP^-1 - X^T Sigma_RP
 * Sigma_RP reaches band + 7 nodes from the diagonal: it is kept in `work`, only its part inside the band is stored.
 * Three launches per panel; no launch depends on its workgroups being resident together.
 * work: vus_ba_band_selinv_work_doubles(n_nodes, band) doubles (0 for invalid sizes). */
long long vus_ba_band_selinv_work_doubles(int n_nodes, int band);
int vus_ba_band_selinv(const double* L, int n_nodes, int band, double* Sigma, double* work, long long work_doubles,
                       void* stream);

/* Positive-definiteness of the landmark information V [n_points, 6] (upper triangle, as vus_ba_linearize writes it) before
 * it is inverted at lambda = 0: first_bad[0] = the smallest landmark whose 3 x 3 block has a leading minor <= 1e-13 of its
 * scale (a landmark whose every observation fails cheirality has V = 0), 0x7F7F7F7F if there is none. */
int vus_ba_point_check(const double* V, int n_points, int* first_bad, void* stream);

/* Landmark covariances  cov[j] = Vinv_j + sum_{(i, k) observing j} Y_ij^T Sigma(i, k) Y_kj,  Y = W Vinv (lambda = 0):
 * cov [n_points, 9] (3 x 3 row-major, world frame).  W, Vinv as vus_ba_linearize / vus_ba_schur at lambda = 0 left them;
 * Sigma from vus_ba_band_selinv (band_nodes as for vus_ba_schur).  The sum is walked along the tile pairs of T, the
 * schedule of the Schur kernel transposed: each pair's 8 x 8 pose blocks of Sigma are read once, then every landmark of
 * the pair adds its terms with f64 atomics (two runs agree to ~1e-15 relative, not bitwise).  Every landmark is computed
 * (2.9 ms at 50 k landmarks / 2 M observations); there is no index list of a subset. */
int vus_ba_point_covariance(const vus_ba_problem* P, const vus_ba_tiles* T, const double* W, const double* Vinv,
                            const double* Sigma, int band_nodes, double* cov, void* stream);

/* Bias border of graphs with inertial factors, after vus_nav_assemble(lambda = 0) and vus_ba_band_solve_multi(rhs, 7):
 * U = rhs[1..6] = A^-1 Scb, Sc = Sbb - Scb^T U,
 *   Sigma_bb [36] = Sc^-1,  Sigma_nb [n_nodes, 36] = -U Sc^-1 (node rows x bias columns),
 *   Sigma (the band from vus_ba_band_selinv of A) += U_i Sc^-1 U_k^T on every stored block.
 * ok[0] = 1.0, or 0.0 when Sc is not positive definite -- a Cholesky pivot of its symmetric part <= 1e-13 of its largest
 * diagonal entry, the criterion of vus_ba_point_check (Sigma_bb and the update are then meaningless). */
int vus_nav_border_covariance(int n_nodes, int band, const double* rhs, const double* Scb, const double* Sbb, double* Sigma,
                              double* Sigma_nb, double* Sigma_bb, double* ok, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VUS_MARGINALS_H */
