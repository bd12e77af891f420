// between.hip -- BetweenFactor<Pose3> kernels for gfx950 (MI355X), fp64 (include/vus_between.h).
//
// Odometry and loop-closure factors between two keyframe poses.  Their blocks are added into the reduced camera system
// after the landmark Schur step, so the band solve, back-substitution and retraction are those of band_solve.hip and ba.hip unchanged.
//   linearize   thread / factor   hx = T1^-1 T2, r = Log(meas^-1 hx), H1 = -Ad(hx^-1), H2 = I, whitened and reweighted:
//                                 the five products of the factor to `lin`, its error to a partial
//   assemble    thread / element of a target block: the fixed-order sum over the block's CSR list, added to Sband (and gs)
//   eval        thread / factor   linearised error at the step (old poses) and error at the new poses
// Errors are summed by the fixed-order reduce of vus_common.hip (vus::reduce_partials).
// Shared with the other pose kernels (se3_device.h): pose_local, load12, the robust-loss table and its per-factor dispatcher;
// with closure.hip (between_device.h): the factor's residual and H1, and the whitening of a full-covariance model
// (vus_between_factors.sqrt_info: the kernels that whiten are templates on the model form, picked on the host);
// with the other add-on families (factor_common.h): read_back and the per-factor loss check.
#include <cmath>
#include <vector>
#include "vus_common.h"
#include "se3_device.h"
#include "between_device.h"
#include "factor_common.h"

namespace {

constexpr int LIN = 120;      // per factor: J1^T J1, J1^T J2, J2^T J2 (36 each), J1^T r, J2^T r (6 each)

// FULL: the factors carry a full-covariance model (B.sqrt_info); the diagonal instantiation is the kernel as it was.
template <bool FULL>
__global__ __launch_bounds__(256) void between_linearize_kernel(vus_between_factors B, const double* __restrict__ poses,
                                                                double* __restrict__ lin, double* __restrict__ err_part) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= B.n) return;
  BetweenLin L;
  between_factor<true>(B, poses, f, L);
  if constexpr (FULL) {
    // the rows of the long path (closure.hip): A = s R H1, Rs = s R, b = s R r with s = sqrt(w(|R r|)); then
    // J1^T J1 = A^T A,  J1^T J2 = A^T Rs,  J2^T J2 = Rs^T Rs,  J1^T b = A^T b,  J2^T b = Rs^T b  (= H1^T M H1, H1^T M, M,
    // H1^T M r, M r with the information M = w R^T R); every sum runs over the residual rows in ascending order
    SqrtInfo S;
    load_sqrt_info(B, f, S);
    double b[6], A[36], rw, rho;
    whiten6(S, 1.0, L.r, b);
    const double d2 = norm_sq6(b);
    robust_weight_of(B.loss_kind, B.loss_k, f, d2, rw, rho);
    const double sw = sqrt(rw);
    whiten66(S, sw, L.H1, A);
#pragma unroll
    for (int k = 0; k < 6; ++k) b[k] *= sw;
#pragma unroll
    for (int k = 0; k < 21; ++k) S.R[k] *= sw;
    double* o = lin + LIN * (size_t)f;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        double s11 = 0, s12 = 0, s22 = 0;
#pragma unroll
        for (int k = 0; k < 6; ++k) s11 += A[6 * k + a] * A[6 * k + c];
#pragma unroll
        for (int k = 0; k <= c; ++k) s12 += A[6 * k + a] * S.R[SqrtInfo::at(k, c)];
#pragma unroll
        for (int k = 0; k <= (a < c ? a : c); ++k) s22 += S.R[SqrtInfo::at(k, a)] * S.R[SqrtInfo::at(k, c)];
        o[6 * a + c] = s11;
        o[36 + 6 * a + c] = s12;
        o[72 + 6 * a + c] = s22;
      }
      double g1 = 0, g2 = 0;
#pragma unroll
      for (int k = 0; k < 6; ++k) g1 += A[6 * k + a] * b[k];
#pragma unroll
      for (int k = 0; k <= a; ++k) g2 += S.R[SqrtInfo::at(k, a)] * b[k];
      o[108 + a] = g1;
      o[114 + a] = g2;
    }
    err_part[f] = 0.5 * rw * d2;
    return;
  }
  double w[6], w2[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) w[k] = B.w[6 * (size_t)f + k];
  double rw, rho;
  const double d2 = whitened_sq(w, L.r);
  robust_weight_of(B.loss_kind, B.loss_k, f, d2, rw, rho);
#pragma unroll
  for (int k = 0; k < 6; ++k) w2[k] = rw * w[k] * w[k];     // the weighted information of each residual row
  double* o = lin + LIN * (size_t)f;
  // J1^T J1 = H1^T diag(w2) H1,  J1^T J2 = H1^T diag(w2),  J2^T J2 = diag(w2),  J1^T b = H1^T (w2 r),  J2^T b = w2 r
#pragma unroll
  for (int a = 0; a < 6; ++a) {
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      double s = 0;
#pragma unroll
      for (int k = 0; k < 6; ++k) s += L.H1[6 * k + a] * w2[k] * L.H1[6 * k + c];
      o[6 * a + c] = s;
      o[36 + 6 * a + c] = L.H1[6 * c + a] * w2[c];
      o[72 + 6 * a + c] = a == c ? w2[a] : 0.0;
    }
    double g = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) g += L.H1[6 * k + a] * w2[k] * L.r[k];
    o[108 + a] = g;
    o[114 + a] = w2[a] * L.r[a];
  }
  err_part[f] = 0.5 * rw * d2;
}

__global__ __launch_bounds__(256) void between_assemble_kernel(vus_between_factors B, const double* __restrict__ lin, int band,
                                                               double* __restrict__ Sband, double* __restrict__ gs) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 36 * B.n_targets) return;
  const int q = t / 36, e = t - 36 * q;
  const int node = B.tgt_node[q], s = B.tgt_s[q];
  if ((unsigned)node >= (unsigned)B.n_nodes || s < 0 || s > band || s > node) return;   // vus_between_check refuses these
  const int d1 = e / 6, d2 = e - 6 * d1;
  double h = 0, g = 0;
  for (int p = B.tgt_ptr[q]; p < B.tgt_ptr[q + 1]; ++p) {
    const int term = B.tgt_terms[p];
    const double* o = lin + LIN * (size_t)(term >> 2);
    switch (term & 3) {
      case 0: h += o[e]; g += o[108 + d2]; break;
      case 1: h += o[72 + e]; g += o[114 + d2]; break;
      case 2: h += o[36 + e]; break;
      default: h += o[36 + 6 * d2 + d1]; break;
    }
  }
  Sband[36 * ((size_t)node * (band + 1) + s) + e] += h;
  if (s == 0 && d1 == 0) gs[6 * (size_t)node + d2] += g;
}

// part_lin[f] = 0.5 w |b + J1 d1 + J2 d2|^2 at the old poses, part_new[f] = rho at the new poses
template <bool FULL>
__global__ __launch_bounds__(256) void between_eval_kernel(vus_between_factors B, const double* __restrict__ poses,
                                                           const double* __restrict__ dp, const double* __restrict__ new_poses,
                                                           double* __restrict__ part_lin, double* __restrict__ part_new) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= B.n) return;
  if constexpr (FULL) {
    BetweenLin L;
    SqrtInfo S;
    double b[6], rw, rho;
    if (part_lin != nullptr) {
      between_factor<true>(B, poses, f, L);
      const double* d1 = dp + 6 * (size_t)B.node1[f];
      const double* d2 = dp + 6 * (size_t)B.node2[f];
      double v[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        v[k] = L.r[k] + d2[k];
#pragma unroll
        for (int c = 0; c < 6; ++c) v[k] += L.H1[6 * k + c] * d1[c];
      }
      load_sqrt_info(B, f, S);
      whiten6(S, 1.0, L.r, b);
      robust_weight_of(B.loss_kind, B.loss_k, f, norm_sq6(b), rw, rho);
      whiten6(S, 1.0, v, b);
      part_lin[f] = 0.5 * rw * norm_sq6(b);
    }
    between_factor<false>(B, new_poses, f, L);
    load_sqrt_info(B, f, S);
    whiten6(S, 1.0, L.r, b);
    robust_weight_of(B.loss_kind, B.loss_k, f, norm_sq6(b), rw, rho);
    part_new[f] = rho;
    return;
  }
  double w[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) w[k] = B.w[6 * (size_t)f + k];
  BetweenLin L;
  double rw, rho;
  if (part_lin != nullptr) {
    between_factor<true>(B, poses, f, L);
    robust_weight_of(B.loss_kind, B.loss_k, f, whitened_sq(w, L.r), rw, rho);
    const double* d1 = dp + 6 * (size_t)B.node1[f];
    const double* d2 = dp + 6 * (size_t)B.node2[f];
    double e = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      double v = L.r[k] + d2[k];
#pragma unroll
      for (int c = 0; c < 6; ++c) v += L.H1[6 * k + c] * d1[c];
      e += (w[k] * v) * (w[k] * v);
    }
    part_lin[f] = 0.5 * rw * e;
  }
  between_factor<false>(B, new_poses, f, L);
  robust_weight_of(B.loss_kind, B.loss_k, f, whitened_sq(w, L.r), rw, rho);
  part_new[f] = rho;
}

int check_args(const vus_between_factors* B) {
  VUS_REQUIRE(B != nullptr, "between factors are null");
  VUS_REQUIRE(B->n >= 1 && B->n_nodes >= 2 && B->pose_stride >= 1 && B->pose_stride <= 3 && B->n_nodes % B->pose_stride == 0,
              "bad sizes: n=%d n_nodes=%d pose_stride=%d", B->n, B->n_nodes, B->pose_stride);
  VUS_REQUIRE(B->node1 && B->node2 && B->meas && (B->w || B->sqrt_info) && B->loss_kind && B->loss_k, "factor arrays are null");
  VUS_REQUIRE(B->n_targets >= 1 && B->tgt_node && B->tgt_s && B->tgt_ptr && B->tgt_terms, "target arrays are null");
  return VUS_OK;
}

}  // namespace

extern "C" long long vus_between_work_doubles(const vus_between_factors* B) {
  if (!B || B->n < 0) return 0;
  return 2ll * B->n + 8;
}

extern "C" int vus_between_check(const vus_between_factors* B, int band, void* stream) {
  if (int rc = check_args(B)) return rc;
  VUS_REQUIRE(band >= 1 && band < B->n_nodes, "band=%d for %d nodes", band, B->n_nodes);
  hipStream_t st = vus::as_stream(stream);
  std::vector<int> n1, n2, tn, ts, tp, terms, kind;
  std::vector<double> lk;
  if (int rc = read_back(B->node1, B->n, n1, st)) return rc;
  if (int rc = read_back(B->node2, B->n, n2, st)) return rc;
  if (int rc = read_back(B->loss_kind, B->n, kind, st)) return rc;
  if (int rc = read_back(B->loss_k, B->n, lk, st)) return rc;
  if (int rc = read_back(B->tgt_node, B->n_targets, tn, st)) return rc;
  if (int rc = read_back(B->tgt_s, B->n_targets, ts, st)) return rc;
  if (int rc = read_back(B->tgt_ptr, (size_t)B->n_targets + 1, tp, st)) return rc;
  VUS_REQUIRE(tp[0] == 0, "tgt_ptr[0]=%d", tp[0]);
  for (int q = 0; q < B->n_targets; ++q) VUS_REQUIRE(tp[q + 1] >= tp[q], "tgt_ptr decreases at %d", q);
  if (int rc = read_back(B->tgt_terms, (size_t)tp[B->n_targets], terms, st)) return rc;
  const int ps = B->pose_stride;
  for (int f = 0; f < B->n; ++f) {
    VUS_REQUIRE(n1[f] >= 0 && n1[f] < B->n_nodes && n2[f] >= 0 && n2[f] < B->n_nodes && n1[f] % ps == 0 && n2[f] % ps == 0,
                "factor %d: nodes (%d, %d) are not pose nodes of %d nodes at pose_stride %d", f, n1[f], n2[f], B->n_nodes, ps);
    VUS_REQUIRE(n1[f] != n2[f], "factor %d joins node %d to itself", f, n1[f]);
    VUS_REQUIRE(std::abs(n1[f] - n2[f]) <= band, "factor %d: nodes %d and %d are more than band=%d apart", f, n1[f], n2[f], band);
    if (int rc = check_factor_loss(f, kind[f], lk[f])) return rc;
  }
  if (int rc = check_sqrt_info(B->sqrt_info, B->n, st)) return rc;
  for (int q = 0; q < B->n_targets; ++q) {
    const int node = tn[q], s = ts[q];
    VUS_REQUIRE(node >= 0 && node < B->n_nodes && s >= 0 && s <= band && s <= node, "target %d: block (%d, s=%d) outside the band",
                q, node, s);
    for (int p = tp[q]; p < tp[q + 1]; ++p) {
      const int f = terms[p] >> 2, kind = terms[p] & 3;
      VUS_REQUIRE(terms[p] >= 0 && f < B->n, "target %d: term %d out of range", q, terms[p]);
      const bool ok = kind == 0 ? (node == n1[f] && s == 0)
                    : kind == 1 ? (node == n2[f] && s == 0)
                    : kind == 2 ? (node == n1[f] && s == n1[f] - n2[f])
                                : (node == n2[f] && s == n2[f] - n1[f]);
      VUS_REQUIRE(ok, "target %d (node %d, s=%d): term %d of factor %d does not land in it", q, node, s, kind, f);
    }
  }
  return VUS_OK;
}

extern "C" int vus_between_linearize(const vus_between_factors* B, const double* poses, double* lin, double* err,
                                     double* work, void* stream) {
  if (int rc = check_args(B)) return rc;
  VUS_REQUIRE(poses && lin && err && work, "null buffer");
  hipStream_t st = vus::as_stream(stream);
  if (B->sqrt_info) between_linearize_kernel<true><<<cdiv(B->n, 256), 256, 0, st>>>(*B, poses, lin, work);
  else between_linearize_kernel<false><<<cdiv(B->n, 256), 256, 0, st>>>(*B, poses, lin, work);
  vus::reduce_partials(work, B->n, err, st);
  VUS_CHECK_LAUNCH("between_linearize");
  return VUS_OK;
}

extern "C" int vus_between_assemble(const vus_between_factors* B, const double* lin, int band, double* Sband, double* gs,
                                    void* stream) {
  if (int rc = check_args(B)) return rc;
  VUS_REQUIRE(lin && Sband && gs, "null buffer");
  VUS_REQUIRE(band >= 1 && band < B->n_nodes, "band=%d for %d nodes", band, B->n_nodes);
  between_assemble_kernel<<<cdiv(36ll * B->n_targets, 256), 256, 0, vus::as_stream(stream)>>>(*B, lin, band, Sband, gs);
  VUS_CHECK_LAUNCH("between_assemble");
  return VUS_OK;
}

extern "C" int vus_between_eval_step(const vus_between_factors* B, const double* poses, const double* dp,
                                     const double* new_poses, double* out, double* work, void* stream) {
  if (int rc = check_args(B)) return rc;
  VUS_REQUIRE(poses && dp && new_poses && out && work, "null buffer");
  hipStream_t st = vus::as_stream(stream);
  double* part_lin = work;
  double* part_new = work + B->n;
  if (B->sqrt_info) between_eval_kernel<true><<<cdiv(B->n, 256), 256, 0, st>>>(*B, poses, dp, new_poses, part_lin, part_new);
  else between_eval_kernel<false><<<cdiv(B->n, 256), 256, 0, st>>>(*B, poses, dp, new_poses, part_lin, part_new);
  vus::reduce_partials(part_lin, B->n, out, st);
  vus::reduce_partials(part_new, B->n, out + 1, st);
  VUS_CHECK_LAUNCH("between_eval_step");
  return VUS_OK;
}

extern "C" int vus_between_error(const vus_between_factors* B, const double* poses, double* err, double* work, void* stream) {
  if (int rc = check_args(B)) return rc;
  VUS_REQUIRE(poses && err && work, "null buffer");
  hipStream_t st = vus::as_stream(stream);
  if (B->sqrt_info) between_eval_kernel<true><<<cdiv(B->n, 256), 256, 0, st>>>(*B, poses, nullptr, poses, nullptr, work + B->n);
  else between_eval_kernel<false><<<cdiv(B->n, 256), 256, 0, st>>>(*B, poses, nullptr, poses, nullptr, work + B->n);
  vus::reduce_partials(work + B->n, B->n, err, st);
  VUS_CHECK_LAUNCH("between_error");
  return VUS_OK;
}
