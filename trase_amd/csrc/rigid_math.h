// rigid_math.h -- the per-row algebra of the rigid-motion fit (neighbors.hip: polar3 / rigid_fit kernels): the rotation of one
// 3 x 3 moment matrix and its closed-form gradient.
//
//   polar3(S) -> R = V U^T  with S = U Sigma V^T: the orthogonal polar factor of S^T (S^T = R H, H = (S S^T)^(1/2) = U Sigma U^T).
//   det R = sign(det S): there is no determinant correction (utils/loss_utils.py:205-207 has none; a reflection stays one).
//
// Arithmetic: one-sided Jacobi (Hestenes) in float64.  B = S and V = I; a plane rotation of the columns p, q of B (and of V)
// makes b_p . b_q = 0; a pair counts as orthogonal when (b_p . b_q)^2 <= 2^-100 |b_p|^2 |b_q|^2, a RELATIVE test, so a small
// column stays orthogonal to a large one to 2^-50 of its own length.  At most RGD_SWEEPS sweeps of the three pairs: a fixed
// bound, whatever the input (a NaN compares false and rotates until the bound ends the loop).  Then S V = B = U Sigma with
// sigma_i = |b_i|; the columns are sorted by length (R = sum_i v_i u_i^T does not depend on their order) and
//     u_1 = b_1 / sigma_1,   u_2 = b_2 / sigma_2,   u_3 = +-(u_1 x u_2) / |u_1 x u_2|,  the sign that of b_3 . (u_1 x u_2),
// so the smallest singular value is never divided by.  b_3 . (u_1 x u_2) = det(B) / (sigma_1 sigma_2) has the sign of det S det V;
// where it is exactly 0 (rank 2) the sign is det V: det R = +1.  sigma_2 = 0 exactly, or b_2 a cancellation remainder parallel to
// b_1: u_2 is a unit vector orthogonal to u_1 (u_1 x the axis u_1 has least of), sigma_1 = 0: R = I.  A non-finite S gives R = NaN
// in every entry.  R is rounded to fp32 once.
//
//   polar3_bwd(S, R, G) -> gS for a cotangent G of R.  With dS^T = dR H + R dH and Omega = R^T dR = [w]_x skew, the skew part of
//   R^T dS^T is Omega H + H Omega = [(tr(H) I - H) w]_x, and <G, dR> = <R^T G, Omega> = b . w with [b]_x = R^T G - G^T R.  Hence
//       H = sym(R^T S^T),  b = (B_21, B_02, B_10),  y = (tr(H) I - H)^-1 b,  gS = (R [y]_x)^T.
//   tr(H) I - H has the eigenvalues sigma_j + sigma_k: no eigenvectors and no sigma_i - sigma_j.  The 3 x 3 solve is the adjugate
//   over the determinant, all in float64, gS rounded to fp32 once.
//
// Degenerate rows: sigma_2 + sigma_3 <= 4 (k + 2) 2^-24 m with m = sum over the row's edges of |e1| |e2| (for a matrix on its
// own: k = 1, m = |S|_F).  (k + 3) 2^-24 sum |e1_a| |e2_b| is the forward error of an entry of S (tests/neighbors_reference.py),
// at most (k + 3) 2^-24 m, and an error E moves a singular value by |E|_2 <= 3 max|E_ab|: the two small singular values of such a row
// lie below what S's own accumulation leaves of them, the rotation about u_1 is decided by rounding, and the row's gradient through
// R is defined as ZERO (the reference's SVD autograd gives Inf or NaN there).  R itself is the formula above in every case: it is a
// function of S alone, whatever k and m are.
//
// Pure scalar functions for HIP device code (the product) and, compiled with g++, for tests/test_rigid_reference.py.  Every body
// is compiled without floating-point contraction, so that a function gives the same bits in every kernel it is inlined into.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TRASE_RGD_HD __host__ __device__ __forceinline__
#else
#define TRASE_RGD_HD inline
#endif
#if defined(__clang__)
#define TRASE_RGD_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define TRASE_RGD_NO_CONTRACT
#endif

namespace trase {

constexpr int RGD_SWEEPS = 12;                              // a 3 x 3 float64 problem converges in 4 to 7
constexpr double RGD_ORTH2 = 7.888609052210118e-31;         // 2^-100: the square of the relative orthogonality 2^-50
constexpr double RGD_U = 5.9604644775390625e-08;            // 2^-24

struct RgdCol { double x, y, z; };

TRASE_RGD_HD double rgd_dot(const RgdCol& a, const RgdCol& b) {
  TRASE_RGD_NO_CONTRACT
  return a.x * b.x + a.y * b.y + a.z * b.z;
}
TRASE_RGD_HD RgdCol rgd_cross(const RgdCol& a, const RgdCol& b) {
  TRASE_RGD_NO_CONTRACT
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
TRASE_RGD_HD RgdCol rgd_scale(const RgdCol& a, double s) {
  TRASE_RGD_NO_CONTRACT
  return {a.x * s, a.y * s, a.z * s};
}
TRASE_RGD_HD void rgd_plane(RgdCol& p, RgdCol& q, double c, double s) {
  TRASE_RGD_NO_CONTRACT
  const RgdCol a = p, b = q;
  p = {c * a.x - s * b.x, c * a.y - s * b.y, c * a.z - s * b.z};
  q = {s * a.x + c * b.x, s * a.y + c * b.y, s * a.z + c * b.z};
}
TRASE_RGD_HD void rgd_swap(RgdCol& a, RgdCol& b) { const RgdCol t = a; a = b; b = t; }

// one Jacobi step on the columns p, q; false if they already count as orthogonal
TRASE_RGD_HD bool rgd_rotate(RgdCol& bp, RgdCol& bq, RgdCol& vp, RgdCol& vq) {
  TRASE_RGD_NO_CONTRACT
  const double alpha = rgd_dot(bp, bp), beta = rgd_dot(bq, bq), gamma = rgd_dot(bp, bq);
  if (gamma == 0.0 || gamma * gamma <= RGD_ORTH2 * alpha * beta) return false;
  const double zeta = (beta - alpha) / (2.0 * gamma);
  const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));     // the smaller root of t^2 + 2 zeta t - 1
  const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
  rgd_plane(bp, bq, c, s);
  rgd_plane(vp, vq, c, s);
  return true;
}

// |S|_F in float64 (+Inf or NaN for a non-finite S)
TRASE_RGD_HD double polar3_frobenius(const float* S) {
  TRASE_RGD_NO_CONTRACT
  double f = 0.0;
  for (int q = 0; q < 9; ++q) f += (double)S[q] * (double)S[q];
  return sqrt(f);
}

// the degenerate rule: s23 = sigma_2 + sigma_3 as polar3 returns it, k edges, m = sum |e1| |e2| (NaN compares false: not degenerate)
TRASE_RGD_HD bool polar3_is_degenerate(double s23, double k, double m) {
  TRASE_RGD_NO_CONTRACT
  return s23 <= 4.0 * (k + 2.0) * RGD_U * m;
}

// R (row-major 3 x 3) = V U^T; returns sigma_2 + sigma_3 (NaN for a non-finite S)
TRASE_RGD_HD double polar3(const float* S, float* R) {
  TRASE_RGD_NO_CONTRACT
  const double fro = polar3_frobenius(S);
  if (!(fro <= 1.7976931348623157e308)) {
    for (int q = 0; q < 9; ++q) R[q] = NAN;
    return NAN;
  }
  RgdCol b0 = {S[0], S[3], S[6]}, b1 = {S[1], S[4], S[7]}, b2 = {S[2], S[5], S[8]};
  RgdCol v0 = {1.0, 0.0, 0.0}, v1 = {0.0, 1.0, 0.0}, v2 = {0.0, 0.0, 1.0};
  for (int sweep = 0; sweep < RGD_SWEEPS; ++sweep) {
    bool any = rgd_rotate(b0, b1, v0, v1);
    any = rgd_rotate(b0, b2, v0, v2) || any;
    any = rgd_rotate(b1, b2, v1, v2) || any;
    if (!any) break;
  }
  double n0 = rgd_dot(b0, b0), n1 = rgd_dot(b1, b1), n2 = rgd_dot(b2, b2);
  double det_v = 1.0;                                        // every rotation is proper; a swap of two columns is not
  if (n0 < n1) { rgd_swap(b0, b1); rgd_swap(v0, v1); const double t = n0; n0 = n1; n1 = t; det_v = -det_v; }
  if (n0 < n2) { rgd_swap(b0, b2); rgd_swap(v0, v2); const double t = n0; n0 = n2; n2 = t; det_v = -det_v; }
  if (n1 < n2) { rgd_swap(b1, b2); rgd_swap(v1, v2); const double t = n1; n1 = n2; n2 = t; det_v = -det_v; }
  if (!(n0 > 0.0)) {                                          // S = 0
    for (int q = 0; q < 9; ++q) R[q] = (q == 0 || q == 4 || q == 8) ? 1.f : 0.f;
    return 0.0;
  }
  const double s1 = sqrt(n0), s2 = sqrt(n1), s3 = sqrt(n2);
  const RgdCol u0 = rgd_scale(b0, 1.0 / s1);
  // u1 = b1 / sigma_2 where b1 is a direction of its own.  It is not where sigma_2 = 0, or where b1 is what cancellation left of a
  // column PARALLEL to b0 (rank 1 with exactly proportional columns: every rotation leaves 2^-53 of it, parallel again, and the sweep
  // bound ends that): then any unit vector orthogonal to u0 completes the basis -- u0 x the axis u0 has least of
  RgdCol u1 = u0, w = {0.0, 0.0, 0.0};
  if (n1 > 0.0) {
    u1 = rgd_scale(b1, 1.0 / s2);
    w = rgd_cross(u0, u1);
  }
  if (!(n1 > 0.0) || rgd_dot(w, w) < 0.5) {
    const double ax = fabs(u0.x), ay = fabs(u0.y), az = fabs(u0.z);
    const RgdCol e = (ax <= ay && ax <= az) ? RgdCol{1.0, 0.0, 0.0} : (ay <= az ? RgdCol{0.0, 1.0, 0.0} : RgdCol{0.0, 0.0, 1.0});
    const RgdCol t = rgd_cross(u0, e);
    u1 = rgd_scale(t, 1.0 / sqrt(rgd_dot(t, t)));
    w = rgd_cross(u0, u1);
  }
  const double d = rgd_dot(b2, w);
  const double sign = d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : det_v);
  const RgdCol u2 = rgd_scale(w, sign / sqrt(rgd_dot(w, w)));
  R[0] = (float)(v0.x * u0.x + v1.x * u1.x + v2.x * u2.x);
  R[1] = (float)(v0.x * u0.y + v1.x * u1.y + v2.x * u2.y);
  R[2] = (float)(v0.x * u0.z + v1.x * u1.z + v2.x * u2.z);
  R[3] = (float)(v0.y * u0.x + v1.y * u1.x + v2.y * u2.x);
  R[4] = (float)(v0.y * u0.y + v1.y * u1.y + v2.y * u2.y);
  R[5] = (float)(v0.y * u0.z + v1.y * u1.z + v2.y * u2.z);
  R[6] = (float)(v0.z * u0.x + v1.z * u1.x + v2.z * u2.x);
  R[7] = (float)(v0.z * u0.y + v1.z * u1.y + v2.z * u2.y);
  R[8] = (float)(v0.z * u0.z + v1.z * u1.z + v2.z * u2.z);
  return s2 + s3;
}

// gS for the cotangent G of R = polar3(S), on a row that is not degenerate (the caller zeroes a degenerate row's gS)
TRASE_RGD_HD void polar3_bwd(const float* S, const float* R, const float* G, float* gS) {
  TRASE_RGD_NO_CONTRACT
  double H[9], W[9];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      H[3 * a + b] = (double)R[a] * (double)S[3 * b] + (double)R[3 + a] * (double)S[3 * b + 1] + (double)R[6 + a] * (double)S[3 * b + 2];
      W[3 * a + b] = (double)R[a] * (double)G[b] + (double)R[3 + a] * (double)G[3 + b] + (double)R[6 + a] * (double)G[6 + b];
    }
  const double h01 = 0.5 * (H[1] + H[3]), h02 = 0.5 * (H[2] + H[6]), h12 = 0.5 * (H[5] + H[7]);
  // M = tr(H) I - H
  const double m00 = H[4] + H[8], m11 = H[0] + H[8], m22 = H[0] + H[4], m01 = -h01, m02 = -h02, m12 = -h12;
  const double b0 = W[7] - W[5], b1 = W[2] - W[6], b2 = W[3] - W[1];
  const double c00 = m11 * m22 - m12 * m12, c01 = m02 * m12 - m01 * m22, c02 = m01 * m12 - m02 * m11;
  const double c11 = m00 * m22 - m02 * m02, c12 = m01 * m02 - m00 * m12, c22 = m00 * m11 - m01 * m01;
  const double inv = 1.0 / (m00 * c00 + m01 * c01 + m02 * c02);
  const double y0 = (c00 * b0 + c01 * b1 + c02 * b2) * inv;
  const double y1 = (c01 * b0 + c11 * b1 + c12 * b2) * inv;
  const double y2 = (c02 * b0 + c12 * b1 + c22 * b2) * inv;
  for (int a = 0; a < 3; ++a) {                                // (R [y]_x)_ab -> gS_ba
    const double r0 = R[3 * a], r1 = R[3 * a + 1], r2 = R[3 * a + 2];
    gS[a] = (float)(r1 * y2 - r2 * y1);
    gS[3 + a] = (float)(r2 * y0 - r0 * y2);
    gS[6 + a] = (float)(r0 * y1 - r1 * y0);
  }
}

// the two functions on a matrix of its own (k = 1, m = |S|_F): what trase_polar3_forward / _backward evaluate per row
TRASE_RGD_HD void polar3_row_bwd(const float* S, const float* R, const float* G, float* gS) {
  float tmp[9];
  const double s23 = polar3(S, tmp);
  if (polar3_is_degenerate(s23, 1.0, polar3_frobenius(S))) {
    for (int q = 0; q < 9; ++q) gS[q] = 0.f;
    return;
  }
  polar3_bwd(S, R, G, gS);
}

}  // namespace trase
