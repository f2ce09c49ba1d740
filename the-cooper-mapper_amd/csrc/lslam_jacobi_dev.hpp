// lslam_jacobi_dev.hpp -- the cyclic Jacobi iteration on a symmetric 3x3 matrix in fp64, shared by the survey extractor's
// normals (lslam_survey.hip: sv_normals_kernel) and the map-quality tail (lslam_mapq.hip: mq_tail_kernel).  Both include this
// one definition, so their eigenvalues are the same bits for the same covariance (the precedent: rigid_transform_point of
// lslam_device.hpp); tests/survey_map_ref.py's _rotate performs the same operations in the same order.
#pragma once

#include <hip/hip_runtime.h>

namespace lslam {

constexpr int JACOBI_SWEEPS = 10;  // cyclic sweeps of the 3x3 Jacobi iteration: a fixed count (fp64 converges in five or six)

// One rotation of the cyclic Jacobi iteration on the symmetric 3x3 matrix {app, aqq, apq, arp, arq} (r: the third index): the
// matrix entries, and the rotation (c, s) for a caller that keeps eigenvectors.  false: apq is zero already, nothing rotates.
// Only + - * / sqrt: tests/survey_map_ref.py performs the same operations in the same order.
__device__ __forceinline__ bool sv_rotate(double &app, double &aqq, double &apq, double &arp, double &arq, double &c, double &s) {
  if (apq == 0.0) return false;
  const double theta = (aqq - app) / (2.0 * apq);
  const double root = sqrt(theta * theta + 1.0);
  const double t = theta >= 0.0 ? 1.0 / (theta + root) : -1.0 / (root - theta);
  c = 1.0 / sqrt(t * t + 1.0);
  s = t * c;
  const double h = t * apq;
  app = app - h;
  aqq = aqq + h;
  apq = 0.0;
  const double rp = c * arp - s * arq, rq = s * arp + c * arq;
  arp = rp;
  arq = rq;
  return true;
}
// ... for the eigenvalues alone
__device__ __forceinline__ void sv_rotate(double &app, double &aqq, double &apq, double &arp, double &arq) {
  double c, s;
  (void)sv_rotate(app, aqq, apq, arp, arq, c, s);
}
// ... and with the eigenvector columns p, q
__device__ __forceinline__ void sv_rotate(double &app, double &aqq, double &apq, double &arp, double &arq, double *vp, double *vq) {
  double c, s;
  if (!sv_rotate(app, aqq, apq, arp, arq, c, s)) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double a = c * vp[k] - s * vq[k], b = s * vp[k] + c * vq[k];
    vp[k] = a;
    vq[k] = b;
  }
}

}  // namespace lslam
