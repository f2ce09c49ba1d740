// lslam_info.hip -- edge information: the Gauss-Newton normal matrix of a scan match in the pose graph's edge coordinates,
// summed in fp64 (include/lslam_c.h, "edge information", is the specification; tests/edge_information_ref.py restates it).
//
// Input: what a sweep's taps leave on the device (coeff, flags, in the caller's point order) and the ordered resident scan.
// Per kept row J = [R^T c | 2 p x (R^T c)] in fp64; the 21 upper-triangular products, b^2 and three counters are summed
//   lane (serial over its points) -> wavefront (butterfly) -> workgroup (its wavefronts in order) -> one final workgroup over
//   the partials in workgroup order,
// with no floating-point atomic anywhere: the order is a function of the point count alone, two calls give the same bits.
//
// The reduction is VALU, not v_mfma_f64_16x16x4_f64.  A row contributes 21 distinct products; the MFMA form (rows as K, J^T
// padded from 6 to 16) computes 256 per row, needs J staged through LDS into the A / B layouts (the f64 C / D layout spreads a
// 16 x 16 tile over four registers per lane, row = 4 * (lane / 16) + register), and fixes a summation order inside the
// instruction that the specification could not state.  A keyframe-sized scan is ~20 000 rows: 0.4 M fp64 multiply-adds, a few
// microseconds of VALU time, behind 36 bytes of loads per point -- the kernel is bound by launch and load latency either way.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "lslam_internal.hpp"

namespace lslam {

namespace {

constexpr int INFO_BLOCK = 256;       // lanes of a workgroup
constexpr int INFO_MAX_BLOCKS = 256;  // workgroups of a launch at most: a lane then takes several points, serially
constexpr int INFO_WAVES = INFO_BLOCK / 64;

struct InfoRot {
  double r[9];  // row-major: the same bits the host reference uses
};

__global__ __launch_bounds__(INFO_BLOCK) void info_partial_kernel(const float4 *__restrict__ q, int n, int n_corner,
                                                                   const float4 *__restrict__ coeff,
                                                                   const uint8_t *__restrict__ flags, const InfoRot R,
                                                                   double *__restrict__ partials) {
  __shared__ double red[INFO_WAVES][INFO_NOUT];
  double acc[INFO_NOUT];
#pragma unroll
  for (int c = 0; c < INFO_NOUT; ++c) acc[c] = 0.0;
  const int stride = (int)gridDim.x * INFO_BLOCK;
  for (int i = (int)blockIdx.x * INFO_BLOCK + (int)threadIdx.x; i < n; i += stride) {
    const float4 p = q[i];
    const bool surf = i >= n_corner;
    const int gi = (surf ? n_corner : 0) + __float_as_int(p.w);  // the caller's index of this point: where its taps lie
    if ((unsigned)gi >= (unsigned)n) continue;                   // (never for a scan the context ordered)
    const unsigned f = flags[gi];
    acc[23] += (f & 2u) && !surf ? 1.0 : 0.0;
    acc[24] += (f & 2u) && surf ? 1.0 : 0.0;
    if (!(f & 4u)) continue;
    const float4 cf = coeff[gi];
    const double c0 = (double)cf.x, c1 = (double)cf.y, c2 = (double)cf.z, b = (double)cf.w;
    const double px = (double)p.x, py = (double)p.y, pz = (double)p.z;
    double J[6];
    J[0] = (R.r[0] * c0 + R.r[3] * c1) + R.r[6] * c2;  // m = R^T c (-ffp-contract=off: every operation rounded on its own)
    J[1] = (R.r[1] * c0 + R.r[4] * c1) + R.r[7] * c2;
    J[2] = (R.r[2] * c0 + R.r[5] * c1) + R.r[8] * c2;
    J[3] = 2.0 * (py * J[2] - pz * J[1]);  // 2 p x m (the doubling is exact)
    J[4] = 2.0 * (pz * J[0] - px * J[2]);
    J[5] = 2.0 * (px * J[1] - py * J[0]);
    int k = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = r; c < 6; ++c) acc[k++] += J[r] * J[c];
    acc[21] += b * b;
    acc[22] += 1.0;
  }
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < INFO_NOUT; ++c) {
    double v = acc[c];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == 0) red[wave][c] = v;
  }
  __syncthreads();
  if (threadIdx.x < INFO_NOUT) {
    double v = red[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < INFO_WAVES; ++w) v += red[w][threadIdx.x];
    partials[(size_t)blockIdx.x * INFO_NOUT + threadIdx.x] = v;
  }
}

__global__ __launch_bounds__(64) void info_final_kernel(const double *__restrict__ partials, int n_blocks, double *__restrict__ out) {
  if (threadIdx.x >= INFO_NOUT) return;
  double v = 0.0;
  for (int b = 0; b < n_blocks; ++b) v += partials[(size_t)b * INFO_NOUT + threadIdx.x];
  out[threadIdx.x] = v;
}

int info_blocks(size_t n) {
  const size_t nb = (n + INFO_BLOCK - 1) / INFO_BLOCK;
  return (int)(nb < (size_t)INFO_MAX_BLOCKS ? nb : (size_t)INFO_MAX_BLOCKS);
}

}  // namespace

size_t info_partial_doubles(size_t n) { return (size_t)(info_blocks(n) ? info_blocks(n) : 1) * INFO_NOUT; }

hipError_t launch_match_information(const float4 *q, int n, int n_corner, const float4 *coeff, const uint8_t *flags, const double R[9],
                                    double *partials, double *out25, hipStream_t s) {
  if (n < 0 || n_corner < 0 || n_corner > n || !partials || !out25 || (n && (!q || !coeff || !flags))) return hipErrorInvalidValue;
  const int nb = info_blocks((size_t)n);
  if (nb) {
    InfoRot rot;
    for (int i = 0; i < 9; ++i) rot.r[i] = R[i];
    hipLaunchKernelGGL(info_partial_kernel, dim3((unsigned)nb), dim3(INFO_BLOCK), 0, s, q, n, n_corner, coeff, flags, rot, partials);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(info_final_kernel, dim3(1), dim3(64), 0, s, partials, nb, out25);
  return hipGetLastError();
}

}  // namespace lslam
