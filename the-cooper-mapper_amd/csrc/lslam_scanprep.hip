// lslam_scanprep.hip -- device side of lslam_scan_set_batch: Morton ordering of the resident scans.
//
// Scan points are processed one per lane and a wavefront is as slow as its most expensive kd-tree
// traversal, so every cloud (per scan: corner, surf) is ordered along a Morton curve of 0.25 m cells
// (see lslam_api.hip).  The order is the one the host implementation defines -- ascending
// (30-bit Morton key, original index) inside each cloud -- produced here by ONE stable radix sort
// (rocPRIM) of the whole batch on the key (cloud id | Morton key); the original index travels in .w.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include "lslam_internal.hpp"

namespace lslam {

namespace {

__device__ __forceinline__ uint32_t spread10(uint32_t v) {
  v &= 0x3FFu;
  v = (v | (v << 16)) & 0x030000FFu;
  v = (v | (v << 8)) & 0x0300F00Fu;
  v = (v | (v << 4)) & 0x030C30C3u;
  v = (v | (v << 2)) & 0x09249249u;
  return v;
}
__device__ __forceinline__ uint32_t quant(float v) {
  float c = __fadd_rn(__fmul_rn(v, 4.0f), 512.0f);  // 0.25 m cells, +-128 m
  c = c < 0.0f ? 0.0f : (c > 1023.0f ? 1023.0f : c);
  return (uint32_t)c;
}

__global__ void sp_key_kernel(const float4 *pts, int n, const int32_t *seg_off, int nseg, uint64_t *keys,
                              uint32_t *idx) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int lo = 0, hi = nseg - 1;  // last segment with seg_off <= i
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (seg_off[mid] <= i) lo = mid; else hi = mid - 1;
  }
  const float4 p = pts[i];
  const uint32_t m = spread10(quant(p.x)) | (spread10(quant(p.y)) << 1) | (spread10(quant(p.z)) << 2);
  keys[i] = ((uint64_t)lo << 30) | m;
  idx[i] = (uint32_t)i;
}

__global__ void sp_gather_kernel(const float4 *pts, const uint32_t *idx, const uint64_t *keys, const int32_t *seg_off,
                                 int n, float4 *out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t src = idx[i];
  float4 p = pts[src];
  const int seg = (int)(keys[i] >> 30);
  p.w = __builtin_bit_cast(float, src - (uint32_t)seg_off[seg]);  // index inside its own cloud
  out[i] = p;
}

}  // namespace

struct ScanPrep {  // the context's (ctx_slot), grow-only
  DevBuf<uint64_t> keys0, keys1;
  DevBuf<uint32_t> idx0, idx1;
  DevBuf<float4> raw;
  DevBuf<int32_t> seg;
  DevBuf<char> tmp;
};

// h_pts: n packed points in caller order (cloud after cloud); h_seg_off: nseg + 1 offsets.
// Writes the ordered points to d_out (n float4) on the context's stream, asynchronously: h_pts must stay untouched until that
// stream has been waited for.
static hipError_t order_impl(lslam_ctx *ctx, const float4 *h_pts, const float4 *const *d_clouds, size_t n, const int32_t *h_seg_off, int nseg,
                             float4 *d_out);
hipError_t scanprep_order(lslam_ctx *ctx, const float4 *h_pts, size_t n, const int32_t *h_seg_off, int nseg, float4 *d_out) {
  return order_impl(ctx, h_pts, nullptr, n, h_seg_off, nseg, d_out);
}
// The same for clouds that are in device memory already: they are copied into the staging array device to device (the
// original index is recomputed by the gather: .w of the input is not read), the kernels are the same.
hipError_t scanprep_order_device(lslam_ctx *ctx, const float4 *const *d_clouds, size_t n, const int32_t *h_seg_off, int nseg, float4 *d_out) {
  return order_impl(ctx, nullptr, d_clouds, n, h_seg_off, nseg, d_out);
}
static hipError_t order_impl(lslam_ctx *ctx, const float4 *h_pts, const float4 *const *d_clouds, size_t n, const int32_t *h_seg_off, int nseg,
                             float4 *d_out) {
  if (n == 0) return hipSuccess;
  ScanPrep *sp = ctx_slot<ScanPrep>(ctx, CTX_SLOT_SCANPREP);
  hipStream_t s = ctx_stream(ctx);
  hipError_t e;
  if ((e = sp->keys0.reserve(n)) != hipSuccess || (e = sp->keys1.reserve(n)) != hipSuccess || (e = sp->idx0.reserve(n)) != hipSuccess ||
      (e = sp->idx1.reserve(n)) != hipSuccess || (e = sp->raw.reserve(n)) != hipSuccess || (e = sp->seg.reserve((size_t)nseg + 1)) != hipSuccess)
    return e;
  if (h_pts) {
    if ((e = hipMemcpyAsync(sp->raw.p, h_pts, n * sizeof(float4), hipMemcpyHostToDevice, s)) != hipSuccess) return e;
  } else {
    for (int k = 0; k < nseg; ++k) {
      const size_t cnt = (size_t)(h_seg_off[k + 1] - h_seg_off[k]);
      if (cnt && (e = hipMemcpyAsync(sp->raw.p + h_seg_off[k], d_clouds[k], cnt * sizeof(float4), hipMemcpyDeviceToDevice, s)) != hipSuccess) return e;
    }
  }
  if ((e = hipMemcpyAsync(sp->seg.p, h_seg_off, ((size_t)nseg + 1) * 4, hipMemcpyHostToDevice, s)) != hipSuccess) return e;
  int seg_bits = 1;
  while ((1 << seg_bits) < nseg) ++seg_bits;
  const unsigned end_bit = 30u + (unsigned)seg_bits;
  uint64_t *k0 = sp->keys0.p, *k1 = sp->keys1.p;
  uint32_t *i0 = sp->idx0.p, *i1 = sp->idx1.p;
  // the library's radix sort; LSLAM_SMALL_SORT=1 (A/B): lslam_sort.hip for a frame's scan (<= SMALL_SORT_MAX points)
  const bool small = n <= SMALL_SORT_MAX && env_once().small_sort;
  size_t tmp_bytes = 0;
  if (small) tmp_bytes = small_sort_tmp_bytes(n);
  else if ((e = rocprim::radix_sort_pairs(nullptr, tmp_bytes, k0, k1, i0, i1, n, 0u, end_bit, s)) != hipSuccess) return e;
  if ((e = sp->tmp.reserve(tmp_bytes)) != hipSuccess) return e;
  const dim3 blk(256), grd((unsigned)((n + 255) / 256));
  hipLaunchKernelGGL(sp_key_kernel, grd, blk, 0, s, (const float4 *)sp->raw.p, (int)n, (const int32_t *)sp->seg.p, nseg, k0, i0);
  if (small) e = small_sort_pairs(s, k0, k1, i0, i1, n, sp->tmp.p);
  else e = rocprim::radix_sort_pairs(sp->tmp.p, tmp_bytes, k0, k1, i0, i1, n, 0u, end_bit, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(sp_gather_kernel, grd, blk, 0, s, (const float4 *)sp->raw.p, i1, k1, (const int32_t *)sp->seg.p, (int)n,
                     d_out);
  // No wait: h_seg_off is pageable (consumed when hipMemcpyAsync returned), h_pts is the context's pinned staging area,
  // which the caller does not touch again before it has waited on `s` (lslam_ctx::stage_busy).
  return hipGetLastError();
}

}  // namespace lslam
