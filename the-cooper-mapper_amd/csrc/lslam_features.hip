// lslam_features.hip -- feature-extraction front end on the device:
// ScanRegistration::extractFeatures (odometry/ScanRegistration.cpp:190-425) on the ring-sorted
// full-resolution cloud, one workgroup per scan ring.
//
// What is parallel and what is not.  Everything that does not depend on the order of picking runs
// across the workgroup: the neighbour tests behind setScanBuffersFor (:471-531), the curvature of
// every region point (:427-455), the stable ascending order by curvature (a rank sort: rank =
// #smaller + #equal-with-lower-index, which is what the reference's `<=` merge sort produces,
// :151-186), and pointClassify (:557-687, two 6-point line fits with the 3x3 symmetric
// eigen-solver) for every point whose curvature reaches the threshold -- exactly the set the
// reference's third loop visits.  The picking itself (marks applied in scan order, at most
// maxSurfaceFlat / maxCornerSharp picks per region with markAsPicked exclusion, regions of a ring
// sharing one mark array) is sequential by definition and is done by lane 0 on LDS-resident state:
// a few thousand integer steps per ring, all rings in parallel.  The per-ring VoxelGrid of the
// less-flat points (:398-407) is the segment filter of lslam_fmap.hip.
#include "../../include/lslam_c.h"

#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "lslam_device.hpp"
#include "lslam_internal.hpp"

namespace {

constexpr int FX_BLOCK = 1024;  // a ring of 1 800 points: every point of every region has a thread in the parallel phases
constexpr int MAXR = 2560;  // points per ring held in LDS
constexpr int SKEY = 8192;  // sort words of a ring's regions (each region padded to a power of two); later 2 x MAXR x 3 floats of pointClassify

// PointLabel, ScanRegistration.h:22-42
enum : int {
  L_UNKNOW = 6, L_SURF_PICKED_NEAR = 3, L_CORNER_SHARP = 1, L_SURFACE_LESS_FLAT = 0, L_SURFACE_FLAT = -1,
  L_ONESIDE_FLAT = 5, L_EDGE_BROKEN = -2, L_NEAR_BLOCK = -3, L_BLIND_BLOCK = -4, L_MESSY = 9
};

struct FxArgs {
  const float4 *pts;        // n_points {x, y, z, intensity-to-copy}
  const int32_t *ranges;    // n_scans x {first, last}
  int32_t n_scans;
  int32_t nf, cr, max_sharp, max_flat;
  float surf_thr, blind_thr;
  double c175, c5, c135, c45;  // cos of the pointClassify angle gates, evaluated on the host
  // staging: every ring writes, from its own first index on, the cloud indices of its picks (index
  // stores only: the sequential picking never waits for a global load)
  int32_t *st_sharp, *st_less_sharp, *st_flat, *st_less_flat;
  int32_t *counts;          // [n_scans][4]
  float *curv_out;          // optional taps, [n_points]
  int8_t *picked_out, *label_out;
  // pointClassify by helper workgroups (fx_ring_kernel): `helpers` per ring, their verdicts in cls_g[n_points], ready[ring]
  // counts the helpers that have published
  int32_t helpers;
  int32_t *cls_g, *ready;
};

__device__ __forceinline__ float fx_pdist(float x, float y, float z) {
  return sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)), __fmul_rn(z, z)));
}

// one half of pointClassify; sign < 0: points idx-0 .. idx-cr, sign > 0: idx+cr .. idx+0
__device__ bool fx_one_sided_line(const float *sx, const float *sy, const float *sz, int idx, int cr, int sign,
                                  float (&v)[3]) {
  float c[3] = {0.f, 0.f, 0.f};
  for (int q = 0; q <= cr; ++q) {
    const int k = sign < 0 ? idx - q : idx + (cr - q);
    c[0] = __fadd_rn(c[0], sx[k]);
    c[1] = __fadd_rn(c[1], sy[k]);
    c[2] = __fadd_rn(c[2], sz[k]);
  }
  const float inv = (float)(cr + 1);
  c[0] = __fdiv_rn(c[0], inv); c[1] = __fdiv_rn(c[1], inv); c[2] = __fdiv_rn(c[2], inv);
  float A[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int q = 0; q <= cr; ++q) {
    const int k = sign < 0 ? idx - q : idx + (cr - q);
    const float a0 = __fsub_rn(sx[k], c[0]), a1 = __fsub_rn(sy[k], c[1]), a2 = __fsub_rn(sz[k], c[2]);
    A[0] = __fadd_rn(A[0], __fmul_rn(a0, a0));
    A[3] = __fadd_rn(A[3], __fmul_rn(a0, a1));
    A[6] = __fadd_rn(A[6], __fmul_rn(a0, a2));
    A[4] = __fadd_rn(A[4], __fmul_rn(a1, a1));
    A[7] = __fadd_rn(A[7], __fmul_rn(a1, a2));
    A[8] = __fadd_rn(A[8], __fmul_rn(a2, a2));
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) A[k] = __fdiv_rn(A[k], inv);
  float D[3], V[9];
  lslam::eig_sym3(A, D, V);
  if (!(D[2] > __fmul_rn(100.0f, D[1]) && D[2] > __fmul_rn(10000.0f, D[0]))) return false;
  v[0] = V[2]; v[1] = V[5]; v[2] = V[8];
  const float vn = fx_pdist(v[0], v[1], v[2]);
  for (int q = 0; q <= cr; ++q) {
    const int k = sign < 0 ? idx - q : idx + (cr - q);
    const float a0 = __fsub_rn(sx[k], c[0]), a1 = __fsub_rn(sy[k], c[1]), a2 = __fsub_rn(sz[k], c[2]);
    const float cx = __fsub_rn(__fmul_rn(a1, v[2]), __fmul_rn(a2, v[1]));
    const float cy = __fsub_rn(__fmul_rn(a2, v[0]), __fmul_rn(a0, v[2]));
    const float cz = __fsub_rn(__fmul_rn(a0, v[1]), __fmul_rn(a1, v[0]));
    const float distance = __fdiv_rn(fx_pdist(cx, cy, cz), vn);
    if ((double)fabsf(distance) > 0.08) return false;
  }
  return true;
}

// pointClassify from its two one-sided fits (:557-687)
__device__ int fx_point_classify(const bool line1, const float (&v1)[3], const bool line2, const float (&v2)[3], const FxArgs &a) {
  if (line1 && line2) {
    const float ab = __fadd_rn(__fadd_rn(__fmul_rn(v1[0], v2[0]), __fmul_rn(v1[1], v2[1])), __fmul_rn(v1[2], v2[2]));
    const float dis = __fmul_rn(fx_pdist(v1[0], v1[1], v1[2]), fx_pdist(v2[0], v2[1], v2[2]));
    const double diff = (double)__fdiv_rn(ab, dis);
    if (diff < a.c175 || diff > a.c5) return L_SURFACE_FLAT;
    if (diff > a.c135 && diff < a.c45) return L_CORNER_SHARP;
  }
  return (line1 || line2) ? L_ONESIDE_FLAT : L_MESSY;
}

// setRegionBuffersFor, :437-454: the curvature of ring point i
__device__ __forceinline__ float fx_curvature(const float *sx, const float *sy, const float *sz, int i, int cr) {
  const float w = (float)(-2 * cr);
  float dx = __fmul_rn(w, sx[i]), dy = __fmul_rn(w, sy[i]), dz = __fmul_rn(w, sz[i]);
  for (int q = 1; q <= cr; ++q) {
    dx = __fadd_rn(dx, __fadd_rn(sx[i + q], sx[i - q]));
    dy = __fadd_rn(dy, __fadd_rn(sy[i + q], sy[i - q]));
    dz = __fadd_rn(dz, __fadd_rn(sz[i + q], sz[i - q]));
  }
  return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

// Bitonic sort of `count` words in LDS, in independent stretches of `seg` words (a power of two >= 2; every stretch ascending),
// by the whole workgroup.  The sort is bound by LDS traffic (a stage reads and writes every word: sixteen wavefronts' 64-bit
// accesses, 66 stages for 2 048 words were 20 us), so up to three consecutive stages -- strides j, j/2, j/4 -- are done on
// eight words in registers between one read and one write: a third of the traffic and of the barriers.  Word p lives at
// fx_at(p) = p + p / 8: a thread's eight neighbouring words then start 72 bytes after its neighbour's, not 64, and a
// wavefront's accesses spread over all banks.
__device__ __forceinline__ int fx_at(int p) { return p + (p >> 3); }
template <int M>
__device__ __forceinline__ void fx_bitonic_group(unsigned long long *w, int count, int seg, int k, int j) {
  constexpr int PER = 1 << M;
  const int jl = j >> (M - 1);  // smallest stride of the group
  for (int t = threadIdx.x; t < (count >> M); t += FX_BLOCK) {
    const int base = ((t & ~(jl - 1)) << M) | (t & (jl - 1));  // M zero bits inserted above the low log2(jl) bits
    unsigned long long x[PER];
#pragma unroll
    for (int e = 0; e < PER; ++e) x[e] = w[fx_at(base + e * jl)];
    const bool up = ((base & (seg - 1)) & k) == 0;  // (j < k: the same for the eight)
#pragma unroll
    for (int sbit = M - 1; sbit >= 0; --sbit) {
#pragma unroll
      for (int e = 0; e < PER; ++e) {
        if (!(e & (1 << sbit))) {
          const unsigned long long a = x[e], b = x[e | (1 << sbit)];
          const bool sw = (a > b) == up;
          x[e] = sw ? b : a;
          x[e | (1 << sbit)] = sw ? a : b;
        }
      }
    }
#pragma unroll
    for (int e = 0; e < PER; ++e) w[fx_at(base + e * jl)] = x[e];
  }
  __syncthreads();
}
__device__ void fx_bitonic(unsigned long long *w, int count, int seg) {
  for (int k = 2; k <= seg; k <<= 1) {
    int j = k >> 1;
    while (j > 0) {
      if (j >= 4) { fx_bitonic_group<3>(w, count, seg, k, j); j >>= 3; }
      else if (j == 2) { fx_bitonic_group<2>(w, count, seg, k, j); j = 0; }
      else { fx_bitonic_group<1>(w, count, seg, k, j); j = 0; }
    }
  }
}

#ifdef LSLAM_FX_CLOCKS  // profiling build: where a ring's workgroup spends its time (100 MHz ticks, summed over rings and calls)
__device__ unsigned long long fx_clk[8];
#define FX_T(i) if (threadIdx.x == 0) { const unsigned long long _n = wall_clock64(); atomicAdd(&fx_clk[i], _n - fx_last); fx_last = _n; }
#else
#define FX_T(i)
#endif
__global__ __launch_bounds__(FX_BLOCK) void fx_ring_kernel(FxArgs a) {
#ifdef LSLAM_FX_CLOCKS
  unsigned long long fx_last = wall_clock64();
#endif
  __shared__ float sx[MAXR], sy[MAXR], sz[MAXR];
  __shared__ float curv_ring[MAXR];
  __shared__ uint16_t sorted_ring[MAXR];
  __shared__ int8_t picked[MAXR], cls_ring[MAXR], rlabel_ring[MAXR];
  __shared__ uint8_t pfl[MAXR];
  __shared__ uint16_t need[MAXR];
  __shared__ unsigned long long skey[SKEY + SKEY / 8];  // (fx_at)
  __shared__ int reg_sp[512], reg_ep[512];  // (n_feature_regions <= 512)
  __shared__ uint8_t side_ok[2 * MAXR];
  __shared__ int n_need;
  __shared__ int s_ready;
  // The first helpers * n_scans workgroups are HELPERS: pointClassify -- two 6-point line fits through an iterative 3 x 3
  // eigen-solver for ~1 000 points of a ring, a third of this kernel on its one CU while three quarters of the chip idle -- is
  // done for a ring by `helpers` workgroups on CUs of their own, each a share of the ring, published through cls_g / ready
  // while the ring's own workgroup marks and sorts.  Helpers have the lower workgroup indices (dispatched first) and wait
  // for nothing; a ring's workgroup that does not see them in time classifies for itself.  Same values either way.
  const int H = a.helpers, tid = threadIdx.x;
  const bool helper = (int)blockIdx.x < H * a.n_scans;
  const int ring = helper ? (int)blockIdx.x / H : (int)blockIdx.x - H * a.n_scans;
  if (tid == 0) n_need = 0;
  const int start = a.ranges[2 * ring], end = a.ranges[2 * ring + 1];
  const int cr = a.cr, nf = a.nf;
  int n_sharp = 0, n_less_sharp = 0, n_flat = 0, n_less = 0;  // uniform across wavefront 0
  if (!(end <= start + 2 * cr)) {  // :205-207
    const int n = end - start + 1;
    for (int i = tid; i < n; i += FX_BLOCK) {
      const float4 p = a.pts[start + i];
      sx[i] = p.x; sy[i] = p.y; sz[i] = p.z;
    }
    __syncthreads();
    // the points the third loop visits (curvature at or above the threshold), collected first -- any order: a point's class
    // depends on nothing else -- so that the eigen-solver runs on full wavefronts; one LDS atomic per wavefront
    auto collect = [&](bool wanted, int i) {
      const unsigned long long wm = __ballot(wanted);
      int wbase = 0;
      if ((tid & 63) == 0 && wm) wbase = atomicAdd(&n_need, __popcll(wm));
      wbase = __builtin_amdgcn_readfirstlane(wbase);
      if (wanted) need[wbase + __popcll(wm & ((1ull << (tid & 63)) - 1ull))] = (uint16_t)i;
    };
    // the two one-sided fits of a point are work items of their own: direction and verdict wait in the sort words' LDS
    float *side_v = reinterpret_cast<float *>(skey);  // [2 n_need][3]
    auto fit_sides = [&]() {
      for (int t = tid; t < 2 * n_need; t += FX_BLOCK) {
        float v[3] = {0.f, 0.f, 0.f};
        const bool ok = fx_one_sided_line(sx, sy, sz, need[t >> 1], cr, (t & 1) ? +1 : -1, v);
        side_v[3 * t] = v[0]; side_v[3 * t + 1] = v[1]; side_v[3 * t + 2] = v[2];
        side_ok[t] = ok ? 1 : 0;
      }
      __syncthreads();
    };
    auto class_of = [&](int t) {
      const float v1[3] = {side_v[6 * t], side_v[6 * t + 1], side_v[6 * t + 2]};
      const float v2[3] = {side_v[6 * t + 3], side_v[6 * t + 4], side_v[6 * t + 5]};
      return fx_point_classify(side_ok[2 * t] != 0, v1, side_ok[2 * t + 1] != 0, v2, a);
    };
    if (helper) {  // block-uniform
      const int part = (int)blockIdx.x % H, total = n - 2 * cr, chunk = (total + H - 1) / H;
      const int i0 = cr + part * chunk, i1 = min(n - cr, i0 + chunk);
      for (int ib = i0; ib < i1; ib += FX_BLOCK) {
        const int i = ib + tid;
        collect(i < i1 && !(fx_curvature(sx, sy, sz, min(i, i1 - 1), cr) < a.surf_thr), i);
      }
      __syncthreads();
      fit_sides();
      for (int t = tid; t < n_need; t += FX_BLOCK)
        __hip_atomic_store(a.cls_g + start + need[t], class_of(t), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      // every thread's own stores out at agent scope BEFORE the barrier: thread 0's release below orders thread 0's stores, and
      // the barrier's workgroup-scope fence does not wait for the other wavefronts' stores to reach the L2 -- a ring workgroup
      // on another CU could see the count and still load a stale class
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      __syncthreads();
      if (tid == 0) __hip_atomic_fetch_add(a.ready + ring, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
      return;
    }
    // ---- neighbour tests of setScanBuffersFor, one per point pair (i, i+1) ------------------------
    // bit0: cos(angle(p_i, p_i+1)) < blindThreshold   bit1: |p_i+1 - p_i|^2 > 1.0
    // bit2: depth_i > depth_i+1                          bit3: |p_i-1 - p_i|^2 / |p_i+1 - p_i|^2 < 0.2
    for (int i = tid; i < n - 1; i += FX_BLOCK) {
      const float x = sx[i], y = sy[i], z = sz[i], xn = sx[i + 1], yn = sy[i + 1], zn = sz[i + 1];
      const float ab = __fadd_rn(__fadd_rn(__fmul_rn(x, xn), __fmul_rn(y, yn)), __fmul_rn(z, zn));
      const float d1 = fx_pdist(x, y, z), d2 = fx_pdist(xn, yn, zn);
      const float cosang = __fdiv_rn(ab, __fmul_rn(d1, d2));
      const float dx = __fsub_rn(xn, x), dy = __fsub_rn(yn, y), dz = __fsub_rn(zn, z);
      const float diff_next = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
      uint8_t f = 0;
      if (cosang < a.blind_thr) f |= 1;
      if ((double)diff_next > 1.0) f |= 2;
      if (d1 > d2) f |= 4;
      if (i > 0) {
        const float px = __fsub_rn(sx[i - 1], x), py = __fsub_rn(sy[i - 1], y), pz = __fsub_rn(sz[i - 1], z);
        const float diff_prev = __fadd_rn(__fadd_rn(__fmul_rn(px, px), __fmul_rn(py, py)), __fmul_rn(pz, pz));
        if ((double)__fdiv_rn(diff_prev, diff_next) < 0.2) f |= 8;
      }
      pfl[i] = f;
    }
    __syncthreads();
    // The marks of setScanBuffersFor (:477-530) are applied in scan order, later writes over earlier ones, and two of them read
    // what is there -- but a step at pair i only touches points within cr of i, so every point replays, in order, the <= 2 cr
    // steps that can reach it and nothing else (round 5; lane 0 applying them one after the other was a sixth of the kernel).
    for (int p = tid; p < n; p += FX_BLOCK) {
      int v = 0;
      for (int i = 0; i < cr; ++i) {  // :477-495, the ring's two ends (only one value is written: any order)
        if ((pfl[i] & 1) && p >= i && p <= i + cr) v = L_BLIND_BLOCK;
        if ((pfl[n - 1 - i - 1] & 1) && p >= n - 1 - i - cr && p <= n - 1 - i) v = L_BLIND_BLOCK;
      }
      const int i_lo = max(cr, p - cr), i_hi = min(n - 2 - cr, p + cr - 1);
      for (int i = i_lo; i <= i_hi; ++i) {  // :497-530
        const int f = pfl[i];
        if ((f & 3) == 0) continue;
        if (f & 1) {
          if (p >= i - cr + 1 && p <= i + cr) v = L_BLIND_BLOCK;
        } else if (f & 4) {
          if (p == i + 1 && v > L_NEAR_BLOCK && (f & 8)) v = L_EDGE_BROKEN;
          if (p >= i - cr + 1 && p <= i) v = L_NEAR_BLOCK;
        } else {
          if (p == i && v > L_NEAR_BLOCK && (f & 8)) v = L_EDGE_BROKEN;
          if (p >= i + 1 && p <= i + cr) v = L_NEAR_BLOCK;
        }
      }
      picked[p] = (int8_t)v;
    }
    __syncthreads();
    FX_T(0)
    if (a.picked_out)
      for (int i = tid; i < n; i += FX_BLOCK) a.picked_out[start + i] = picked[i];
    // ---- everything about the regions that does not depend on the picking, for ALL regions at once -------------
    // (curvature, the stable rank inside the region, pointClassify: a region is ~300 points, the ring ~1800 -- region
    // after region a 256-thread workgroup ran these in twelve rounds, most of the time of the kernel)
    const size_t S = (size_t)start + cr, E = (size_t)end - cr;
    // the regions' bounds (:208-209), once per ring: two 64-bit divisions each, which every thread of every phase repeated
    for (int j = tid; j < nf; j += FX_BLOCK) {
      reg_sp[j] = (int)((S * (size_t)(nf - j) + E * (size_t)j) / (size_t)nf);
      reg_ep[j] = (int)((S * (size_t)(nf - 1 - j) + E * (size_t)(j + 1)) / (size_t)nf) - 1;
    }
    __syncthreads();
    auto region_of = [&](int j, int &sp, int &ep) {
      sp = reg_sp[j];
      ep = reg_ep[j];
    };
    {
      for (int i = cr + tid; i <= n - 1 - cr; i += FX_BLOCK) {
        curv_ring[i] = fx_curvature(sx, sy, sz, i, cr);
        rlabel_ring[i] = L_UNKNOW;
      }
      __syncthreads();
      FX_T(1)
      // The stable ascending order by curvature inside every region (what the reference's `<=` merge sort yields, :151-186):
      // curvature is a sum of squares, so its bit pattern orders like its value, and (bits << 16 | index in region) sorts by
      // curvature, then index.  All regions at once, each in its own power-of-two stretch of `skey`, bitonic (round 5: the rank
      // sort this replaces -- every point counting the smaller ones of its region -- was a quarter of the kernel).
      int rs_max = 0;
      for (int j = 0; j < nf; ++j) {
        int sp, ep;
        region_of(j, sp, ep);
        rs_max = max(rs_max, ep - sp + 1);
      }
      int rpad = 2, rlg = 1;
      while (rpad < rs_max) { rpad <<= 1; ++rlg; }  // block-uniform; nf * rpad <= SKEY (regions are equal to +-1; the host bounds nf)
      for (int t = tid; t < nf * rpad; t += FX_BLOCK) {
        const int j = t >> rlg, r = t & (rpad - 1);
        int sp, ep;
        region_of(j, sp, ep);
        const int rs = ep > sp ? ep - sp + 1 : 0;  // :210 skips a region of one point
        unsigned long long w = ~0ull;
        bool wanted = false;
        int i = 0;
        if (r < rs) {
          i = sp - start + r;
          const float c = curv_ring[i];
          w = ((unsigned long long)__float_as_uint(c) << 16) | (unsigned long long)r;
          cls_ring[i] = (int8_t)L_UNKNOW;
          wanted = !(c < a.surf_thr);
          if (a.curv_out) a.curv_out[start + i] = c;
        }
        skey[fx_at(t)] = w;
        collect(wanted, i);
      }
      __syncthreads();
      fx_bitonic(skey, nf * rpad, rpad);
      for (int t = tid; t < nf * rpad; t += FX_BLOCK) {
        const int j = t >> rlg, r = t & (rpad - 1);
        int sp, ep;
        region_of(j, sp, ep);
        const int rs = ep > sp ? ep - sp + 1 : 0;
        if (r < rs) sorted_ring[sp - start + r] = (uint16_t)(skey[fx_at(t)] & 0xFFFFull);
      }
      __syncthreads();
      FX_T(5)
      // pointClassify of the collected points: the helpers' verdicts if they have all published, else here
      bool have = false;
      if (H > 0) {
        if (tid == 0) {
          int ok = 0;
          for (int spin = 0; spin < (1 << 14) && !ok; ++spin) {
            ok = __hip_atomic_load(a.ready + ring, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) >= H;
            if (!ok) __builtin_amdgcn_s_sleep(16);
          }
          s_ready = ok;
        }
        __syncthreads();
        have = s_ready != 0;
      }
#ifdef LSLAM_FX_CLOCKS
      if (tid == 0) { atomicAdd(&fx_clk[6], (unsigned long long)n_need); atomicAdd(&fx_clk[7], 1ull); }
#endif
      if (have) {
        for (int t = tid; t < n_need; t += FX_BLOCK)
          cls_ring[need[t]] = (int8_t)__hip_atomic_load(a.cls_g + start + need[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } else {
        fit_sides();
        for (int t = tid; t < n_need; t += FX_BLOCK) cls_ring[need[t]] = (int8_t)class_of(t);
      }
      __syncthreads();
      FX_T(2)
    }
    // ---- regions: the picking, in order (regions of a ring share one mark array) -----------------------------
    for (int j = 0; j < nf; ++j) {
      int sp, ep;
      region_of(j, sp, ep);
      if (ep <= sp) continue;  // block-uniform
      const int rs = ep - sp + 1, r0 = sp - start;  // r0: ring-relative index of the region's first point
      const float *curv = curv_ring + r0;            // region-relative views
      const uint16_t *sorted = sorted_ring + r0;
      const int8_t *cls = cls_ring + r0;
      int8_t *rlabel = rlabel_ring + r0;
      if (tid < 64) {  // wavefront 0; the counters are wave-uniform
        const unsigned long long lt_mask = tid == 0 ? 0ull : (~0ull >> (64 - tid));
        // flat surface features, :268-284 -- sequential: every pick excludes its neighbourhood
        // A pick excludes its neighbourhood from the later ones, so the picks are sequential -- but the candidates are not: 64
        // of them (ascending curvature) are tested at once, the first eligible lane is the pick, the lanes within cr of it drop
        // out in registers, its marks are written by 2 cr + 1 lanes (round 5: lane 0 walking the order with two dependent LDS
        // reads per candidate, most of them neighbours of a pick, was a seventh of the kernel).
        int surf_picked = 0;
        for (int base = 0; base < rs && surf_picked < a.max_flat; base += 64) {
          const int k = base + tid;
          const int r = k < rs ? (int)sorted[k] : 0, si = r0 + r;
          bool elig = k < rs && curv[r] < a.surf_thr && picked[si] != L_SURF_PICKED_NEAR;
          const bool more = __ballot(k < rs && curv[r] < a.surf_thr) != 0ull;  // ascending: a chunk without one ends the search
          unsigned long long m;
          while (surf_picked < a.max_flat && (m = __ballot(elig)) != 0ull) {
            const int L = __builtin_ctzll(m);
            const int si_L = __builtin_amdgcn_readlane(si, L);
            if (tid == L) {
              rlabel[r] = L_SURFACE_FLAT;
              a.st_flat[start + n_flat + surf_picked] = sp + r;
            }
            if (tid <= 2 * cr) picked[si_L - cr + tid] = L_SURF_PICKED_NEAR;  // markAsPicked, :533-555
            elig = elig && abs(si - si_L) > cr;
            ++surf_picked;
          }
          if (!more) break;
        }
        n_flat += surf_picked;  // (wave-uniform)
        FX_T(3)
        // less flat + broken edges, :286-302 -- an ordered compaction, 64 region points at a time
        int n_low = 0;
        for (int base = 0; base < rs; base += 64) {
          const int k = base + tid;
          const bool valid = k < rs;
          const bool low = valid && curv[valid ? k : 0] < a.surf_thr;
          const bool eb = valid && picked[r0 + (valid ? k : 0)] == L_EDGE_BROKEN;
          const unsigned long long m1 = __ballot(low), m2 = __ballot(eb);
          if (low) {
            a.st_less_flat[start + n_less + __popcll(m1 & lt_mask)] = sp + k;
            if (rlabel[k] != L_SURFACE_FLAT) rlabel[k] = L_SURFACE_LESS_FLAT;
          }
          if (eb) {
            const int pos = __popcll(m2 & lt_mask);
            a.st_sharp[start + n_sharp + pos] = sp + k;
            a.st_less_sharp[start + n_less_sharp + pos] = sp + k;
            rlabel[k] = L_CORNER_SHARP;
          }
          n_less += __popcll(m1);
          n_low += __popcll(m1);
          n_sharp += __popcll(m2);
          n_less_sharp += __popcll(m2);
        }
        // classified features in descending curvature, :304-354: the loop only reads the marks and
        // counts its own picks, so it is an ordered compaction too (the saturating counters of the
        // reference equal min(max, number of earlier candidates of that kind))
        int run_surf = 0, run_corner = 0;
        const int T = rs - n_low;  // points with curvature >= threshold: sorted[n_low .. rs)
        for (int base = 0; base < T; base += 64) {
          const int t = base + tid;
          const bool valid = t < T;
          const int r = sorted[valid ? rs - 1 - t : 0], si = r0 + r;
          const int lab = valid ? (int)cls[r] : L_MESSY;
          const bool is_f = lab == L_SURFACE_FLAT, is_o = lab == L_ONESIDE_FLAT;
          const bool is_c = lab == L_CORNER_SHARP && picked[si] > L_EDGE_BROKEN;
          const unsigned long long ms = __ballot(is_f || is_o), mc = __ballot(is_c), mo = __ballot(is_o);
          const int surf_before = run_surf + __popcll(ms & lt_mask);
          const int corner_before = run_corner + __popcll(mc & lt_mask);
          // flat picks among the one-side-flat candidates: those with fewer than max earlier surf-like ones
          const bool flat_pick = is_o && surf_before < a.max_flat;
          const bool sharp_pick = is_c && corner_before < a.max_sharp;
          const unsigned long long mfp = __ballot(flat_pick), msp = __ballot(sharp_pick);
          if (is_f || is_o) a.st_less_flat[start + n_less + __popcll(ms & lt_mask)] = sp + r;
          if (flat_pick) a.st_flat[start + n_flat + __popcll(mfp & lt_mask)] = sp + r;
          if (is_c) a.st_less_sharp[start + n_less_sharp + __popcll(mc & lt_mask)] = sp + r;
          if (sharp_pick) a.st_sharp[start + n_sharp + __popcll(msp & lt_mask)] = sp + r;
          if (is_f) rlabel[r] = L_SURFACE_FLAT;
          else if (is_o) rlabel[r] = L_ONESIDE_FLAT;
          else if (is_c) rlabel[r] = L_CORNER_SHARP;
          (void)mo;
          n_less += __popcll(ms);
          n_flat += __popcll(mfp);
          n_less_sharp += __popcll(mc);
          n_sharp += __popcll(msp);
          run_surf += __popcll(ms);
          run_corner += __popcll(mc);
        }
        FX_T(4)
      }
      __syncthreads();
      if (a.label_out)
        for (int r = tid; r < rs; r += FX_BLOCK) a.label_out[sp + r] = rlabel[r];
      __syncthreads();
    }
  }
  if (tid == 0 && !helper) {
    a.counts[4 * ring + 0] = n_sharp;
    a.counts[4 * ring + 1] = n_less_sharp;
    a.counts[4 * ring + 2] = n_flat;
    a.counts[4 * ring + 3] = n_less;
  }
}

// ring r's list (written from its first index) -> out[off[r] ...]; seg_out optional
__global__ void fx_compact_kernel(const float4 *pts, const int32_t *stage, const int32_t *ranges, const int32_t *off,
                                  int n_scans, int total, float4 *out, int32_t *seg_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  int lo = 0, hi = n_scans - 1;  // last ring with off <= i
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= i) lo = mid; else hi = mid - 1;
  }
  out[i] = pts[stage[ranges[2 * lo] + (i - off[lo])]];
  if (seg_out) seg_out[i] = lo;
}


// ---- the lists of a sweep, without the host in between (round 5) ---------------------------------------------------------
// Until round 5 the host fetched the rings' counts, made the offsets, launched four compactions and ran the per-ring
// VoxelGrid of the less-flat points (:398-407) through the general segment filter of lslam_fmap.hip -- a 64-bit merge sort of
// all rings' points at once, sixteen launches and three waits for what is 64 independent problems of <= 2 560 points.  Now:
//   fx_lists_block         one workgroup per small list (sharp, less sharp, flat): the rings' offsets by a scan in LDS, the
//                          points gathered in ring order STRAIGHT INTO PINNED HOST MEMORY, the total next to them (the last
//                          three workgroups of the next kernel's launch)
//   fx_ring_voxel_kernel   one workgroup per ring: pcl::VoxelGrid::applyFilter on the ring's less-flat list entirely in LDS --
//                          bounding box, the "leaf too small" guard, voxel index ijk0 + ijk1 * div0 + ijk2 * div0 * div1,
//                          a bitonic sort of (index, position in the list), heads, their scan, centroids summed in list order
//   fx_lessflat_out_kernel one workgroup per ring: the ring's centroids behind those of the rings before it, into pinned memory
// and ONE wait.  Same arithmetic, same order as the segment filter (tests/test_gpu_features.py holds both against the oracle).
constexpr int VX_PAD = 4096;  // MAXR rounded up to a power of two
static_assert(MAXR <= VX_PAD && VX_PAD <= 4096, "the list position takes the low 12 bits of the sort word");

struct FxOutArgs {
  const float4 *pts;
  const int32_t *ranges, *counts;  // counts[4 * ring + list]
  const int32_t *stage[4];         // per list: the rings' picks (cloud indices), each ring's from its first index on
  int32_t n_scans, cap;            // cap: points a list's slice of `host` holds
  float inv_leaf;                  // 1 / lessFlatFilterSize, as pcl::VoxelGrid forms it
  float4 *vox_stage;               // [n_points] ring r's centroids from ranges[2 r] on
  int32_t *ring_out;               // [n_scans] centroids per ring
  float4 *host;                    // pinned: 16 header slots, then four slices of `cap` points
  uint32_t *hdr;                   // = (uint32_t *)host: [0..2] totals of the small lists, [3] less-flat points out, [4] error
};

// exclusive scan of v over the workgroup's 1024 threads (LDS part[>= 16]); returns this thread's prefix, *total = the sum
__device__ int fx_block_scan(int v, int *part, int *total) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(incl, o, 64);
    if (lane >= o) incl += u;
  }
  __syncthreads();  // (part may still be read from an earlier call)
  if (lane == 63) part[wave] = incl;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < FX_BLOCK / 64; ++w) {
    const int c = part[w];
    before += w < wave ? c : 0;
    all += c;
  }
  *total = all;
  return before + incl - v;
}

__device__ void fx_lists_block(const FxOutArgs &a, const int k) {
  __shared__ int part[FX_BLOCK];
  __shared__ int32_t off[4096 + 1];
  const int tid = threadIdx.x;
  const int per = (a.n_scans + FX_BLOCK - 1) / FX_BLOCK;
  const int r0 = min(a.n_scans, tid * per), r1 = min(a.n_scans, r0 + per);
  int sum = 0;
  for (int r = r0; r < r1; ++r) sum += a.counts[4 * r + k];
  int total;
  int run = fx_block_scan(sum, part, &total);
  for (int r = r0; r < r1; ++r) {
    off[r] = run;
    run += a.counts[4 * r + k];
  }
  if (tid == 0) {
    off[a.n_scans] = total;
    a.hdr[k] = (uint32_t)total;
    if (total > a.cap) a.hdr[4] = 2u;  // (cannot happen: a list holds a point at most once)
  }
  __syncthreads();
  float4 *out = a.host + 16 + (size_t)k * a.cap;
  const int32_t *stage = a.stage[k];
  for (int i = tid; i < min(total, a.cap); i += FX_BLOCK) {
    int lo = 0, hi = a.n_scans - 1;  // last ring with off <= i
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (off[mid] <= i) lo = mid; else hi = mid - 1;
    }
    out[i] = a.pts[stage[a.ranges[2 * lo] + (i - off[lo])]];
  }
}

#ifdef LSLAM_FX_CLOCKS
__device__ unsigned long long vx_clk[8];
#define VX_T(i) if (threadIdx.x == 0) { const unsigned long long _n = wall_clock64(); atomicAdd(&vx_clk[i], _n - vx_last); vx_last = _n; }
#else
#define VX_T(i)
#endif
// one launch: workgroups [0, n_scans) filter a ring each, the three after them gather the small lists (fx_lists_block)
__global__ __launch_bounds__(FX_BLOCK) void fx_ring_voxel_kernel(FxOutArgs a) {
#ifdef LSLAM_FX_CLOCKS
  unsigned long long vx_last = wall_clock64();
#endif
  if ((int)blockIdx.x >= a.n_scans) {  // block-uniform
    fx_lists_block(a, (int)blockIdx.x - a.n_scans);
    return;
  }
  __shared__ float4 sp[MAXR];
  __shared__ unsigned long long key[VX_PAD + VX_PAD / 8];  // (fx_at)
  __shared__ float wred[6][FX_BLOCK / 64];
  __shared__ int part[FX_BLOCK];
  __shared__ int s_err;
  const int ring = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int start = a.ranges[2 * ring];
  const int n = min(a.counts[4 * ring + 3], MAXR);
  if (n <= 0) {  // block-uniform
    if (tid == 0) a.ring_out[ring] = 0;
    return;
  }
  if (tid == 0) s_err = 0;
  // ---- the ring's list and its bounding box (getMinMax3D) ----------------------------------------------------------------
  float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  for (int i = tid; i < n; i += FX_BLOCK) {
    const float4 p = a.pts[a.stage[3][start + i]];
    sp[i] = p;
    mn[0] = fminf(mn[0], p.x); mn[1] = fminf(mn[1], p.y); mn[2] = fminf(mn[2], p.z);
    mx[0] = fmaxf(mx[0], p.x); mx[1] = fmaxf(mx[1], p.y); mx[2] = fmaxf(mx[2], p.z);
  }
#pragma unroll
  for (int d = 0; d < 3; ++d) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      mn[d] = fminf(mn[d], __shfl_xor(mn[d], o, 64));
      mx[d] = fmaxf(mx[d], __shfl_xor(mx[d], o, 64));
    }
    if (lane == 0) { wred[d][wave] = mn[d]; wred[3 + d][wave] = mx[d]; }
  }
  __syncthreads();
  long long vol = 1;
  int32_t b0[3], div[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    float lo = wred[d][0], hi = wred[3 + d][0];
#pragma unroll
    for (int w = 1; w < FX_BLOCK / 64; ++w) { lo = fminf(lo, wred[d][w]); hi = fmaxf(hi, wred[3 + d][w]); }
    // applyFilter's guard and its min_b / div_b (voxel_grid.hpp), as fm_extent_kernel forms them
    vol *= (long long)(__fmul_rn(__fsub_rn(hi, lo), a.inv_leaf)) + 1;
    b0[d] = (int32_t)floorf(__fmul_rn(lo, a.inv_leaf));
    div[d] = (int32_t)floorf(__fmul_rn(hi, a.inv_leaf)) - b0[d] + 1;
  }
  const bool filtered = vol <= 2147483647ll;  // else: PCL warns and hands the cloud back unfiltered
  VX_T(0)
  int npad = 64;
  while (npad < n) npad <<= 1;
  // ---- sort words: voxel index, then the position in the list (a stable sort by index) -----------------------------------
  for (int i = tid; i < npad; i += FX_BLOCK) {
    unsigned long long w = ~0ull;
    if (i < n) {
      unsigned long long idx = (unsigned long long)i;  // unfiltered: every point its own voxel, in list order
      if (filtered) {
        const float4 p = sp[i];
        const float v[3] = {p.x, p.y, p.z};
        int32_t r[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          r[d] = (int32_t)floorf(__fmul_rn(v[d], a.inv_leaf)) - b0[d];
          if (r[d] < 0 || r[d] >= div[d]) {  // a non-finite coordinate
            s_err = 1;
            r[d] = 0;
          }
        }
        idx = ((unsigned long long)r[2] * (unsigned long long)div[1] + (unsigned long long)r[1]) * (unsigned long long)div[0] + (unsigned long long)r[0];
      }
      w = (idx << 12) | (unsigned long long)i;
    }
    key[fx_at(i)] = w;
  }
  __syncthreads();
  VX_T(1)
  fx_bitonic(key, npad, npad);
  VX_T(2)
  // ---- heads, their places, centroids over the members in list order ------------------------------------------------------
  constexpr int PER = VX_PAD / FX_BLOCK;
  const int per = max(1, npad / FX_BLOCK);  // consecutive entries per thread
  int heads = 0;
  for (int u = 0; u < PER; ++u) {
    const int i = tid * per + u;
    if (u < per && i < n) heads += (i == 0 || (key[fx_at(i)] >> 12) != (key[fx_at(i - 1)] >> 12)) ? 1 : 0;
  }
  int total;
  int pos = fx_block_scan(heads, part, &total);
  VX_T(3)
  for (int u = 0; u < PER; ++u) {
    const int i = tid * per + u;
    if (!(u < per && i < n)) continue;
    const unsigned long long vi = key[fx_at(i)] >> 12;
    if (!(i == 0 || vi != (key[fx_at(i - 1)] >> 12))) continue;
    float4 s = sp[(int)(key[fx_at(i)] & 4095ull)];
    if (filtered) {  // PCL starts from a zero vector: 0 + x is x for every x but -0.0f (+0.0f then); an unfiltered point stays as it is
      s.x = __fadd_rn(0.0f, s.x);
      s.y = __fadd_rn(0.0f, s.y);
      s.z = __fadd_rn(0.0f, s.z);
      s.w = __fadd_rn(0.0f, s.w);
    }
    int m = i + 1;
    for (; m < n && (key[fx_at(m)] >> 12) == vi; ++m) {
      const float4 q = sp[(int)(key[fx_at(m)] & 4095ull)];
      s.x = __fadd_rn(s.x, q.x);
      s.y = __fadd_rn(s.y, q.y);
      s.z = __fadd_rn(s.z, q.z);
      s.w = __fadd_rn(s.w, q.w);
    }
    const float cnt = (float)(m - i);
    a.vox_stage[start + pos] = make_float4(__fdiv_rn(s.x, cnt), __fdiv_rn(s.y, cnt), __fdiv_rn(s.z, cnt), __fdiv_rn(s.w, cnt));
    ++pos;
  }
  VX_T(4)
  if (tid == 0) {
    a.ring_out[ring] = total;
    if (s_err) a.hdr[4] = 1u;
  }
}

__global__ __launch_bounds__(FX_BLOCK) void fx_lessflat_out_kernel(FxOutArgs a) {
  __shared__ int part[FX_BLOCK];
  const int ring = blockIdx.x, tid = threadIdx.x;
  int before = 0;
  for (int r = tid; r < ring; r += FX_BLOCK) before += a.ring_out[r];
  int off;
  (void)fx_block_scan(before, part, &off);
  const int cnt = a.ring_out[ring], start = a.ranges[2 * ring];
  float4 *out = a.host + 16 + (size_t)3 * a.cap;
  for (int i = tid; i < cnt && off + i < a.cap; i += FX_BLOCK) out[off + i] = a.vox_stage[start + i];
  if (ring == a.n_scans - 1 && tid == 0) a.hdr[3] = (uint32_t)(off + cnt);
}

// ---- MultiScanRegistration::process (MultiScanRegistration.cpp:94-190, no IMU) -------------------
struct MsArgs {
  const float4 *in;   // raw driver cloud {x, y, z, *}
  int n, n_rings;
  float lower, factor, scan_period, start_ori, end_ori;
  float4 *out;        // {x', y', z', ring + relTime} in the registration's swapped axes, arrival order
  int32_t *ring;      // -1 = dropped
  float *ori_raw;
  int32_t *first_half;  // index of the first kept point at which halfPassed flips
  float *rel_out;       // optional: relTime of every kept point on its own (the IMU branch interpolates with it)
};

__device__ __forceinline__ float ms_mode_a(float ori, float start_ori) {  // :150-156
  if ((double)ori < (double)start_ori - M_PI / 2) ori = (float)((double)ori + 2 * M_PI);
  else if ((double)ori > (double)start_ori + M_PI * 3 / 2) ori = (float)((double)ori - 2 * M_PI);
  return ori;
}

__global__ void ms_prep_kernel(MsArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const float4 p = a.in[i];
  const float x = p.y, y = p.z, z = p.x;  // :127-129
  int ring = -1;
  float ori = 0.0f;
  if (isfinite(x) && isfinite(y) && isfinite(z) &&
      !((double)__fadd_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)), __fmul_rn(z, z)) < 0.0001)) {
    const float angle = atanf(__fdiv_rn(y, sqrtf(__fadd_rn(__fmul_rn(x, x), __fmul_rn(z, z)))));
    const int id = (int)((((double)__fmul_rn(angle, 180.0f) / M_PI) - (double)a.lower) * (double)a.factor + 0.5);
    if (id < a.n_rings && id >= 0) {
      ring = id;
      ori = -atan2f(x, z);
      const float oa = ms_mode_a(ori, a.start_ori);
      if ((double)__fsub_rn(oa, a.start_ori) > M_PI) atomicMin(a.first_half, i);
    }
  }
  a.ring[i] = ring;
  a.ori_raw[i] = ori;
}

__global__ void ms_final_kernel(MsArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const int ring = a.ring[i];
  if (ring < 0) return;
  const float4 p = a.in[i];
  float ori = a.ori_raw[i];
  if (i <= *a.first_half) {  // the point that flips halfPassed is itself still handled as "not passed"
    ori = ms_mode_a(ori, a.start_ori);
  } else {                   // :157-165
    ori = (float)((double)ori + 2 * M_PI);
    if ((double)ori < (double)a.end_ori - M_PI * 3 / 2) ori = (float)((double)ori + 2 * M_PI);
    else if ((double)ori > (double)a.end_ori + M_PI / 2) ori = (float)((double)ori - 2 * M_PI);
  }
  const float rel = __fdiv_rn(__fmul_rn(a.scan_period, __fsub_rn(ori, a.start_ori)), __fsub_rn(a.end_ori, a.start_ori));
  a.out[i] = make_float4(p.y, p.z, p.x, __fadd_rn((float)ring, rel));
  if (a.rel_out) a.rel_out[i] = rel;
}

// ---- the registration node (lslam_sreg_*): the IMU branch of MultiScanRegistration::process and the ring ranges -----------
// Per sweep, behind ms_prep_kernel / ms_final_kernel: sr_stats_kernel (points per ring, the workgroups' largest relTime, the
// last kept point), with an IMU history sr_deskew_kernel (ScanRegistration::setIMUTransformFor + transformToStartIMU, in place
// on the cloud in arrival order), the stable grouping by ring, sr_ranges_kernel (the IndexRange of every ring and the check of
// the extraction's ring limit), then the extraction's three launches on the grouped cloud.
constexpr int SR_BLOCK = 1024;
constexpr int SR_MAX_HIST = 512;  // IMU states a sweep can see (their time offsets sit in LDS); the reference keeps 200
struct SrState {    // an IMUState (ScanRegistration.h:122-170) as one sweep sees it
  double tsec;      // (scanTime - stamp).toSec()
  double dt_prev;   // (stamp - the previous state's stamp).toSec(); 0 for the oldest
  float roll, pitch, yaw;
  float sr, cr, sp, cp, sy, cy;  // what Angle cached on the host when the state was made
  float pos[3], vel[3];
  float pad;
};
static_assert(sizeof(SrState) == 80, "SrState is uploaded as it is");
struct SrCtl {  // uploaded with the sweep: {INT32_MAX, -1, 0...}
  int32_t first_half;  // ms_prep_kernel
  int32_t last_kept;   // arrival index of the last kept point
  int32_t pad[14];
};
// what comes back behind the node's one wait: the extraction's header, the last kept point's IMU state, the ranges
constexpr int SR_RES_WORDS = 32;  // [0..15] FxOutArgs::hdr, [16..27] {roll, pitch, yaw, position, velocity, shift}, [28] points kept
struct SrArgs {
  float4 *pts;          // {x', y', z', ring + relTime} in arrival order (ms_final_kernel's output), de-skewed in place
  const int32_t *ring;  // -1 = dropped
  const float *rel;     // relTime of the kept points; nullptr without an IMU history
  int n, n_rings;
  SrCtl *ctl;
  int32_t *hist;        // [n_rings] points per ring (zeroed by the upload)
  float *bmax;          // [workgroups] max(0, relTime of the workgroup's kept points)
  const SrState *states;
  int n_states;
  SrState start;        // _imuStart: interpolateIMUStateFor(0), made on the host
  float *cur_out;       // 12 floats: the state and shift of the last kept point
};

__global__ __launch_bounds__(SR_BLOCK) void sr_stats_kernel(SrArgs a) {
  __shared__ int32_t h[4096];
  __shared__ float wmax[SR_BLOCK / 64];
  __shared__ int wlast[SR_BLOCK / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int r = tid; r < a.n_rings; r += SR_BLOCK) h[r] = 0;
  __syncthreads();
  const int i = blockIdx.x * SR_BLOCK + tid;
  const int ring = i < a.n ? a.ring[i] : -1;
  float t = 0.0f;
  int last = -1;
  if (ring >= 0 && ring < a.n_rings) {
    atomicAdd(&h[ring], 1);
    if (a.rel) t = fmaxf(0.0f, a.rel[i]);
    last = i;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    t = fmaxf(t, __shfl_xor(t, o, 64));
    last = max(last, __shfl_xor(last, o, 64));
  }
  if (lane == 0) { wmax[wave] = t; wlast[wave] = last; }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < SR_BLOCK / 64; ++w) { t = fmaxf(t, wmax[w]); last = max(last, wlast[w]); }
    a.bmax[blockIdx.x] = t;
    if (last >= 0) atomicMax(&a.ctl->last_kept, last);
  }
  for (int r = tid; r < a.n_rings; r += SR_BLOCK)
    if (h[r]) atomicAdd(&a.hist[r], h[r]);
}

// sin / cos of a float angle as the correctly rounded float: a double evaluation (accurate to a few double ulp) rounded once --
// off by a float ulp only where the exact value lies within ~1e-16 of a rounding boundary
__device__ __forceinline__ float sr_sin(float x) { return (float)sin((double)x); }
__device__ __forceinline__ float sr_cos(float x) { return (float)cos((double)x); }
__device__ __forceinline__ void sr_rot(float c, float s, float &u, float &v) {  // u' = c u - s v, v' = s u + c v (rotZ on x, y)
  const float u0 = u;
  u = __fsub_rn(__fmul_rn(c, u0), __fmul_rn(s, v));
  v = __fadd_rn(__fmul_rn(s, u0), __fmul_rn(c, v));
}

__global__ __launch_bounds__(SR_BLOCK) void sr_deskew_kernel(SrArgs a) {
  __shared__ double tsec[SR_MAX_HIST];
  __shared__ float wpart[SR_BLOCK / 64];
  __shared__ float s_carry;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int k = tid; k < a.n_states; k += SR_BLOCK) tsec[k] = a.states[k].tsec;
  // the walking index of interpolateIMUStateFor never goes back: it is f(the largest relTime among the kept points so far),
  // f(t) = the first state with tsec + t <= 0 (or the last state).  The carry of the workgroups before this one ...
  float c = 0.0f;
  for (int b = tid; b < (int)blockIdx.x; b += SR_BLOCK) c = fmaxf(c, a.bmax[b]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c = fmaxf(c, __shfl_xor(c, o, 64));
  if (lane == 0) wpart[wave] = c;
  __syncthreads();
  if (tid == 0) {
    float m = wpart[0];
#pragma unroll
    for (int w = 1; w < SR_BLOCK / 64; ++w) m = fmaxf(m, wpart[w]);
    s_carry = m;
  }
  __syncthreads();
  const float carry = s_carry;
  // ... and the inclusive prefix maximum inside it (a dropped point contributes the identity, 0)
  const int i = blockIdx.x * SR_BLOCK + tid;
  const int ring = i < a.n ? a.ring[i] : -1;
  const bool kept = ring >= 0 && ring < a.n_rings;
  const float rel = kept ? a.rel[i] : 0.0f;
  float pm = kept ? fmaxf(0.0f, rel) : 0.0f;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float u = __shfl_up(pm, o, 64);
    if (lane >= o) pm = fmaxf(pm, u);
  }
  __syncthreads();  // (wpart is read above)
  if (lane == 63) wpart[wave] = pm;
  __syncthreads();
  pm = fmaxf(pm, carry);
  for (int w = 0; w < wave; ++w) pm = fmaxf(pm, wpart[w]);
  if (!kept) return;
  int lo = 0, hi = a.n_states - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (__dadd_rn(tsec[mid], (double)pm) <= 0.0) hi = mid; else lo = mid + 1;
  }
  const int idx = lo;
  const double time_diff = __dadd_rn(tsec[idx], (double)rel);
  const SrState S = a.states[idx];
  float roll = S.roll, pitch = S.pitch, yaw = S.yaw, sr = S.sr, cr = S.cr, sp = S.sp, cp = S.cp, sy = S.sy, cy = S.cy;
  float pos[3] = {S.pos[0], S.pos[1], S.pos[2]}, vel[3] = {S.vel[0], S.vel[1], S.vel[2]};
  if (!(idx == 0 || time_diff > 0.0)) {  // IMUState::interpolate(history[idx], history[idx - 1], ratio)
    const SrState E = a.states[idx - 1];
    const float ratio = (float)(-time_diff / S.dt_prev);
    const float inv = __fsub_rn(1.0f, ratio);
    roll = __fadd_rn(__fmul_rn(S.roll, inv), __fmul_rn(E.roll, ratio));
    pitch = __fadd_rn(__fmul_rn(S.pitch, inv), __fmul_rn(E.pitch, ratio));
    const double dyaw = (double)__fsub_rn(S.yaw, E.yaw);
    if (dyaw > M_PI) yaw = (float)__dadd_rn((double)__fmul_rn(S.yaw, inv), __dmul_rn(__dadd_rn((double)E.yaw, 2 * M_PI), (double)ratio));
    else if (dyaw < -M_PI) yaw = (float)__dadd_rn((double)__fmul_rn(S.yaw, inv), __dmul_rn(__dsub_rn((double)E.yaw, 2 * M_PI), (double)ratio));
    else yaw = __fadd_rn(__fmul_rn(S.yaw, inv), __fmul_rn(E.yaw, ratio));
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      vel[d] = __fadd_rn(__fmul_rn(S.vel[d], inv), __fmul_rn(E.vel[d], ratio));
      pos[d] = __fadd_rn(__fmul_rn(S.pos[d], inv), __fmul_rn(E.pos[d], ratio));
    }
    sr = sr_sin(roll); cr = sr_cos(roll);
    sp = sr_sin(pitch); cp = sr_cos(pitch);
    sy = sr_sin(yaw); cy = sr_cos(yaw);
  }
  // setIMUTransformFor: the sweep starts at the scan time, so relSweepTime is relTime
  float shift[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) shift[d] = __fsub_rn(__fsub_rn(pos[d], a.start.pos[d]), __fmul_rn(a.start.vel[d], rel));
  // transformToStartIMU: rotateZXY(p, roll, pitch, yaw), + shift, rotateYXZ(p, -start.yaw, -start.pitch, -start.roll)
  float4 p = a.pts[i];
  sr_rot(cr, sr, p.x, p.y);                    // rotZ
  sr_rot(cp, sp, p.y, p.z);                    // rotX
  sr_rot(cy, sy, p.z, p.x);                    // rotY: z' = c z - s x, x' = s z + c x
  p.x = __fadd_rn(p.x, shift[0]);
  p.y = __fadd_rn(p.y, shift[1]);
  p.z = __fadd_rn(p.z, shift[2]);
  sr_rot(a.start.cy, -a.start.sy, p.z, p.x);   // -angle: the sine negated, the cosine kept (Angle::operator-)
  sr_rot(a.start.cp, -a.start.sp, p.y, p.z);
  sr_rot(a.start.cr, -a.start.sr, p.x, p.y);
  a.pts[i] = p;
  if (i == a.ctl->last_kept) {  // _imuCur and _imuPositionShift as the sweep leaves them
    a.cur_out[0] = roll; a.cur_out[1] = pitch; a.cur_out[2] = yaw;
#pragma unroll
    for (int d = 0; d < 3; ++d) { a.cur_out[3 + d] = pos[d]; a.cur_out[6 + d] = vel[d]; a.cur_out[9 + d] = shift[d]; }
  }
}

// IndexRange(first, last) of every ring (MultiScanRegistration.cpp:184-189: an empty ring is {size, size - 1}, {0, 0} at the
// front) from the points per ring; one workgroup.  ranges_fx is what the extraction reads: the same, or every ring empty when
// nothing was kept or a ring has more points than the extraction holds in LDS (hdr[4] = 3: the call fails behind its wait)
__global__ __launch_bounds__(FX_BLOCK) void sr_ranges_kernel(const int32_t *hist, int n_rings, int32_t *ranges_out, int32_t *ranges_fx,
                                                             uint32_t *res) {
  __shared__ int part[FX_BLOCK];
  const int tid = threadIdx.x;
  const int per = (n_rings + FX_BLOCK - 1) / FX_BLOCK;
  const int r0 = min(n_rings, tid * per), r1 = min(n_rings, r0 + per);
  int sum = 0, big = 0;
  for (int r = r0; r < r1; ++r) {
    sum += hist[r];
    big |= hist[r] > MAXR ? 1 : 0;
  }
  int total;
  int run = fx_block_scan(sum, part, &total);
  const int bad = __syncthreads_or(big);
  const bool none = bad || total == 0;
  for (int r = r0; r < r1; ++r) {
    const int first = run;
    run += hist[r];
    const int last = run > 0 ? run - 1 : 0;
    ranges_out[2 * r] = first;
    ranges_out[2 * r + 1] = last;
    ranges_fx[2 * r] = none ? 0 : first;
    ranges_fx[2 * r + 1] = none ? -1 : last;
  }
  if (tid == 0) {
    res[28] = (uint32_t)total;
    if (bad) res[4] = 3u;
  }
}

// the launch sequence's device arrays, carved from one blob of fx_work_bytes
struct FxWork {
  float4 *pts;                // the ring-sorted cloud {x, y, z, intensity-to-copy}
  int32_t *st[4];             // per list: cloud indices of the picks, ring r's from its first index on
  int32_t *ranges, *counts;   // [n_scans][2] {first, last}, [n_scans][4]
  float *curv;                // taps
  int8_t *picked, *label;
  int32_t *ring_out;          // centroids per ring (fx_ring_voxel_kernel)
  float4 *vox;                // ... and the centroids, ring r's from its first index on
  int32_t *cls, *ready;       // the classify helpers' (fx_ring_kernel)
};
size_t fx_work_bytes(size_t n_points, size_t n_scans) {
  const size_t np4 = n_points * sizeof(float4);
  return 5 * np4 + 2 * n_scans * 4 + 4 * n_scans * 4 + n_points * 4 + 2 * n_points + (n_scans + 1) * 4 + np4 + n_points * 4 +
         n_scans * 4 + 256 + 18 * 16;
}
void fx_carve(char *blob, size_t n_points, size_t n_scans, FxWork &w) {
  const size_t np4 = n_points * sizeof(float4);
  char *q = blob;
  auto take = [&](size_t b) { char *r = q; q += (b + 15) & ~(size_t)15; return r; };
  w.pts = (float4 *)take(np4);
  for (int k = 0; k < 4; ++k) w.st[k] = (int32_t *)take(np4);
  w.ranges = (int32_t *)take(2 * n_scans * 4);
  w.counts = (int32_t *)take(4 * n_scans * 4);
  w.curv = (float *)take(n_points * 4);
  w.picked = (int8_t *)take(n_points);
  w.label = (int8_t *)take(n_points);
  w.ring_out = (int32_t *)take((n_scans + 1) * 4);
  w.vox = (float4 *)take(np4);
  w.cls = (int32_t *)take(n_points * 4);
  w.ready = (int32_t *)take(n_scans * 4);
}
// ScanRegistration::extractFeatures on the cloud and ranges in w (device memory both): the three launches every entry point
// shares -- the host-cloud ones and the resident registration node.  out: sixteen header slots, then four slices of `cap`
// points; hdr: [0..2] totals of the small lists, [3] less-flat points, [4] error (zeroed by the caller).  Nothing is waited for.
hipError_t fx_enqueue(hipStream_t s, const lslam_reg_params &prm, const FxWork &w, size_t n_points, size_t n_scans, bool tap_curv,
                      bool tap_picked, bool tap_label, float4 *out, uint32_t *hdr, size_t cap) {
  hipError_t e;
  if (tap_curv && (e = hipMemsetAsync(w.curv, 0, n_points * 4, s)) != hipSuccess) return e;
  if (tap_picked && (e = hipMemsetAsync(w.picked, 0, n_points, s)) != hipSuccess) return e;
  if (tap_label && (e = hipMemsetAsync(w.label, L_UNKNOW, n_points, s)) != hipSuccess) return e;
  FxArgs a{};
  a.pts = w.pts;
  a.ranges = w.ranges;
  a.n_scans = (int32_t)n_scans;
  a.nf = prm.n_feature_regions;
  a.cr = prm.curvature_region;
  a.max_sharp = prm.max_corner_sharp;
  a.max_flat = prm.max_surface_flat;
  a.surf_thr = prm.surface_curvature_threshold;
  a.blind_thr = prm.blind_threshold;
  a.c175 = std::cos(175.0 * M_PI / 180.0);  // deg2rad(double), util/math_utils.h:29
  a.c5 = std::cos(5.0 * M_PI / 180.0);
  a.c135 = std::cos(135.0 * M_PI / 180.0);
  a.c45 = std::cos(45.0 * M_PI / 180.0);
  a.st_sharp = w.st[0]; a.st_less_sharp = w.st[1]; a.st_flat = w.st[2]; a.st_less_flat = w.st[3];
  a.counts = w.counts;
  a.curv_out = tap_curv ? w.curv : nullptr;
  a.picked_out = tap_picked ? w.picked : nullptr;
  a.label_out = tap_label ? w.label : nullptr;
  a.helpers = lslam::env_once().fx_helpers;
  a.cls_g = w.cls;
  a.ready = w.ready;
  if (a.helpers > 0 && (e = hipMemsetAsync(w.ready, 0, n_scans * 4, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(fx_ring_kernel, dim3((unsigned)n_scans * (unsigned)(1 + a.helpers)), dim3(FX_BLOCK), 0, s, a);
  FxOutArgs oa{};
  oa.pts = w.pts;
  oa.ranges = w.ranges;
  oa.counts = w.counts;
  for (int k = 0; k < 4; ++k) oa.stage[k] = w.st[k];
  oa.n_scans = (int32_t)n_scans;
  oa.cap = (int32_t)cap;
  oa.inv_leaf = 1.0f / prm.less_flat_filter_size;
  oa.vox_stage = w.vox;
  oa.ring_out = w.ring_out;
  oa.host = out;
  oa.hdr = hdr;
  hipLaunchKernelGGL(fx_ring_voxel_kernel, dim3((unsigned)n_scans + 3u), dim3(FX_BLOCK), 0, s, oa);
  hipLaunchKernelGGL(fx_lessflat_out_kernel, dim3((unsigned)n_scans), dim3(FX_BLOCK), 0, s, oa);
  return hipGetLastError();
}


// what the two entry points keep in their context between calls (lslam::ctx_slot); each blob is carved into the call's arrays
struct FxCache {  // extract_features_impl
  lslam::DevBuf<char> blob;
  lslam::PinBuf<float4> pin, pout;
};
struct MsCache {  // lslam_multiscan_register
  lslam::DevBuf<char> blob;
  lslam::PinBuf<float4> pin;
};

}  // namespace

extern "C" {
#ifdef LSLAM_FX_CLOCKS
int lslam_debug_fx_clocks(double out[16]) {
  unsigned long long h[8];
  if (hipMemcpyFromSymbol(h, HIP_SYMBOL(fx_clk), sizeof(h)) != hipSuccess) return -1;
  for (int i = 0; i < 8; ++i) out[i] = (double)h[i];
  if (hipMemcpyFromSymbol(h, HIP_SYMBOL(vx_clk), sizeof(h)) != hipSuccess) return -1;
  for (int i = 0; i < 8; ++i) out[8 + i] = (double)h[i];
  return 0;
}
#endif


void lslam_reg_default_params(lslam_reg_params *p) {
  if (!p) return;
  // RegistrationParams ctor defaults, ScanRegistration.h:49-57 / ScanRegistration.cpp:14-30
  p->n_feature_regions = 6;
  p->curvature_region = 5;
  p->max_corner_sharp = 2;
  p->max_surface_flat = 4;
  p->less_flat_filter_size = 0.2f;
  p->surface_curvature_threshold = 0.02f;
  const float deg = 0.5f;                              // blindDegreeThreshold
  const float rad = (float)(deg * M_PI / 180.0);       // deg2rad(float), util/math_utils.h:37
  p->blind_threshold = (float)std::cos((double)rad);
  p->reserved = 0;
}

static int extract_features_impl(lslam_ctx *ctx, const void *cloud, size_t n_points, size_t stride_bytes,
                                 size_t intensity_offset_bytes, const int32_t *scan_ranges, size_t n_scans,
                                 const lslam_reg_params *params, float *sharp, float *less_sharp, float *flat,
                                 float *less_flat, size_t counts[4], float *curvature_out, int8_t *picked_out,
                                 int8_t *label_out, lslam_fset *dev_out);
int lslam_extract_features_dev(lslam_ctx *ctx, const void *cloud, size_t n_points, size_t stride_bytes,
                               size_t intensity_offset_bytes, const int32_t *scan_ranges, size_t n_scans,
                               const lslam_reg_params *params, lslam_fset *out, size_t counts[4]) {
  if (!out) {
    lslam::set_error("no feature set to extract into");
    return LSLAM_ERR_INVALID;
  }
  size_t local[4];
  const int rc = extract_features_impl(ctx, cloud, n_points, stride_bytes, intensity_offset_bytes, scan_ranges, n_scans, params, nullptr,
                                       nullptr, nullptr, nullptr, counts ? counts : local, nullptr, nullptr, nullptr, out);
  if (rc != LSLAM_OK && ctx && lslam::ctx_alive(ctx)) (void)hipStreamSynchronize((hipStream_t)lslam_stream(ctx));
  return rc;
}
int lslam_extract_features(lslam_ctx *ctx, const void *cloud, size_t n_points, size_t stride_bytes,
                           size_t intensity_offset_bytes, const int32_t *scan_ranges, size_t n_scans,
                           const lslam_reg_params *params, float *sharp, float *less_sharp, float *flat,
                           float *less_flat, size_t counts[4], float *curvature_out, int8_t *picked_out,
                           int8_t *label_out) {
  const int rc = extract_features_impl(ctx, cloud, n_points, stride_bytes, intensity_offset_bytes, scan_ranges, n_scans, params, sharp,
                                       less_sharp, flat, less_flat, counts, curvature_out, picked_out, label_out, nullptr);
  // a failure half way leaves copies out of / into the pinned staging in flight: the next call shares it
  if (rc != LSLAM_OK && ctx && lslam::ctx_alive(ctx)) (void)hipStreamSynchronize((hipStream_t)lslam_stream(ctx));
  return rc;
}
static int extract_features_impl(lslam_ctx *ctx, const void *cloud, size_t n_points, size_t stride_bytes,
                                 size_t intensity_offset_bytes, const int32_t *scan_ranges, size_t n_scans,
                                 const lslam_reg_params *params, float *sharp, float *less_sharp, float *flat,
                                 float *less_flat, size_t counts[4], float *curvature_out, int8_t *picked_out,
                                 int8_t *label_out, lslam_fset *dev_out) {
  if (!ctx || !lslam::ctx_alive(ctx) || !scan_ranges || !counts || (n_points && !cloud) || stride_bytes < 12 ||
      (stride_bytes & 3) || intensity_offset_bytes + 4 > stride_bytes || n_scans == 0 || n_scans > 4096) {
    lslam::set_error("bad feature-extraction arguments");
    return LSLAM_ERR_INVALID;
  }
  lslam_reg_params prm;
  if (params) prm = *params; else lslam_reg_default_params(&prm);
  if (prm.curvature_region < 1 || prm.curvature_region > 16 || prm.n_feature_regions < 1 || prm.n_feature_regions > 512) {  // (512: fx_ring_kernel's sort words)
    lslam::set_error("bad registration parameters");
    return LSLAM_ERR_INVALID;
  }
  for (int k = 0; k < 4; ++k) counts[k] = 0;
  if (dev_out) {
    if (dev_out->device != lslam::ctx_device(ctx)) {
      lslam::set_error("the feature set lives on another device");
      return LSLAM_ERR_INVALID;
    }
    for (int k = 0; k < 4; ++k) dev_out->counts[k] = 0;
  }
  for (size_t s = 0; s < n_scans; ++s) {
    const int32_t a = scan_ranges[2 * s], b = scan_ranges[2 * s + 1];
    if (b < a) continue;  // empty ring (MultiScanRegistration.cpp:184-189 gives {size, size - 1})
    if (a < 0 || (size_t)b >= n_points) {
      lslam::set_error("scan range outside the cloud");
      return LSLAM_ERR_INVALID;
    }
    if (b - a + 1 > MAXR) {
      lslam::set_error("a scan ring has more points than the kernel holds in LDS (2560)");
      return LSLAM_ERR_INVALID;
    }
  }
  if (n_points == 0) return LSLAM_OK;
  LSLAM_TRY(hipSetDevice(lslam::ctx_device(ctx)));
  hipStream_t s = (hipStream_t)lslam_stream(ctx);
  // device scratch and the pinned staging areas are the context's, kept between calls (a sweep arrives every 100 ms); the
  // outputs are WRITTEN to pinned memory by the kernels that make them: sixteen header slots (totals, error), then a slice of
  // n_points per list
  FxCache &cache = *lslam::ctx_slot<FxCache>(ctx, lslam::CTX_SLOT_FEATURES);
  const size_t np4 = n_points * sizeof(float4);
  LSLAM_TRY(cache.pin.reserve(n_points));
  LSLAM_TRY(cache.pout.reserve(4 * n_points + 16));
  // pack {x, y, z, intensity-to-copy} (toXYZI, util/pcl_util.h:30-37: the `curvature` field)
  float4 *h = cache.pin.p;
  const char *src = static_cast<const char *>(cloud);
  bool uploaded = false;
  if (stride_bytes == 16 && intensity_offset_bytes == 12) {
    // already {x, y, z, w}: copied to pinned memory and sent off a quarter at a time -- the link works on one quarter while
    // the host copies the next (the device arrays are carved further down; the upload target is the blob's head)
    uploaded = true;
  } else {
    for (size_t i = 0; i < n_points; ++i) {
      float v[3], w;
      std::memcpy(v, src + i * stride_bytes, 12);
      std::memcpy(&w, src + i * stride_bytes + intensity_offset_bytes, 4);
      h[i] = make_float4(v[0], v[1], v[2], w);
    }
  }
  LSLAM_TRY(cache.blob.reserve(fx_work_bytes(n_points, n_scans)));
  FxWork w;
  fx_carve(cache.blob.p, n_points, n_scans, w);
  float4 *d_pts = w.pts;
  int32_t *d_ranges = w.ranges;
  float *d_curv = w.curv;
  int8_t *d_picked = w.picked, *d_label = w.label;
  int rc = LSLAM_OK;
  auto fail = [&](int code) { return code; };
#define FX_TRY2(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { lslam::set_error(hipGetErrorString(_e)); return fail(LSLAM_ERR_HIP); } } while (0)
  if (uploaded) {
    const size_t quarter = (n_points + 3) / 4;
    for (size_t b = 0; b < n_points; b += quarter) {
      const size_t cnt = std::min(quarter, n_points - b);
      std::memcpy(h + b, src + b * sizeof(float4), cnt * sizeof(float4));
      FX_TRY2(hipMemcpyAsync(d_pts + b, h + b, cnt * sizeof(float4), hipMemcpyHostToDevice, s));
    }
  } else {
    FX_TRY2(hipMemcpyAsync(d_pts, h, np4, hipMemcpyHostToDevice, s));
  }
  FX_TRY2(hipMemcpyAsync(d_ranges, scan_ranges, 2 * n_scans * 4, hipMemcpyHostToDevice, s));
  // the four lists, on the device to the end (see fx_lists_block): nothing waits until everything is in pinned memory
  uint32_t *hdr = reinterpret_cast<uint32_t *>(cache.pout.p);
  for (int k = 0; k < 8; ++k) hdr[k] = 0u;
  if (dev_out) {  // ... or in the feature set's slices in HBM: only the eight header words come back
    FX_TRY2(lslam::fset_reserve(dev_out, n_points));
    FX_TRY2(hipMemsetAsync(dev_out->buf.p, 0, 8 * sizeof(uint32_t), s));
  }
  FX_TRY2(fx_enqueue(s, prm, w, n_points, n_scans, curvature_out != nullptr, picked_out != nullptr, label_out != nullptr,
                     dev_out ? dev_out->buf.p : cache.pout.p, dev_out ? reinterpret_cast<uint32_t *>(dev_out->buf.p) : hdr,
                     dev_out ? dev_out->cap : n_points));
  if (curvature_out) FX_TRY2(hipMemcpyAsync(curvature_out, d_curv, n_points * 4, hipMemcpyDeviceToHost, s));
  if (picked_out) FX_TRY2(hipMemcpyAsync(picked_out, d_picked, n_points, hipMemcpyDeviceToHost, s));
  if (label_out) FX_TRY2(hipMemcpyAsync(label_out, d_label, n_points, hipMemcpyDeviceToHost, s));
  if (dev_out) FX_TRY2(hipMemcpyAsync(hdr, dev_out->buf.p, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  FX_TRY2(hipStreamSynchronize(s));
  if (hdr[4]) {
    lslam::set_error(hdr[4] == 1u ? "voxel index outside its range (non-finite point?)" : "a feature list overflowed its staging slice");
    return fail(LSLAM_ERR_INVALID);
  }
  float *outs[4] = {sharp, less_sharp, flat, less_flat};
  for (int k = 0; k < 4; ++k) {
    counts[k] = (size_t)hdr[k];
    if (dev_out) dev_out->counts[k] = counts[k];
    if (!dev_out && outs[k] && hdr[k]) std::memcpy(outs[k], cache.pout.p + 16 + (size_t)k * n_points, (size_t)hdr[k] * sizeof(float4));
  }
  return rc;
}


int lslam_multiscan_register(lslam_ctx *ctx, const void *cloud, size_t n_points, size_t stride_bytes, float lower_deg,
                             float upper_deg, int32_t n_rings, float scan_period, float *out_xyzc, size_t cap,
                             size_t *n_out, int32_t *ranges_out) {
  if (!ctx || !lslam::ctx_alive(ctx) || !n_out || !ranges_out || (n_points && !cloud) || stride_bytes < 12 ||
      (stride_bytes & 3) || n_rings <= 0 || n_rings > 4096 || !(upper_deg > lower_deg) || n_points > 0x3FFFFFFFu) {
    lslam::set_error("bad multi-scan registration arguments");
    return LSLAM_ERR_INVALID;
  }
  *n_out = 0;
  for (int r = 0; r < n_rings; ++r) { ranges_out[2 * r] = 0; ranges_out[2 * r + 1] = 0; }
  if (n_points == 0) return LSLAM_OK;
  LSLAM_TRY(hipSetDevice(lslam::ctx_device(ctx)));
  hipStream_t s = (hipStream_t)lslam_stream(ctx);
  MsCache &cache = *lslam::ctx_slot<MsCache>(ctx, lslam::CTX_SLOT_MULTISCAN);
  const size_t np4 = n_points * sizeof(float4);
  LSLAM_TRY(cache.pin.reserve(n_points));
  float4 *h = cache.pin.p;
  const char *src = static_cast<const char *>(cloud);
  for (size_t i = 0; i < n_points; ++i) {
    float v[3];
    std::memcpy(v, src + i * stride_bytes, 12);
    h[i] = make_float4(v[0], v[1], v[2], 0.0f);
  }
  // sweep start / end orientation (:101-109), on the host with the C library the reference uses
  float start_ori = -std::atan2(h[0].y, h[0].x);
  float end_ori = -std::atan2(h[n_points - 1].y, h[n_points - 1].x) + 2 * float(M_PI);
  if (end_ori - start_ori > 3 * M_PI) end_ori -= 2 * M_PI;
  else if (end_ori - start_ori < M_PI) end_ori += 2 * M_PI;
  const size_t bytes = 3 * np4 + 4 * n_points * 4 + 64;
  LSLAM_TRY(cache.blob.reserve(bytes));
  char *blob = cache.blob.p;
  float4 *d_in = (float4 *)blob, *d_tmp = d_in + n_points, *d_out = d_tmp + n_points;
  int32_t *d_ring = (int32_t *)(d_out + n_points), *d_seg = d_ring + n_points;
  float *d_ori = (float *)(d_seg + n_points);
  int32_t *d_first = (int32_t *)(d_ori + n_points);
  auto fail = [&](int code) { return code; };
  const int32_t big = INT32_MAX;
  FX_TRY2(hipMemcpyAsync(d_in, h, np4, hipMemcpyHostToDevice, s));
  FX_TRY2(hipMemcpyAsync(d_first, &big, 4, hipMemcpyHostToDevice, s));
  MsArgs a{};
  a.in = d_in;
  a.n = (int)n_points;
  a.n_rings = n_rings;
  a.lower = lower_deg;
  a.factor = (n_rings - 1) / (upper_deg - lower_deg);  // MultiScanRegistration.h:63
  a.scan_period = scan_period;
  a.start_ori = start_ori;
  a.end_ori = end_ori;
  a.out = d_tmp;
  a.ring = d_ring;
  a.ori_raw = d_ori;
  a.first_half = d_first;
  const dim3 grd((unsigned)((n_points + 255) / 256)), blk(256);
  hipLaunchKernelGGL(ms_prep_kernel, grd, blk, 0, s, a);
  hipLaunchKernelGGL(ms_final_kernel, grd, blk, 0, s, a);
  size_t m = 0;  // per-ring clouds in arrival order (:178-190): a stable grouping by ring
  int rc = lslam::voxel_filter_segments(ctx, d_tmp, d_ring, n_points, n_rings, 1.0f, d_out, d_seg, &m, false);
  if (rc) return fail(rc);
  if (m > cap && out_xyzc) {
    lslam::set_error("registration output buffer too small");
    return fail(LSLAM_ERR_INVALID);
  }
  std::vector<int32_t> seg(m);
  if (m) {
    if (out_xyzc) FX_TRY2(hipMemcpyAsync(out_xyzc, d_out, m * sizeof(float4), hipMemcpyDeviceToHost, s));
    FX_TRY2(hipMemcpyAsync(seg.data(), d_seg, m * 4, hipMemcpyDeviceToHost, s));
    FX_TRY2(hipStreamSynchronize(s));
  }
  std::vector<size_t> count((size_t)n_rings, 0);
  for (size_t i = 0; i < m; ++i) count[(size_t)seg[i]]++;
  size_t total = 0;
  for (int r = 0; r < n_rings; ++r) {  // IndexRange(first, last), :184-189
    ranges_out[2 * r] = (int32_t)total;
    total += count[(size_t)r];
    ranges_out[2 * r + 1] = total > 0 ? (int32_t)total - 1 : 0;
  }
  *n_out = m;
  return LSLAM_OK;
}

// ---- the registration node resident on the device (include/lslam_c.h lslam_sreg_*) ---------------------------------------
}  // extern "C"

namespace {
struct SrImu {  // an IMUState on the host; the Angles with the sin / cos they cached when they were made (Angle(float))
  int64_t stamp = 0;
  float roll = 0.f, pitch = 0.f, yaw = 0.f;
  float sr = 0.f, cr = 1.f, sp = 0.f, cp = 1.f, sy = 0.f, cy = 1.f;
  float pos[3] = {0.f, 0.f, 0.f}, vel[3] = {0.f, 0.f, 0.f};
};
// ros::Duration::toSec() of an exact nanosecond difference: sec + 1e-9 * nsec with 0 <= nsec < 1e9
double sr_to_sec(int64_t d) {
  int64_t sec = d / 1000000000ll, nsec = d % 1000000000ll;
  if (nsec < 0) { nsec += 1000000000ll; sec -= 1; }
  return (double)sec + 1e-9 * (double)nsec;
}
void sr_rot_h(float c, float s, float &u, float &v) {
  const float u0 = u;
  u = c * u0 - s * v;
  v = s * u0 + c * v;
}
void sr_set_angles(SrImu &st, float roll, float pitch, float yaw) {  // three Angle(float)
  st.roll = roll; st.pitch = pitch; st.yaw = yaw;
  st.sr = std::sin(roll); st.cr = std::cos(roll);
  st.sp = std::sin(pitch); st.cp = std::cos(pitch);
  st.sy = std::sin(yaw); st.cy = std::cos(yaw);
}
void sr_rotate_yxz_neg(const SrImu &st, float v[3]) {  // rotateYXZ(v, -yaw, -pitch, -roll)
  sr_rot_h(st.cy, -st.sy, v[2], v[0]);
  sr_rot_h(st.cp, -st.sp, v[1], v[2]);
  sr_rot_h(st.cr, -st.sr, v[0], v[1]);
}
size_t sr_up16(size_t b) { return (b + 15) & ~(size_t)15; }

// _imuHistory (CircularBuffer.h) with handleIMUMessage and interpolateIMUStateFor(0): host arithmetic on the history alone,
// held by both registration nodes (lslam_sreg, lslam_oreg)
struct SrImuHistory {
  std::vector<SrImu> hist;  // `size` states from `first` on, the oldest overwritten when full
  size_t first = 0, size = 0;
  const SrImu &at(size_t k) const { return hist[(first + k) % hist.size()]; }
  void clear() { first = size = 0; }
  bool later_than_last(int64_t stamp_ns) const { return !size || stamp_ns > at(size - 1).stamp; }
  // handleIMUMessage, ScanRegistration.cpp:96-117 (the stamp is later than the last state's: the caller has checked)
  void push(int64_t stamp_ns, double roll, double pitch, double yaw, const double *la) {
    float acc[3];
    acc[0] = float(la[1] - std::sin(roll) * std::cos(pitch) * 9.81);
    acc[1] = float(la[2] - std::cos(roll) * std::cos(pitch) * 9.81);
    acc[2] = float(la[0] + std::sin(pitch) * 9.81);
    SrImu st;
    st.stamp = stamp_ns;
    sr_set_angles(st, (float)roll, (float)pitch, (float)yaw);
    if (size) {
      sr_rot_h(st.cr, st.sr, acc[0], acc[1]);  // rotateZXY(acc, roll, pitch, yaw)
      sr_rot_h(st.cp, st.sp, acc[1], acc[2]);
      sr_rot_h(st.cy, st.sy, acc[2], acc[0]);
      const SrImu &prev = at(size - 1);
      const float dt = float(sr_to_sec(stamp_ns - prev.stamp));
      for (int d = 0; d < 3; ++d) {
        st.pos[d] = (prev.pos[d] + prev.vel[d] * dt) + ((0.5f * acc[d]) * dt) * dt;
        st.vel[d] = prev.vel[d] + acc[d] * dt;
      }
    }
    const size_t cap = hist.size();
    if (size < cap) {
      hist[(first + size) % cap] = st;
      size++;
    } else {
      hist[first] = st;
      first = (first + 1) % cap;
    }
  }
  void info(int32_t *n, double last_position[3], double last_velocity[3]) const {
    if (n) *n = (int32_t)size;
    if (!size) return;
    const SrImu &l = at(size - 1);
    for (int d = 0; d < 3; ++d) {
      if (last_position) last_position[d] = (double)l.pos[d];
      if (last_velocity) last_velocity[d] = (double)l.vel[d];
    }
  }
  // reset(scanTime): _imuIdx = 0, interpolateIMUStateFor(0, _imuStart) -- on the host, as the reference does it (size > 0)
  SrImu start_for(int64_t scan_time_ns) const {
    size_t idx = 0;
    double time_diff = sr_to_sec(scan_time_ns - at(0).stamp) + 0.0f;
    while (idx < size - 1 && time_diff > 0) time_diff = sr_to_sec(scan_time_ns - at(++idx).stamp) + 0.0f;
    const SrImu &S = at(idx);
    if (idx == 0 || time_diff > 0) return S;
    SrImu start;
    const SrImu &E = at(idx - 1);
    const float ratio = -time_diff / sr_to_sec(S.stamp - E.stamp);
    const float inv = 1 - ratio;
    float yaw;
    if (S.yaw - E.yaw > M_PI) yaw = S.yaw * inv + (E.yaw + 2 * M_PI) * ratio;
    else if (S.yaw - E.yaw < -M_PI) yaw = S.yaw * inv + (E.yaw - 2 * M_PI) * ratio;
    else yaw = S.yaw * inv + E.yaw * ratio;
    sr_set_angles(start, S.roll * inv + E.roll * ratio, S.pitch * inv + E.pitch * ratio, yaw);
    for (int c = 0; c < 3; ++c) {
      start.vel[c] = S.vel[c] * inv + E.vel[c] * ratio;
      start.pos[c] = S.pos[c] * inv + E.pos[c] * ratio;
    }
    return start;
  }
};
}  // namespace

struct lslam_sreg {
  lslam_ctx *ctx = nullptr;
  int device = 0;
  hipStream_t stream = nullptr;
  lslam_reg_params prm;
  float lower = 0.f, upper = 0.f, scan_period = 0.1f;
  int32_t n_rings = 0;
  SrImuHistory imu;             // _imuHistory
  SrImu start, cur;             // _imuStart, _imuCur
  float shift[3] = {0.f, 0.f, 0.f};  // _imuPositionShift
  uint64_t sweeps = 0;
  // the last sweep's registered cloud, for lslam_sreg_cloud
  size_t last_m = 0;
  bool last_valid = false;
  float4 *d_sorted = nullptr;
  lslam::PinBuf<char> h_in;        // what a sweep uploads in one copy: control words, result words, ranges, ring counts, IMU states, cloud
  lslam::PinBuf<uint32_t> h_res;   // what comes back: SR_RES_WORDS, then the ranges
  lslam::PinBuf<uint32_t> done;    // the grouping's {points out, key-range error, -}
  lslam::DevBuf<char> d_in, d_work;
};

extern "C" {

int lslam_sreg_create(lslam_ctx *ctx, const lslam_reg_params *params, float lower_deg, float upper_deg, int32_t n_rings,
                      float scan_period, int32_t imu_history_size, lslam_sreg **out) {
  if (out) *out = nullptr;
  if (!ctx || !lslam::ctx_alive(ctx)) {
    lslam::set_error("lslam_sreg_create: null context, or it was destroyed");
    return LSLAM_ERR_INVALID;
  }
  lslam_reg_params prm;
  if (params) prm = *params; else lslam_reg_default_params(&prm);
  if (!out || n_rings <= 0 || n_rings > 4096 || !(upper_deg > lower_deg) || !(scan_period > 0.f) || imu_history_size < 1 ||
      imu_history_size > SR_MAX_HIST || prm.curvature_region < 1 || prm.curvature_region > 16 || prm.n_feature_regions < 1 ||
      prm.n_feature_regions > 512 || !(prm.less_flat_filter_size > 0.f)) {
    lslam::set_error("lslam_sreg_create: bad registration arguments (rings 1..4096, upper > lower, IMU history 1..512)");
    return LSLAM_ERR_INVALID;
  }
  lslam_sreg *sr = new lslam_sreg();
  sr->ctx = ctx;
  sr->device = lslam::ctx_device(ctx);
  sr->stream = (hipStream_t)lslam_stream(ctx);
  sr->prm = prm;
  sr->lower = lower_deg; sr->upper = upper_deg; sr->n_rings = n_rings; sr->scan_period = scan_period;
  sr->imu.hist.resize((size_t)imu_history_size);
  *out = sr;
  return LSLAM_OK;
}

void lslam_sreg_destroy(lslam_sreg *sr) {
  if (!sr) return;
  if (lslam::ctx_alive(sr->ctx)) {  // a node may outlive its context; the stream is then gone (and was waited for)
    (void)hipSetDevice(sr->device);
    (void)hipStreamSynchronize(sr->stream);
  }
  delete sr;
}

int lslam_sreg_imu_push(lslam_sreg *sr, int64_t stamp_ns, double roll, double pitch, double yaw, const double linear_acceleration[3]) {
  if (!sr) {
    lslam::set_error("lslam_sreg_imu_push: null node");
    return LSLAM_ERR_INVALID;
  }
  if (!linear_acceleration) {
    lslam::set_error("lslam_sreg_imu_push: no acceleration");
    return LSLAM_ERR_INVALID;
  }
  if (!sr->imu.later_than_last(stamp_ns)) {
    lslam::set_error("lslam_sreg_imu_push: the stamp is not later than the previous state's");
    return LSLAM_ERR_INVALID;
  }
  sr->imu.push(stamp_ns, roll, pitch, yaw, linear_acceleration);
  return LSLAM_OK;
}

int lslam_sreg_imu_info(const lslam_sreg *sr, int32_t *size, double last_position[3], double last_velocity[3]) {
  if (size) *size = 0;
  for (int d = 0; d < 3; ++d) {
    if (last_position) last_position[d] = 0.0;
    if (last_velocity) last_velocity[d] = 0.0;
  }
  if (!sr) {
    lslam::set_error("lslam_sreg_imu_info: null node");
    return LSLAM_ERR_INVALID;
  }
  sr->imu.info(size, last_position, last_velocity);
  return LSLAM_OK;
}

int lslam_sreg_imu_clear(lslam_sreg *sr) {
  if (!sr) {
    lslam::set_error("lslam_sreg_imu_clear: null node");
    return LSLAM_ERR_INVALID;
  }
  sr->imu.clear();
  sr->start = SrImu();
  sr->cur = SrImu();
  sr->shift[0] = sr->shift[1] = sr->shift[2] = 0.f;
  return LSLAM_OK;
}

int lslam_sreg_process(lslam_sreg *sr, const void *cloud, size_t n_points, size_t stride_bytes, int64_t scan_time_ns, lslam_fset *out,
                       size_t counts[4], float imu_trans[12], lslam_sreg_stats *stats) {
  if (counts) for (int k = 0; k < 4; ++k) counts[k] = 0;
  if (imu_trans) for (int k = 0; k < 12; ++k) imu_trans[k] = 0.f;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (!sr) {
    lslam::set_error("lslam_sreg_process: null node");
    return LSLAM_ERR_INVALID;
  }
  if (!lslam::ctx_alive(sr->ctx)) {
    lslam::set_error("lslam_sreg_process: the node's context was destroyed");
    return LSLAM_ERR_INVALID;
  }
  if (!out || out->device != sr->device) {
    lslam::set_error("lslam_sreg_process: no feature set, or it lives on another device");
    return LSLAM_ERR_INVALID;
  }
  for (int k = 0; k < 4; ++k) out->counts[k] = 0;
  if (!cloud || n_points == 0 || n_points > 0x3FFFFFFFu || stride_bytes < 12 || (stride_bytes & 3)) {
    lslam::set_error("lslam_sreg_process: empty cloud or bad stride");
    return LSLAM_ERR_INVALID;
  }
  LSLAM_TRY(hipSetDevice(sr->device));
  hipStream_t s = sr->stream;
  sr->last_valid = false;
  const size_t n = n_points, R = (size_t)sr->n_rings, K = sr->imu.size;
  const bool imu = K > 0;  // hasIMUData()
  // ---- what goes up, in one block: [SrCtl][result words][ranges][points per ring][IMU states][cloud] --------------------------
  const size_t o_res = sr_up16(sizeof(SrCtl)), o_ranges = o_res + SR_RES_WORDS * 4, o_hist = o_ranges + sr_up16(2 * R * 4),
               o_states = o_hist + sr_up16(R * 4), o_cloud = o_states + sr_up16(K * sizeof(SrState)),
               in_bytes = o_cloud + n * sizeof(float4);
  LSLAM_TRY(sr->h_in.reserve(in_bytes));
  LSLAM_TRY(sr->d_in.reserve(in_bytes));
  LSLAM_TRY(sr->h_res.reserve(SR_RES_WORDS + 2 * R));
  LSLAM_TRY(sr->done.reserve(4));
  char *hb = sr->h_in.p;
  std::memset(hb, 0, o_cloud);
  SrCtl *hctl = reinterpret_cast<SrCtl *>(hb);
  hctl->first_half = INT32_MAX;
  hctl->last_kept = -1;
  float4 *h = reinterpret_cast<float4 *>(hb + o_cloud);
  const char *src = static_cast<const char *>(cloud);
  if (stride_bytes == 16) {
    std::memcpy(h, src, n * sizeof(float4));  // (the fourth float is never read)
  } else {
    for (size_t i = 0; i < n; ++i) {
      float v[3];
      std::memcpy(v, src + i * stride_bytes, 12);
      h[i] = make_float4(v[0], v[1], v[2], 0.0f);
    }
  }
  // sweep start / end orientation (MultiScanRegistration.cpp:101-109), on the host with the C library the reference uses
  float start_ori = -std::atan2(h[0].y, h[0].x);
  float end_ori = -std::atan2(h[n - 1].y, h[n - 1].x) + 2 * float(M_PI);
  if (end_ori - start_ori > 3 * M_PI) end_ori -= 2 * M_PI;
  else if (end_ori - start_ori < M_PI) end_ori += 2 * M_PI;
  // ---- reset(scanTime): _imuIdx = 0, interpolateIMUStateFor(0, _imuStart) -- on the host, as the reference does it ---------
  SrImu start = sr->start;
  SrState dstart{};
  if (imu) {
    SrState *hs = reinterpret_cast<SrState *>(hb + o_states);
    for (size_t k = 0; k < K; ++k) {
      const SrImu &st = sr->imu.at(k);
      SrState &d = hs[k];
      d.tsec = sr_to_sec(scan_time_ns - st.stamp);
      d.dt_prev = k ? sr_to_sec(st.stamp - sr->imu.at(k - 1).stamp) : 0.0;
      d.roll = st.roll; d.pitch = st.pitch; d.yaw = st.yaw;
      d.sr = st.sr; d.cr = st.cr; d.sp = st.sp; d.cp = st.cp; d.sy = st.sy; d.cy = st.cy;
      for (int c = 0; c < 3; ++c) { d.pos[c] = st.pos[c]; d.vel[c] = st.vel[c]; }
    }
    start = sr->imu.start_for(scan_time_ns);
    dstart.roll = start.roll; dstart.pitch = start.pitch; dstart.yaw = start.yaw;
    dstart.sr = start.sr; dstart.cr = start.cr; dstart.sp = start.sp; dstart.cp = start.cp; dstart.sy = start.sy; dstart.cy = start.cy;
    for (int c = 0; c < 3; ++c) { dstart.pos[c] = start.pos[c]; dstart.vel[c] = start.vel[c]; }
  }
  // ---- device arrays -----------------------------------------------------------------------------------------------------
  const size_t nblk = (n + SR_BLOCK - 1) / SR_BLOCK;
  const size_t np4 = n * sizeof(float4);
  const size_t o_ring = sr_up16(np4), o_seg = o_ring + sr_up16(n * 4), o_ori = o_seg + sr_up16(n * 4), o_rel = o_ori + sr_up16(n * 4),
               o_bmax = o_rel + sr_up16(n * 4), o_fx = o_bmax + sr_up16(nblk * 4);
  LSLAM_TRY(sr->d_work.reserve(o_fx + fx_work_bytes(n, R)));
  char *wb = sr->d_work.p, *db = sr->d_in.p;
  float4 *d_tmp = (float4 *)wb;
  int32_t *d_ring = (int32_t *)(wb + o_ring), *d_seg = (int32_t *)(wb + o_seg);
  float *d_ori = (float *)(wb + o_ori), *d_rel = (float *)(wb + o_rel), *d_bmax = (float *)(wb + o_bmax);
  FxWork w;
  fx_carve(wb + o_fx, n, R, w);
  uint32_t *d_res = (uint32_t *)(db + o_res);
  int32_t *d_ranges_out = (int32_t *)(db + o_ranges), *d_hist = (int32_t *)(db + o_hist);
  LSLAM_TRY(lslam::fset_reserve(out, n));
  LSLAM_TRY(hipMemcpyAsync(db, hb, in_bytes, hipMemcpyHostToDevice, s));
  MsArgs a{};
  a.in = (const float4 *)(db + o_cloud);
  a.n = (int)n;
  a.n_rings = sr->n_rings;
  a.lower = sr->lower;
  a.factor = (sr->n_rings - 1) / (sr->upper - sr->lower);  // MultiScanRegistration.h:63
  a.scan_period = sr->scan_period;
  a.start_ori = start_ori;
  a.end_ori = end_ori;
  a.out = d_tmp;
  a.ring = d_ring;
  a.ori_raw = d_ori;
  a.first_half = &reinterpret_cast<SrCtl *>(db)->first_half;
  a.rel_out = imu ? d_rel : nullptr;
  const dim3 grd((unsigned)((n + 255) / 256)), blk(256);
  hipLaunchKernelGGL(ms_prep_kernel, grd, blk, 0, s, a);
  hipLaunchKernelGGL(ms_final_kernel, grd, blk, 0, s, a);
  SrArgs sa{};
  sa.pts = d_tmp;
  sa.ring = d_ring;
  sa.rel = imu ? d_rel : nullptr;
  sa.n = (int)n;
  sa.n_rings = sr->n_rings;
  sa.ctl = reinterpret_cast<SrCtl *>(db);
  sa.hist = d_hist;
  sa.bmax = d_bmax;
  sa.states = (const SrState *)(db + o_states);
  sa.n_states = (int)K;
  sa.start = dstart;
  sa.cur_out = reinterpret_cast<float *>(d_res + 16);
  hipLaunchKernelGGL(sr_stats_kernel, dim3((unsigned)nblk), dim3(SR_BLOCK), 0, s, sa);
  if (imu) hipLaunchKernelGGL(sr_deskew_kernel, dim3((unsigned)nblk), dim3(SR_BLOCK), 0, s, sa);
  // per-ring clouds in arrival order (:178-190): a stable grouping by ring; nothing is waited for
  sr->done.p[0] = sr->done.p[1] = sr->done.p[2] = 0;
  size_t m_unused = 0;
  int rc = lslam::voxel_filter_segments(sr->ctx, d_tmp, d_ring, n, sr->n_rings, 1.0f, w.pts, d_seg, &m_unused, false, sr->done.p);
  if (rc) {
    (void)hipStreamSynchronize(s);
    return rc;
  }
  hipLaunchKernelGGL(sr_ranges_kernel, dim3(1), dim3(FX_BLOCK), 0, s, d_hist, sr->n_rings, d_ranges_out, w.ranges, d_res);
  hipError_t e = fx_enqueue(s, sr->prm, w, n, R, false, false, false, out->buf.p, d_res, out->cap);
  if (e == hipSuccess) e = hipMemcpyAsync(sr->h_res.p, d_res, (SR_RES_WORDS + 2 * R) * 4, hipMemcpyDeviceToHost, s);
  const hipError_t e2 = hipStreamSynchronize(s);  // the node's one wait
  if (e != hipSuccess || e2 != hipSuccess) {
    lslam::set_error(hipGetErrorString(e != hipSuccess ? e : e2));
    return LSLAM_ERR_HIP;
  }
  const uint32_t *res = sr->h_res.p;
  if (res[4] || sr->done.p[1]) {
    lslam::set_error(res[4] == 3u ? "lslam_sreg_process: a scan ring has more points than the extraction holds in LDS (2560)"
                     : res[4] == 1u ? "voxel index outside its range (non-finite point?)"
                     : res[4] == 2u ? "a feature list overflowed its staging slice" : "the grouping by ring failed");
    return LSLAM_ERR_INVALID;
  }
  const size_t m = (size_t)res[28];
  for (int k = 0; k < 4; ++k) {
    out->counts[k] = (size_t)res[k];
    if (counts) counts[k] = (size_t)res[k];
  }
  sr->last_m = m;
  sr->last_valid = true;
  sr->d_sorted = w.pts;
  sr->sweeps++;
  if (imu) {
    sr->start = start;
    if (m) {  // (a sweep without a kept point leaves _imuCur and _imuPositionShift as they were)
      const float *c = reinterpret_cast<const float *>(res + 16);
      sr->cur.roll = c[0]; sr->cur.pitch = c[1]; sr->cur.yaw = c[2];
      for (int d = 0; d < 3; ++d) { sr->cur.pos[d] = c[3 + d]; sr->cur.vel[d] = c[6 + d]; sr->shift[d] = c[9 + d]; }
    }
  }
  if (imu_trans) {  // publishResult, ScanRegistration.cpp:684-707
    imu_trans[0] = sr->start.pitch; imu_trans[1] = sr->start.yaw; imu_trans[2] = sr->start.roll;
    imu_trans[3] = sr->cur.pitch; imu_trans[4] = sr->cur.yaw; imu_trans[5] = sr->cur.roll;
    float v[3] = {sr->shift[0], sr->shift[1], sr->shift[2]};
    sr_rotate_yxz_neg(sr->start, v);
    for (int d = 0; d < 3; ++d) imu_trans[6 + d] = v[d];
    for (int d = 0; d < 3; ++d) v[d] = sr->cur.vel[d] - sr->start.vel[d];
    sr_rotate_yxz_neg(sr->start, v);
    for (int d = 0; d < 3; ++d) imu_trans[9 + d] = v[d];
  }
  if (stats) {
    stats->sweeps = sr->sweeps;
    stats->n_points = m;
    stats->imu_states = (int32_t)K;
    stats->launches = imu ? 8 : 7;
    stats->bytes_up = in_bytes;
    stats->bytes_down = (SR_RES_WORDS + 2 * R) * 4 + 12;
  }
  return LSLAM_OK;
}

int lslam_sreg_cloud(lslam_sreg *sr, float *out_xyzc, size_t cap, size_t *n_out, int32_t *ranges_out) {
  if (n_out) *n_out = 0;
  if (!sr) {
    lslam::set_error("lslam_sreg_cloud: null node");
    return LSLAM_ERR_INVALID;
  }
  if (ranges_out) for (int r = 0; r < 2 * sr->n_rings; ++r) ranges_out[r] = 0;
  if (!n_out || !lslam::ctx_alive(sr->ctx)) {
    lslam::set_error("lslam_sreg_cloud: no place for the size, or the node's context was destroyed");
    return LSLAM_ERR_INVALID;
  }
  if (!sr->last_valid) {
    lslam::set_error("lslam_sreg_cloud: no sweep has been registered (or the last one was refused)");
    return LSLAM_ERR_INVALID;
  }
  *n_out = sr->last_m;
  if (ranges_out) std::memcpy(ranges_out, sr->h_res.p + SR_RES_WORDS, 2 * (size_t)sr->n_rings * 4);
  if (!out_xyzc || sr->last_m == 0) return LSLAM_OK;
  if (cap < sr->last_m) {
    lslam::set_error("lslam_sreg_cloud: output buffer too small");
    return LSLAM_ERR_INVALID;
  }
  LSLAM_TRY(hipSetDevice(sr->device));
  LSLAM_TRY(hipMemcpyAsync(out_xyzc, sr->d_sorted, sr->last_m * sizeof(float4), hipMemcpyDeviceToHost, sr->stream));
  LSLAM_TRY(hipStreamSynchronize(sr->stream));
  return LSLAM_OK;
}

}  // extern "C"

// ---- the registration node for organised clouds (include/lslam_c.h lslam_oreg_*) ---------------------------------------------
// OrganisedScanRegistration::process (odometry/OrganizedScanRegistration.cpp:82-150): the rows of the height x width image are
// visited in order and the columns in order, so "the per-row clouds concatenated" is a stable compaction of the row-major image:
// no grouping sort, no atan.  Per sweep: or_count_kernel (kept cells per tile of OR_TILE, kept cells per row), or_place_kernel
// (every workgroup sums the tiles before its own and writes {x, y, z, ring + relTime} where the extraction reads its cloud),
// sr_ranges_kernel with n_rings = height, then the extraction's three launches: six kernels.  The memsets of the extraction
// (its helpers' flags, when they are on) are not in that count.
namespace {
constexpr int OR_BLOCK = 256;
constexpr int OR_TILE = 1024;  // cells per workgroup, OR_TILE / OR_BLOCK rounds of one cell per thread
constexpr int OR_RES_WORDS = SR_RES_WORDS;  // the result words sr_ranges_kernel and the extraction write; the ranges follow them
struct OrArgs {
  const float4 *cells;  // row-major {x, y, z, word}: the ring in the low 16 bits of word
  const float *rel;     // [width] relTime of every column, made on the host
  int n, width;         // n = height * width
  float blind2;         // _blindRaduis * _blindRaduis
  int32_t *tile_count;  // [tiles] kept cells per tile
  int32_t *hist;        // [height] kept cells per row (zeroed by the upload)
  float4 *out;          // FxWork::pts
};
// :114-123: finite coordinates, then x*x + y*y + z*z < blind^2 drops the point (float, left to right, nothing contracted)
__device__ __forceinline__ bool or_kept(const float4 &c, float blind2) {
  const uint32_t e = 0x7f800000u;
  if ((__float_as_uint(c.x) & e) == e || (__float_as_uint(c.y) & e) == e || (__float_as_uint(c.z) & e) == e) return false;
  const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(c.x, c.x), __fmul_rn(c.y, c.y)), __fmul_rn(c.z, c.z));
  return !(d2 < blind2);
}

// Pass 1: kept cells per tile (ballot + popcount, the wavefronts' counts through LDS) and per row.  A tile touches at most
// OR_TILE rows (width 1); their counters sit in LDS and reach the global table with integer atomics, so the result does not
// depend on the order the atomics ran in.  A wavefront whose 64 cells lie in one row adds its popcount once.
__global__ __launch_bounds__(OR_BLOCK) void or_count_kernel(OrArgs a) {
  __shared__ int32_t h[OR_TILE];
  __shared__ int part[OR_BLOCK / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int base = blockIdx.x * OR_TILE, end = min(a.n, base + OR_TILE);
  const int row0 = base / a.width, rows = (end - 1) / a.width - row0 + 1;
  for (int r = tid; r < rows; r += OR_BLOCK) h[r] = 0;
  __syncthreads();
  int c = 0;
#pragma unroll
  for (int r = 0; r < OR_TILE / OR_BLOCK; ++r) {
    const int i = base + r * OR_BLOCK + tid;
    const bool in = i < end;
    const bool kept = in && or_kept(a.cells[i], a.blind2);
    const unsigned long long m = __ballot(kept);
    const int row = in ? i / a.width - row0 : -1;
    const int r_first = __shfl(row, 0, 64), r_last = __shfl(row, 63, 64);
    if (r_first == r_last) {  // (a ragged wavefront has row -1 in lane 63: the other branch)
      if (lane == 0 && m) atomicAdd(&h[r_first], __popcll(m));
    } else if (kept) {
      atomicAdd(&h[row], 1);
    }
    c += __popcll(m);
  }
  if (lane == 0) part[wave] = c;
  __syncthreads();
  if (tid == 0) {
    int t = 0;
#pragma unroll
    for (int w = 0; w < OR_BLOCK / 64; ++w) t += part[w];
    a.tile_count[blockIdx.x] = t;
  }
  for (int r = tid; r < rows; r += OR_BLOCK)
    if (h[r]) atomicAdd(&a.hist[row0 + r], h[r]);
}

// Pass 2: the tiles before this one summed by the workgroup itself (a few hundred words: no scan launch between the passes),
// then every kept cell placed in order -- ballot prefix inside a wavefront, the wavefronts' counts through LDS.  Validity is
// computed again, not stored; the point goes straight into the extraction's input array.
__global__ __launch_bounds__(OR_BLOCK) void or_place_kernel(OrArgs a) {
  __shared__ int part[OR_BLOCK / 64];
  __shared__ int wave_n[OR_BLOCK / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int before = 0;
  for (int b = tid; b < (int)blockIdx.x; b += OR_BLOCK) before += a.tile_count[b];
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) before += __shfl_xor(before, d, 64);
  if (lane == 0) part[wave] = before;
  __syncthreads();
  int offset = 0;
#pragma unroll
  for (int w = 0; w < OR_BLOCK / 64; ++w) offset += part[w];
  const int base = blockIdx.x * OR_TILE, end = min(a.n, base + OR_TILE);
  for (int r = 0; r < OR_TILE / OR_BLOCK; ++r) {
    const int i = base + r * OR_BLOCK + tid;
    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < end) c = a.cells[i];
    const bool kept = i < end && or_kept(c, a.blind2);
    const unsigned long long m = __ballot(kept);
    __syncthreads();  // (wave_n of the previous round has been read)
    if (lane == 0) wave_n[wave] = __popcll(m);
    __syncthreads();
    int w_before = 0, round_total = 0;
#pragma unroll
    for (int w = 0; w < OR_BLOCK / 64; ++w) {
      if (w < wave) w_before += wave_n[w];
      round_total += wave_n[w];
    }
    if (kept) {
      const int dst = offset + w_before + __popcll(m & ((1ull << lane) - 1ull));
      const int col = i % a.width;
      const uint32_t ring = __float_as_uint(c.w) & 0xFFFFu;  // p.ring, a uint16: int -> float, one float add (:112)
      if (dst < a.n) a.out[dst] = make_float4(c.x, c.y, c.z, __fadd_rn((float)ring, a.rel[col]));
    }
    offset += round_total;
  }
}
}  // namespace

struct lslam_oreg {
  lslam_ctx *ctx = nullptr;
  int device = 0;
  hipStream_t stream = nullptr;
  lslam_reg_params prm;
  float scan_period = 0.1f, blind_radius = 2.5f;
  SrImuHistory imu;             // _imuHistory; _imuCur and _imuPositionShift stay as constructed (process never sets them)
  SrImu start;                  // _imuStart
  uint64_t sweeps = 0;
  std::vector<float> rel;       // relTime of every column, for the width it was made for
  // the last sweep's registered cloud, for lslam_oreg_cloud
  size_t last_m = 0, last_h = 0;
  bool last_valid = false;
  float4 *d_sorted = nullptr;
  lslam::PinBuf<char> h_in;       // what a sweep uploads in one copy: result words, ranges, row counters, column times, cells
  lslam::PinBuf<uint32_t> h_res;  // what comes back: OR_RES_WORDS, then the ranges
  lslam::DevBuf<char> d_in, d_work;
};

extern "C" {

int lslam_oreg_create(lslam_ctx *ctx, const lslam_reg_params *params, float scan_period, float blind_radius, int32_t imu_history_size,
                      lslam_oreg **out) {
  if (out) *out = nullptr;
  if (!ctx || !lslam::ctx_alive(ctx)) {
    lslam::set_error("lslam_oreg_create: null context, or it was destroyed");
    return LSLAM_ERR_INVALID;
  }
  lslam_reg_params prm;
  if (params) prm = *params; else lslam_reg_default_params(&prm);
  if (!out || !(scan_period > 0.f) || !std::isfinite(scan_period) || !(blind_radius >= 0.f) || !std::isfinite(blind_radius) ||
      imu_history_size < 1 || imu_history_size > SR_MAX_HIST || prm.curvature_region < 1 || prm.curvature_region > 16 ||
      prm.n_feature_regions < 1 || prm.n_feature_regions > 512 || !(prm.less_flat_filter_size > 0.f)) {
    lslam::set_error("lslam_oreg_create: bad registration arguments (scan period > 0, finite blind radius >= 0, IMU history 1..512)");
    return LSLAM_ERR_INVALID;
  }
  lslam_oreg *og = new lslam_oreg();
  og->ctx = ctx;
  og->device = lslam::ctx_device(ctx);
  og->stream = (hipStream_t)lslam_stream(ctx);
  og->prm = prm;
  og->scan_period = scan_period;
  og->blind_radius = blind_radius;
  og->imu.hist.resize((size_t)imu_history_size);
  *out = og;
  return LSLAM_OK;
}

void lslam_oreg_destroy(lslam_oreg *og) {
  if (!og) return;
  if (lslam::ctx_alive(og->ctx)) {  // a node may outlive its context; the stream is then gone (and was waited for)
    (void)hipSetDevice(og->device);
    (void)hipStreamSynchronize(og->stream);
  }
  delete og;
}

int lslam_oreg_imu_push(lslam_oreg *og, int64_t stamp_ns, double roll, double pitch, double yaw, const double linear_acceleration[3]) {
  if (!og) {
    lslam::set_error("lslam_oreg_imu_push: null node");
    return LSLAM_ERR_INVALID;
  }
  if (!linear_acceleration) {
    lslam::set_error("lslam_oreg_imu_push: no acceleration");
    return LSLAM_ERR_INVALID;
  }
  if (!og->imu.later_than_last(stamp_ns)) {
    lslam::set_error("lslam_oreg_imu_push: the stamp is not later than the previous state's");
    return LSLAM_ERR_INVALID;
  }
  og->imu.push(stamp_ns, roll, pitch, yaw, linear_acceleration);
  return LSLAM_OK;
}

int lslam_oreg_imu_info(const lslam_oreg *og, int32_t *size, double last_position[3], double last_velocity[3]) {
  if (size) *size = 0;
  for (int d = 0; d < 3; ++d) {
    if (last_position) last_position[d] = 0.0;
    if (last_velocity) last_velocity[d] = 0.0;
  }
  if (!og) {
    lslam::set_error("lslam_oreg_imu_info: null node");
    return LSLAM_ERR_INVALID;
  }
  og->imu.info(size, last_position, last_velocity);
  return LSLAM_OK;
}

int lslam_oreg_imu_clear(lslam_oreg *og) {
  if (!og) {
    lslam::set_error("lslam_oreg_imu_clear: null node");
    return LSLAM_ERR_INVALID;
  }
  og->imu.clear();
  og->start = SrImu();
  return LSLAM_OK;
}

int lslam_oreg_process(lslam_oreg *og, const void *cloud, size_t height, size_t width, size_t stride_bytes, size_t ring_offset_bytes,
                       int64_t scan_time_ns, lslam_fset *out, size_t counts[4], float imu_trans[12], lslam_oreg_stats *stats) {
  if (counts) for (int k = 0; k < 4; ++k) counts[k] = 0;
  if (imu_trans) for (int k = 0; k < 12; ++k) imu_trans[k] = 0.f;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (!og) {
    lslam::set_error("lslam_oreg_process: null node");
    return LSLAM_ERR_INVALID;
  }
  if (!lslam::ctx_alive(og->ctx)) {
    lslam::set_error("lslam_oreg_process: the node's context was destroyed");
    return LSLAM_ERR_INVALID;
  }
  if (!out || out->device != og->device) {
    lslam::set_error("lslam_oreg_process: no feature set, or it lives on another device");
    return LSLAM_ERR_INVALID;
  }
  for (int k = 0; k < 4; ++k) out->counts[k] = 0;
  if (!cloud) {
    lslam::set_error("lslam_oreg_process: null cloud");
    return LSLAM_ERR_INVALID;
  }
  if (height == 0 || width == 0 || height > 4096 || width > (size_t)0x3FFFFFFFu / height) {
    lslam::set_error("lslam_oreg_process: bad image size (height 1..4096, width >= 1, height * width <= 0x3FFFFFFF)");
    return LSLAM_ERR_INVALID;
  }
  if (stride_bytes < 12 || (stride_bytes & 3) || ring_offset_bytes > stride_bytes || ring_offset_bytes + 2 > stride_bytes) {
    lslam::set_error("lslam_oreg_process: bad stride or ring offset");
    return LSLAM_ERR_INVALID;
  }
  LSLAM_TRY(hipSetDevice(og->device));
  hipStream_t s = og->stream;
  const size_t H = height, W = width, n = H * W, K = og->imu.size;
  const size_t tiles = (n + OR_TILE - 1) / OR_TILE;
  og->last_valid = false;  // from here on the node's buffers may move and its scratch is written
  // ---- what goes up, in one block: [result words][ranges][kept cells per row][relTime per column][cells] -----------------------
  const size_t o_ranges = OR_RES_WORDS * 4, o_hist = o_ranges + sr_up16(2 * H * 4), o_rel = o_hist + sr_up16(H * 4),
               o_cloud = o_rel + sr_up16(W * 4), in_bytes = o_cloud + n * sizeof(float4);
  LSLAM_TRY(og->h_in.reserve(in_bytes));
  LSLAM_TRY(og->d_in.reserve(in_bytes));
  LSLAM_TRY(og->h_res.reserve(OR_RES_WORDS + 2 * H));
  LSLAM_TRY(og->d_work.reserve(sr_up16(tiles * 4) + fx_work_bytes(n, H)));
  LSLAM_TRY(lslam::fset_reserve(out, n));
  char *hb = og->h_in.p;
  std::memset(hb, 0, o_rel);
  if (og->rel.size() != W) {  // float relTime = scanPeriod * static_cast<double>(col) / width (:111), rounded once
    og->rel.resize(W);
    for (size_t c = 0; c < W; ++c) og->rel[c] = (float)(((double)og->scan_period * (double)c) / (double)W);
  }
  std::memcpy(hb + o_rel, og->rel.data(), W * 4);
  char *h = hb + o_cloud;
  const char *src = static_cast<const char *>(cloud);
  if (stride_bytes == 16 && ring_offset_bytes == 12) {
    std::memcpy(h, src, n * 16);  // (the upper half of the fourth word is never read)
  } else {
    for (size_t i = 0; i < n; ++i) {
      uint16_t ring;
      std::memcpy(&ring, src + i * stride_bytes + ring_offset_bytes, 2);
      const uint32_t word = ring;
      std::memcpy(h + i * 16, src + i * stride_bytes, 12);
      std::memcpy(h + i * 16 + 12, &word, 4);
    }
  }
  // ---- reset(scanTime): interpolateIMUStateFor(0, _imuStart), on the host; nothing of it reaches the device ------------------
  const bool imu = K > 0;
  SrImu start = og->start;
  if (imu) start = og->imu.start_for(scan_time_ns);
  // ---- device arrays -----------------------------------------------------------------------------------------------------
  char *db = og->d_in.p, *wb = og->d_work.p;
  FxWork w;
  fx_carve(wb + sr_up16(tiles * 4), n, H, w);
  uint32_t *d_res = (uint32_t *)db;
  int32_t *d_ranges_out = (int32_t *)(db + o_ranges);
  LSLAM_TRY(hipMemcpyAsync(db, hb, in_bytes, hipMemcpyHostToDevice, s));
  OrArgs a{};
  a.cells = (const float4 *)(db + o_cloud);
  a.rel = (const float *)(db + o_rel);
  a.n = (int)n;
  a.width = (int)W;
  a.blind2 = og->blind_radius * og->blind_radius;
  a.tile_count = (int32_t *)wb;
  a.hist = (int32_t *)(db + o_hist);
  a.out = w.pts;
  hipLaunchKernelGGL(or_count_kernel, dim3((unsigned)tiles), dim3(OR_BLOCK), 0, s, a);
  hipLaunchKernelGGL(or_place_kernel, dim3((unsigned)tiles), dim3(OR_BLOCK), 0, s, a);
  hipLaunchKernelGGL(sr_ranges_kernel, dim3(1), dim3(FX_BLOCK), 0, s, a.hist, (int)H, d_ranges_out, w.ranges, d_res);
  hipError_t e = fx_enqueue(s, og->prm, w, n, H, false, false, false, out->buf.p, d_res, out->cap);
  if (e == hipSuccess) e = hipMemcpyAsync(og->h_res.p, d_res, (OR_RES_WORDS + 2 * H) * 4, hipMemcpyDeviceToHost, s);
  const hipError_t e2 = hipStreamSynchronize(s);  // the node's one wait
  if (e != hipSuccess || e2 != hipSuccess) {
    lslam::set_error(hipGetErrorString(e != hipSuccess ? e : e2));
    return LSLAM_ERR_HIP;
  }
  const uint32_t *res = og->h_res.p;
  if (res[4]) {
    lslam::set_error(res[4] == 3u ? "lslam_oreg_process: a row keeps more points than the extraction holds in LDS (2560)"
                     : res[4] == 1u ? "lslam_oreg_process: voxel index outside its range"
                                    : "lslam_oreg_process: a feature list overflowed its staging slice");
    return LSLAM_ERR_INVALID;
  }
  const size_t m = (size_t)res[28];
  for (int k = 0; k < 4; ++k) {
    out->counts[k] = (size_t)res[k];
    if (counts) counts[k] = (size_t)res[k];
  }
  og->last_m = m;
  og->last_h = H;
  og->last_valid = true;
  og->d_sorted = w.pts;
  og->sweeps++;
  og->start = start;
  if (imu_trans && imu) {  // publishResult, ScanRegistration.cpp:684-707, with _imuCur and _imuPositionShift as constructed
    imu_trans[0] = start.pitch; imu_trans[1] = start.yaw; imu_trans[2] = start.roll;
    float v[3] = {0.f, 0.f, 0.f};
    sr_rotate_yxz_neg(start, v);
    for (int d = 0; d < 3; ++d) imu_trans[6 + d] = v[d];
    for (int d = 0; d < 3; ++d) v[d] = 0.f - start.vel[d];
    sr_rotate_yxz_neg(start, v);
    for (int d = 0; d < 3; ++d) imu_trans[9 + d] = v[d];
  }
  if (stats) {
    stats->sweeps = og->sweeps;
    stats->n_cells = n;
    stats->n_points = m;
    stats->imu_states = (int32_t)K;
    stats->launches = 6;
    stats->bytes_up = in_bytes;
    stats->bytes_down = (OR_RES_WORDS + 2 * H) * 4;
  }
  return LSLAM_OK;
}

int lslam_oreg_cloud(lslam_oreg *og, float *out_xyzc, size_t cap, size_t *n_out, int32_t *ranges_out) {
  if (n_out) *n_out = 0;
  if (!og) {
    lslam::set_error("lslam_oreg_cloud: null node");
    return LSLAM_ERR_INVALID;
  }
  if (!n_out || !lslam::ctx_alive(og->ctx)) {
    lslam::set_error("lslam_oreg_cloud: no place for the size, or the node's context was destroyed");
    return LSLAM_ERR_INVALID;
  }
  if (!og->last_valid) {
    lslam::set_error("lslam_oreg_cloud: no sweep has been registered (or the last one was refused on the device)");
    return LSLAM_ERR_INVALID;
  }
  *n_out = og->last_m;
  if (ranges_out) std::memcpy(ranges_out, og->h_res.p + OR_RES_WORDS, 2 * og->last_h * 4);
  if (!out_xyzc || og->last_m == 0) return LSLAM_OK;
  if (cap < og->last_m) {
    lslam::set_error("lslam_oreg_cloud: output buffer too small");
    return LSLAM_ERR_INVALID;
  }
  LSLAM_TRY(hipSetDevice(og->device));
  LSLAM_TRY(hipMemcpyAsync(out_xyzc, og->d_sorted, og->last_m * sizeof(float4), hipMemcpyDeviceToHost, og->stream));
  LSLAM_TRY(hipStreamSynchronize(og->stream));
  return LSLAM_OK;
}

}  // extern "C"
