// lslam_reloc_impl.hpp -- global re-localisation of the localisation node (lslam_reloc_*, include/lslam_c.h has the
// specification).  Included at the end of lslam_loc.hip: it works on struct lslam_loc and reuses prepare_scan / solve_scan.
//
// Coarse stage, all on the node's stream behind one host wait:
//   rl_meta / rl_pack     the filtered clouds, subsampled, back to back in one array (.w = feature type)
//   rl_score_kernel       one workgroup per (rotation, tile of RL_POS_TILE positions): the scan is rotated ONCE per workgroup
//                         into LDS, chunk by chunk (R p does not depend on the position, and ((r0 x + r1 y) + r2 z) + t adds t
//                         last, so sharing it is exact); a wavefront owns RL_POS_PER_WAVE positions, its lanes stride over the
//                         chunk, and every LDS read feeds that many independent table probes (the kernel is bound by the
//                         probes' latency); hits are counted with a ballot and popcount; lane k stores position k's score and
//                         adds it to the score histogram
//   rl_thresh_kernel      the score s* at which the top list is cut, from the histogram
//   rl_gather / rl_scan / rl_ties   everything above s* (few: atomics), then the first K hypotheses AT s* in index order (a
//                         per-tile count, an exclusive scan, an ordered compaction), so that the list is deterministic
//   rl_sort_kernel        bitonic sort of the <= 1024 keys ((INT_MAX - score) << 32 | index), one workgroup
// The occupancy sets: open addressing (linear probing) over packed 64-bit voxel keys, one table per type at a load of at most
// 1/2, a 64-bit finaliser as the hash (voxels packed along a line spread like any others), filled with global 64-bit CAS.
#pragma once

#include <chrono>

namespace {

constexpr int RL_BLOCK = 256;
constexpr int RL_WAVES = RL_BLOCK / 64;
constexpr int RL_POS_PER_WAVE = 8;
constexpr int RL_POS_TILE = LSLAM_RELOC_POS_TILE;
constexpr int RL_CHUNK = LSLAM_RELOC_CHUNK;  // 3 x 4 KB of LDS per workgroup: LDS never limits the waves per CU
constexpr int RL_SEL_TILE = 1024;            // hypotheses per workgroup of the selection passes (256 lanes x 4 in a row)
constexpr int RL_TOP_MAX = 1024;
constexpr int RL_OUT_HEAD = 8;               // rl_out: {n selected, s*, scored corner, scored surf, filtered corner, filtered surf, -, -}
constexpr int RL_OUT_INTS = RL_OUT_HEAD + 2 * RL_TOP_MAX;
constexpr unsigned long long RL_EMPTY = ~0ull;  // never a key: a key's bit 63 is clear
constexpr float RL_IDX_LIM = 1048576.0f;        // voxel indices live in [-2^20, 2^20): 21 bits per axis
static_assert(RL_POS_TILE == RL_WAVES * RL_POS_PER_WAVE, "a wavefront owns RL_POS_PER_WAVE positions of the tile");

struct RlOpts {
  float voxel, inv, nms_m, min_fraction;
  int max_points, top_m, max_cand, nms_rot, rounds;
  bool cyclic, apply;
};

struct RlScoreArgs {
  const float4 *scan;       // [scored corner | scored surf], .w = type
  const int32_t *meta;      // {scored corner, scored surf, filtered corner, filtered surf}
  const float *R;           // [n_rot][9]
  const float4 *pos;        // [n_pos], .w != 0: refused (the edge band)
  int32_t n_rot, n_pos;
  float inv;
  const unsigned long long *tab;
  uint32_t cap;             // slots per type, a power of two
  int32_t *scores;          // [n_rot * n_pos]
  uint32_t *hist;           // [score]
};

// floor(x * inv) per axis, packed; false: the point has no voxel (a non-finite or out-of-range index)
LSLAM_DEV bool rl_voxel_key(float x, float y, float z, float inv, unsigned long long &key) {
  const float fx = floorf(__fmul_rn(x, inv)), fy = floorf(__fmul_rn(y, inv)), fz = floorf(__fmul_rn(z, inv));
  const bool ok = fx >= -RL_IDX_LIM && fx < RL_IDX_LIM && fy >= -RL_IDX_LIM && fy < RL_IDX_LIM && fz >= -RL_IDX_LIM && fz < RL_IDX_LIM;
  const unsigned long long ix = ok ? (unsigned long long)((int)fx + 1048576) : 0ull;
  const unsigned long long iy = ok ? (unsigned long long)((int)fy + 1048576) : 0ull;
  const unsigned long long iz = ok ? (unsigned long long)((int)fz + 1048576) : 0ull;
  key = (ix << 42) | (iy << 21) | iz;
  return ok;
}
LSLAM_DEV uint32_t rl_hash(unsigned long long k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return (uint32_t)k;
}
// the slots after the first (rare at this load)
LSLAM_DEV bool rl_probe_rest(const unsigned long long *T, uint32_t mask, uint32_t h, unsigned long long key) {
  for (uint32_t n = 0; n < mask; ++n) {
    h = (h + 1u) & mask;
    const unsigned long long v = T[h];
    if (v == key) return true;
    if (v == RL_EMPTY) return false;
  }
  return false;
}
LSLAM_DEV bool rl_lookup(const unsigned long long *T, uint32_t mask, unsigned long long key) {
  const uint32_t h = rl_hash(key) & mask;
  const unsigned long long v = T[h];
  if (v == key) return true;
  if (v == RL_EMPTY) return false;
  return rl_probe_rest(T, mask, h, key);
}
LSLAM_DEV unsigned long long rl_sort_key(int score, int idx) {
  return ((unsigned long long)(uint32_t)(0x7fffffff - score) << 32) | (unsigned long long)(uint32_t)idx;
}

__global__ void rl_fill_kernel(unsigned long long *tab, size_t n, unsigned long long *cnt) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) tab[i] = RL_EMPTY;
  if (i < 2) cnt[i] = 0ull;
}

// pts: [corner | surf], n0 corner points of n
__global__ void rl_occ_build_kernel(const float4 *pts, int n0, int n, float inv, unsigned long long *tab, uint32_t cap, unsigned long long *cnt) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 p = pts[i];
  const int t = i >= n0 ? 1 : 0;
  unsigned long long key;
  if (!rl_voxel_key(p.x, p.y, p.z, inv, key)) return;
  unsigned long long *T = tab + (size_t)t * cap;
  const uint32_t mask = cap - 1u;
  uint32_t h = rl_hash(key) & mask;
  for (uint32_t k = 0; k < cap; ++k) {
    const unsigned long long prev = atomicCAS(T + h, RL_EMPTY, key);
    if (prev == RL_EMPTY) {
      atomicAdd(cnt + t, 1ull);
      return;
    }
    if (prev == key) return;
    h = (h + 1u) & mask;
  }
}

__global__ void rl_occupied_kernel(const float4 *q, int nq, float inv, const unsigned long long *T, uint32_t cap, uint8_t *out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nq) return;
  const float4 p = q[i];
  unsigned long long key;
  const bool ok = rl_voxel_key(p.x, p.y, p.z, inv, key);
  out[i] = ok && rl_lookup(T, cap - 1u, key) ? 1 : 0;
}

// counts: {first corner, corner points, first surf, surf points} of the filtered clouds
__global__ void rl_meta_kernel(const int32_t *counts, int cap_corner, int cap_surf, int max_points, int32_t *meta) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  for (int t = 0; t < 2; ++t) {
    const int n = max(0, min(counts[2 * t + 1], t ? cap_surf : cap_corner));  // (a filter never adds points)
    const int st = (max_points > 0 && n > max_points) ? (n + max_points - 1) / max_points : 1;
    meta[t] = (n + st - 1) / st;
    meta[2 + t] = n;
    meta[4 + t] = st;
  }
}
__global__ void rl_pack_kernel(const float4 *q0, const float4 *q1, const int32_t *counts, const int32_t *meta, int cap, float4 *out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int pc = meta[0], ps = meta[1];
  if (i >= cap || i >= pc + ps) return;
  float4 p = i < pc ? q0[counts[0] + i * meta[4]] : q1[counts[2] + (i - pc) * meta[5]];
  p.w = i < pc ? 0.0f : 1.0f;
  out[i] = p;
}

__global__ __launch_bounds__(RL_BLOCK) void rl_score_kernel(const RlScoreArgs a) {
  __shared__ float lx[RL_CHUNK], ly[RL_CHUNK], lz[RL_CHUNK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = blockIdx.y;
  const int pc = a.meta[0], P = pc + a.meta[1];
  float R[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = a.R[(size_t)r * 9 + k];
  const int j0 = blockIdx.x * RL_POS_TILE + wave * RL_POS_PER_WAVE;
  float tx[RL_POS_PER_WAVE], ty[RL_POS_PER_WAVE], tz[RL_POS_PER_WAVE];
  bool live[RL_POS_PER_WAVE], refused[RL_POS_PER_WAVE];
  int cnt[RL_POS_PER_WAVE];
  bool any_live = false;
#pragma unroll
  for (int k = 0; k < RL_POS_PER_WAVE; ++k) {
    const int j = j0 + k;
    const float4 t = j < a.n_pos ? a.pos[j] : make_float4(0.f, 0.f, 0.f, 1.f);
    tx[k] = t.x; ty[k] = t.y; tz[k] = t.z;
    refused[k] = t.w != 0.0f;
    live[k] = j < a.n_pos && !refused[k];
    any_live = any_live || live[k];
    cnt[k] = 0;
  }
  const uint32_t mask = a.cap - 1u;
  for (int base = 0; base < P; base += RL_CHUNK) {
    const int n = min(RL_CHUNK, P - base);
    __syncthreads();  // the chunk before has been read by every wavefront
    for (int i = tid; i < n; i += RL_BLOCK) {
      const float4 p = a.scan[base + i];
      lx[i] = __fadd_rn(__fadd_rn(__fmul_rn(R[0], p.x), __fmul_rn(R[1], p.y)), __fmul_rn(R[2], p.z));
      ly[i] = __fadd_rn(__fadd_rn(__fmul_rn(R[3], p.x), __fmul_rn(R[4], p.y)), __fmul_rn(R[5], p.z));
      lz[i] = __fadd_rn(__fadd_rn(__fmul_rn(R[6], p.x), __fmul_rn(R[7], p.y)), __fmul_rn(R[8], p.z));
    }
    __syncthreads();
    if (!any_live) continue;  // wavefront-uniform (the barriers above are still reached)
    for (int i0 = 0; i0 < n; i0 += 64) {
      const int i = i0 + lane;
      const bool on = i < n;
      const float rx = on ? lx[i] : 0.0f, ry = on ? ly[i] : 0.0f, rz = on ? lz[i] : 0.0f;
      const unsigned long long *T = a.tab + ((base + i) >= pc ? (size_t)a.cap : 0);
      // the first slot of all the positions' probes first: independent loads in flight together
      unsigned long long key[RL_POS_PER_WAVE], v[RL_POS_PER_WAVE];
      uint32_t h[RL_POS_PER_WAVE];
      bool ok[RL_POS_PER_WAVE];
#pragma unroll
      for (int k = 0; k < RL_POS_PER_WAVE; ++k) {
        ok[k] = rl_voxel_key(__fadd_rn(rx, tx[k]), __fadd_rn(ry, ty[k]), __fadd_rn(rz, tz[k]), a.inv, key[k]) && on && live[k];
        h[k] = ok[k] ? rl_hash(key[k]) & mask : 0u;
        v[k] = T[h[k]];
      }
#pragma unroll
      for (int k = 0; k < RL_POS_PER_WAVE; ++k) {
        bool hit = ok[k] && v[k] == key[k];
        if (ok[k] && !hit && v[k] != RL_EMPTY) hit = rl_probe_rest(T, mask, h[k], key[k]);
        cnt[k] += __popcll(__ballot(hit));
      }
    }
  }
  int mine = 0;
  bool mine_refused = false;
#pragma unroll
  for (int k = 0; k < RL_POS_PER_WAVE; ++k) {
    mine = lane == k ? cnt[k] : mine;
    mine_refused = lane == k ? refused[k] : mine_refused;
  }
  const int j = j0 + lane;
  if (lane < RL_POS_PER_WAVE && j < a.n_pos) {
    a.scores[(size_t)r * a.n_pos + j] = mine_refused ? -1 : mine;
    if (!mine_refused) atomicAdd(a.hist + mine, 1u);
  }
}

// sel: {s*, K = hypotheses to take at s*, length of the list, hypotheses above s*, slot counter of the gather}.  Fewer valid
// hypotheses than M: s* = -1, all of them are "above".
__global__ __launch_bounds__(1024) void rl_thresh_kernel(const uint32_t *hist, int nbins, int M, int32_t *sel) {
  __shared__ uint32_t sc[1024];
  __shared__ int found[3];
  const int tid = threadIdx.x;
  if (tid == 0) found[0] = 0;
  uint32_t acc = 0;  // hypotheses in the bins above this round's
  __syncthreads();
  for (int top = nbins - 1; top >= 0; top -= 1024) {
    const int b = top - tid;
    const uint32_t c = b >= 0 ? hist[b] : 0u;
    sc[tid] = c;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
      const uint32_t v = tid >= off ? sc[tid - off] : 0u;
      __syncthreads();
      sc[tid] += v;
      __syncthreads();
    }
    const uint32_t incl = acc + sc[tid], excl = incl - c;
    if (b >= 0 && incl >= (uint32_t)M && excl < (uint32_t)M) {
      found[0] = 1;
      found[1] = b;
      found[2] = (int)excl;
    }
    const uint32_t total = sc[1023];
    __syncthreads();
    if (found[0]) break;
    acc += total;
  }
  if (tid == 0) {
    if (found[0]) {
      sel[0] = found[1];
      sel[1] = M - found[2];
      sel[2] = M;
      sel[3] = found[2];
    } else {
      sel[0] = -1;
      sel[1] = 0;
      sel[2] = (int)acc;
      sel[3] = (int)acc;
    }
    sel[4] = 0;
  }
}

__global__ __launch_bounds__(256) void rl_gather_kernel(const int32_t *scores, int H, int32_t *sel, unsigned long long *keys, int32_t *blk) {
  __shared__ int wsum[4];
  const int tid = threadIdx.x;
  const int s = sel[0];
  const int base = blockIdx.x * RL_SEL_TILE + tid * 4;
  int ties = 0;
  for (int k = 0; k < 4; ++k) {
    const int i = base + k;
    if (i >= H) break;
    const int v = scores[i];
    if (v > s && v >= 0) {
      const int slot = atomicAdd(sel + 4, 1);
      if (slot < RL_TOP_MAX) keys[slot] = rl_sort_key(v, i);
    } else if (v == s) {
      ++ties;
    }
  }
  for (int off = 32; off > 0; off >>= 1) ties += __shfl_down(ties, off, 64);
  if ((tid & 63) == 0) wsum[tid >> 6] = ties;
  __syncthreads();
  if (tid == 0) blk[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// exclusive scan in place, one workgroup
__global__ __launch_bounds__(1024) void rl_scan_kernel(int32_t *blk, int nblk) {
  __shared__ int sc[1024];
  const int tid = threadIdx.x;
  const int per = (nblk + 1023) / 1024;
  const int lo = min(tid * per, nblk), hi = min(lo + per, nblk);
  int sum = 0;
  for (int i = lo; i < hi; ++i) sum += blk[i];
  sc[tid] = sum;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const int v = tid >= off ? sc[tid - off] : 0;
    __syncthreads();
    sc[tid] += v;
    __syncthreads();
  }
  int run = sc[tid] - sum;
  for (int i = lo; i < hi; ++i) {
    const int v = blk[i];
    blk[i] = run;
    run += v;
  }
}

// the first K hypotheses at s*, in index order, behind the ones above it
__global__ __launch_bounds__(256) void rl_ties_kernel(const int32_t *scores, int H, const int32_t *sel, const int32_t *blk, unsigned long long *keys) {
  __shared__ int sc[256];
  const int tid = threadIdx.x;
  const int K = sel[1], off0 = blk[blockIdx.x];
  if (K <= 0 || off0 >= K) return;  // workgroup-uniform
  const int s = sel[0], above = sel[3];
  const int base = blockIdx.x * RL_SEL_TILE + tid * 4;
  bool m[4];
  int c = 0;
  for (int k = 0; k < 4; ++k) {
    const int i = base + k;
    m[k] = i < H && scores[i] == s;
    c += m[k] ? 1 : 0;
  }
  sc[tid] = c;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const int v = tid >= off ? sc[tid - off] : 0;
    __syncthreads();
    sc[tid] += v;
    __syncthreads();
  }
  int rank = off0 + sc[tid] - c;
  for (int k = 0; k < 4; ++k)
    if (m[k]) {
      if (rank < K && above + rank < RL_TOP_MAX) keys[above + rank] = rl_sort_key(s, base + k);
      ++rank;
    }
}

__global__ __launch_bounds__(1024) void rl_sort_kernel(const unsigned long long *keys, const int32_t *sel, const int32_t *meta, int32_t *out) {
  __shared__ unsigned long long k[RL_TOP_MAX];
  const int tid = threadIdx.x;
  const int n = min(sel[2], RL_TOP_MAX);
  k[tid] = tid < n ? keys[tid] : ~0ull;
  __syncthreads();
  for (int size = 2; size <= RL_TOP_MAX; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      const int partner = tid ^ stride;
      if (partner > tid) {
        const bool up = (tid & size) == 0;
        const unsigned long long x = k[tid], y = k[partner];
        if ((x > y) == up) {
          k[tid] = y;
          k[partner] = x;
        }
      }
      __syncthreads();
    }
  out[RL_OUT_HEAD + tid] = tid < n ? (int32_t)(uint32_t)(k[tid] & 0xffffffffull) : -1;
  out[RL_OUT_HEAD + RL_TOP_MAX + tid] = tid < n ? 0x7fffffff - (int32_t)(uint32_t)(k[tid] >> 32) : -1;
  if (tid == 0) {
    out[0] = n;
    out[1] = sel[0];
    out[2] = meta[0];
    out[3] = meta[1];
    out[4] = meta[2];
    out[5] = meta[3];
    out[6] = out[7] = 0;
  }
}

struct RlHostSinCos {
  void operator()(float a, float &sn, float &cs) const { sn = std::sin(a); cs = std::cos(a); }
};

int rl_read_opts(const char *fn, const lslam_reloc_opts *o, RlOpts &r) {
  lslam_reloc_opts z;
  std::memset(&z, 0, sizeof(z));
  if (o) z = *o;
  if (!(z.voxel >= 0.0f) || !std::isfinite(z.voxel) || z.max_points < 0 || z.top_m < 0 || z.top_m > RL_TOP_MAX || z.max_candidates < 0 ||
      z.max_candidates > 64 || !(z.nms_m >= 0.0f) || z.refine_rounds < 0 || z.refine_rounds > 64 || !(z.min_fraction >= 0.0f))
    return invalid(fn, "an option is out of range (top_m <= 1024, max_candidates <= 64, nothing negative but nms_rot)");
  r.voxel = z.voxel == 0.0f ? 2.0f : z.voxel;
  r.inv = 1.0f / r.voxel;
  r.max_points = z.max_points;
  r.top_m = z.top_m ? z.top_m : 256;
  r.max_cand = z.max_candidates ? z.max_candidates : 8;
  r.nms_m = z.nms_m == 0.0f ? 2.0f : z.nms_m;
  r.nms_rot = z.nms_rot == 0 ? 2 : (z.nms_rot < 0 ? 0 : z.nms_rot);
  r.cyclic = z.rot_cyclic != 0;
  r.rounds = z.refine_rounds ? z.refine_rounds : 3;
  r.min_fraction = z.min_fraction == 0.0f ? 0.4f : z.min_fraction;
  r.apply = z.apply != 0;
  return LSLAM_OK;
}

int rl_check_node(lslam_loc *loc, const char *fn) {
  int rc = check_loc(loc, fn);
  if (rc) return rc;
  if (loc->pg.on) return invalid(fn, "the paged mode (lslam_pmap_open) is not supported: relocalise over a static map");
  if (!loc->have_map) return invalid(fn, "no map (lslam_loc_load / _set_map / _set_map_from_fmap)");
  return LSLAM_OK;
}

// the occupancy sets of the loaded map for this voxel edge: built when missing or stale (its own wait, once per map)
int rl_ensure_occ(lslam_loc *loc, float voxel) {
  if (loc->occ_epoch == loc->structure_builds && loc->occ_voxel == voxel && loc->occ_cap) return LSLAM_OK;
  hipStream_t s = loc->stream;
  const size_t n0 = loc->view.n[0], n = loc->view.n[0] + loc->view.n[1];
  if (n > ((size_t)1 << 30)) return invalid("relocalisation", "more than 2^30 map points");
  size_t cap = 1024;
  while (cap < 2 * std::max(n0, n - n0)) cap <<= 1;
  loc->occ_epoch = -1;
  LOC_TRY(loc->occ_tab.reserve(2 * cap));
  LOC_TRY(loc->occ_cnt.reserve(2));
  hipLaunchKernelGGL(rl_fill_kernel, dim3((unsigned)((2 * cap + 255) / 256)), dim3(256), 0, s, loc->occ_tab.p, 2 * cap, loc->occ_cnt.p);
  if (n)
    hipLaunchKernelGGL(rl_occ_build_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const float4 *)loc->tpts.p, (int)n0, (int)n,
                       1.0f / voxel, loc->occ_tab.p, (uint32_t)cap, loc->occ_cnt.p);
  LOC_TRY(hipGetLastError());
  unsigned long long cnt[2] = {0, 0};
  LOC_TRY(hipMemcpyAsync(cnt, loc->occ_cnt.p, sizeof(cnt), hipMemcpyDeviceToHost, s));
  LOC_TRY(hipStreamSynchronize(s));
  loc->occ_cap = cap;
  loc->occ_voxel = voxel;
  loc->occ_voxels[0] = (int64_t)cnt[0];
  loc->occ_voxels[1] = (int64_t)cnt[1];
  loc->occ_epoch = loc->structure_builds;
  loc->occ_builds++;
  return LSLAM_OK;
}

bool rl_at_edge(const lslam_loc *loc, const float pos[3]) {
  int g[3];
  cube_of(loc, pos, g);
  const int lim[3] = {loc->view.W, loc->view.H, loc->view.D};
  bool e = false;
  for (int d = 0; d < 3; ++d) e = e || g[d] < 3 || g[d] > lim[d] - 4;
  return e;
}

// Scan preparation, scoring and the device half of the selection: rl_out_pin holds the list when this returns.
int rl_coarse(lslam_loc *loc, const char *fn, const void *corner, size_t n_corner, const void *surf, size_t n_surf, size_t stride_bytes,
              const float *rot, size_t n_rot, const float *pos, size_t n_pos, const RlOpts &o, bool sync_filter, int64_t *skipped) {
  hipStream_t s = loc->stream;
  const size_t H = n_rot * n_pos;
  int rc = prepare_scan(loc, corner, n_corner, surf, n_surf, stride_bytes, false, sync_filter);
  if (rc) return rc;
  const bool two_runs = loc->scan_leaf[0] != loc->scan_leaf[1];
  const int cap_pts = (int)(n_corner + n_surf);
  const int nbins = cap_pts + 1;
  const int nblk = (int)((H + RL_SEL_TILE - 1) / RL_SEL_TILE);
  LOC_TRY(loc->rl_R_pin.reserve(n_rot * 9));
  LOC_TRY(loc->rl_pos_pin.reserve(n_pos));
  LOC_TRY(loc->rl_out_pin.reserve(RL_OUT_INTS));
  LOC_TRY(loc->rl_R.reserve(n_rot * 9));
  LOC_TRY(loc->rl_pos.reserve(n_pos));
  LOC_TRY(loc->rl_scan.reserve((size_t)cap_pts + 1));
  LOC_TRY(loc->rl_meta.reserve(8));
  LOC_TRY(loc->rl_scores.reserve(H));
  LOC_TRY(loc->rl_hist.reserve((size_t)nbins));
  LOC_TRY(loc->rl_blk.reserve((size_t)nblk));
  LOC_TRY(loc->rl_sel.reserve(8));
  LOC_TRY(loc->rl_keys.reserve(RL_TOP_MAX));
  LOC_TRY(loc->rl_out.reserve(RL_OUT_INTS));
  for (size_t r = 0; r < n_rot; ++r) {
    const float tw[6] = {rot[3 * r], rot[3 * r + 1], rot[3 * r + 2], 0.0f, 0.0f, 0.0f};
    float t[3], sc[6];
    pose_to_Rt_sc(tw, loc->rl_R_pin.p + 9 * r, t, sc, RlHostSinCos());
  }
  int64_t refused = 0;
  for (size_t j = 0; j < n_pos; ++j) {
    const float p[3] = {pos[3 * j], pos[3 * j + 1], pos[3 * j + 2]};
    const bool e = rl_at_edge(loc, p);
    refused += e ? 1 : 0;
    loc->rl_pos_pin.p[j] = make_float4(p[0], p[1], p[2], e ? 1.0f : 0.0f);
  }
  *skipped = refused * (int64_t)n_rot;
  LOC_TRY(hipMemcpyAsync(loc->rl_R.p, loc->rl_R_pin.p, n_rot * 9 * sizeof(float), hipMemcpyHostToDevice, s));
  LOC_TRY(hipMemcpyAsync(loc->rl_pos.p, loc->rl_pos_pin.p, n_pos * sizeof(float4), hipMemcpyHostToDevice, s));
  LOC_TRY(hipMemsetAsync(loc->rl_hist.p, 0, (size_t)nbins * sizeof(uint32_t), s));
  LOC_TRY(hipMemsetAsync(loc->rl_meta.p, 0, 8 * sizeof(int32_t), s));
  hipLaunchKernelGGL(rl_meta_kernel, dim3(1), dim3(64), 0, s, (const int32_t *)loc->counts.p, (int)n_corner, (int)n_surf, o.max_points,
                     loc->rl_meta.p);
  if (cap_pts > 0)
    hipLaunchKernelGGL(rl_pack_kernel, dim3((unsigned)((cap_pts + 255) / 256)), dim3(256), 0, s, (const float4 *)loc->out_pts[0].p,
                       (const float4 *)loc->out_pts[two_runs ? 1 : 0].p, (const int32_t *)loc->counts.p, (const int32_t *)loc->rl_meta.p, cap_pts,
                       loc->rl_scan.p);
  RlScoreArgs a{};
  a.scan = loc->rl_scan.p;
  a.meta = loc->rl_meta.p;
  a.R = loc->rl_R.p;
  a.pos = loc->rl_pos.p;
  a.n_rot = (int32_t)n_rot;
  a.n_pos = (int32_t)n_pos;
  a.inv = o.inv;
  a.tab = loc->occ_tab.p;
  a.cap = (uint32_t)loc->occ_cap;
  a.scores = loc->rl_scores.p;
  a.hist = loc->rl_hist.p;
  hipLaunchKernelGGL(rl_score_kernel, dim3((unsigned)((n_pos + RL_POS_TILE - 1) / RL_POS_TILE), (unsigned)n_rot), dim3(RL_BLOCK), 0, s, a);
  hipLaunchKernelGGL(rl_thresh_kernel, dim3(1), dim3(1024), 0, s, (const uint32_t *)loc->rl_hist.p, nbins, o.top_m, loc->rl_sel.p);
  hipLaunchKernelGGL(rl_gather_kernel, dim3((unsigned)nblk), dim3(256), 0, s, (const int32_t *)loc->rl_scores.p, (int)H, loc->rl_sel.p,
                     loc->rl_keys.p, loc->rl_blk.p);
  hipLaunchKernelGGL(rl_scan_kernel, dim3(1), dim3(1024), 0, s, loc->rl_blk.p, nblk);
  hipLaunchKernelGGL(rl_ties_kernel, dim3((unsigned)nblk), dim3(256), 0, s, (const int32_t *)loc->rl_scores.p, (int)H,
                     (const int32_t *)loc->rl_sel.p, (const int32_t *)loc->rl_blk.p, loc->rl_keys.p);
  hipLaunchKernelGGL(rl_sort_kernel, dim3(1), dim3(1024), 0, s, (const unsigned long long *)loc->rl_keys.p, (const int32_t *)loc->rl_sel.p,
                     (const int32_t *)loc->rl_meta.p, loc->rl_out.p);
  LOC_TRY(hipGetLastError());
  LOC_TRY(hipMemcpyAsync(loc->rl_out_pin.p, loc->rl_out.p, RL_OUT_INTS * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  LOC_TRY(hipStreamSynchronize(s));  // the coarse stage's one wait
  if (!sync_filter && scan_filter_overflowed(loc))  // the scan filter's key range did not hold: once more, the filter measuring it
    return rl_coarse(loc, fn, corner, n_corner, surf, n_surf, stride_bytes, rot, n_rot, pos, n_pos, o, true, skipped);
  return LSLAM_OK;
}

// greedy NMS over the list, in its order -> positions in the list of the survivors, at most max_cand
int rl_nms(const int32_t *top_idx, int n_top, const float *pos, size_t n_rot, size_t n_pos, const RlOpts &o, int32_t *keep) {
  int nk = 0;
  for (int i = 0; i < n_top && nk < o.max_cand; ++i) {
    const int64_t h = top_idx[i];
    const int r = (int)(h / (int64_t)n_pos);
    const float *p = pos + 3 * (size_t)(h % (int64_t)n_pos);
    bool dropped = false;
    for (int k = 0; k < nk && !dropped; ++k) {
      const int64_t hk = top_idx[keep[k]];
      const int rk = (int)(hk / (int64_t)n_pos);
      const float *pk = pos + 3 * (size_t)(hk % (int64_t)n_pos);
      const float d = std::max(std::fabs(p[0] - pk[0]), std::max(std::fabs(p[1] - pk[1]), std::fabs(p[2] - pk[2])));
      int dr = std::abs(r - rk);
      if (o.cyclic) dr = std::min(dr, (int)n_rot - dr);
      dropped = d <= o.nms_m && dr <= o.nms_rot;
    }
    if (!dropped) keep[nk++] = i;
  }
  return nk;
}

int rl_check_args(const char *fn, const void *corner, size_t n_corner, const void *surf, size_t n_surf, size_t stride_bytes, const float *rot,
                  size_t n_rot, const float *pos, size_t n_pos) {
  if ((n_corner && !corner) || (n_surf && !surf) || stride_bytes < 12 || (stride_bytes & 3) || !rot || !pos || n_rot == 0 || n_pos == 0)
    return invalid(fn, "bad arguments");
  if (n_rot > 4096 || n_pos > ((size_t)1 << 26) || n_rot * n_pos > ((size_t)1 << 26))
    return invalid(fn, "too many hypotheses (n_rot <= 4096, n_rot * n_pos <= 2^26)");
  if (n_corner + n_surf > ((size_t)1 << 27)) return invalid(fn, "too many scan points");
  return LSLAM_OK;
}

void rl_fill_coarse_result(const lslam_loc *loc, lslam_reloc_result *res, size_t H, int64_t skipped) {
  std::memset(res, 0, sizeof(*res));
  const int32_t *out = loc->rl_out_pin.p;
  res->winner = res->runner_up = -1;
  identity16(res->T);
  res->n_hypotheses = (int64_t)H;
  res->skipped = skipped;
  res->n_scored[0] = out[2];
  res->n_scored[1] = out[3];
  res->n_points[0] = out[4];
  res->n_points[1] = out[5];
  res->occupied_voxels[0] = loc->occ_voxels[0];
  res->occupied_voxels[1] = loc->occ_voxels[1];
  res->n_selected = out[0];
}

float rl_ms_since(const std::chrono::steady_clock::time_point &t0) {
  return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

extern "C" {

int lslam_reloc_relocalize(lslam_loc *loc, const void *corner, size_t n_corner, const void *surf, size_t n_surf, size_t stride_bytes,
                           const float *rot_xyz, size_t n_rot, const float *pos_xyz, size_t n_pos, const lslam_reloc_opts *opts,
                           lslam_reloc_result *result) {
  const char *fn = "lslam_reloc_relocalize";
  if (result) {
    std::memset(result, 0, sizeof(*result));
    result->winner = result->runner_up = -1;
  }
  int rc = rl_check_node(loc, fn);
  if (rc) return rc;
  if (!result) return invalid(fn, "null result");
  rc = rl_check_args(fn, corner, n_corner, surf, n_surf, stride_bytes, rot_xyz, n_rot, pos_xyz, n_pos);
  if (rc) return rc;
  RlOpts o;
  rc = rl_read_opts(fn, opts, o);
  if (rc) return rc;
  rc = rl_ensure_occ(loc, o.voxel);
  if (rc) return rc;
  auto t0 = std::chrono::steady_clock::now();
  int64_t skipped = 0;
  rc = rl_coarse(loc, fn, corner, n_corner, surf, n_surf, stride_bytes, rot_xyz, n_rot, pos_xyz, n_pos, o, false, &skipped);
  if (rc) {
    (void)hipStreamSynchronize(loc->stream);
    return rc;
  }
  rl_fill_coarse_result(loc, result, n_rot * n_pos, skipped);
  const int32_t *top_idx = loc->rl_out_pin.p + RL_OUT_HEAD, *top_score = top_idx + RL_TOP_MAX;
  int32_t keep[64];
  const int nc = rl_nms(top_idx, result->n_selected, pos_xyz, n_rot, n_pos, o, keep);
  result->n_candidates = nc;
  result->ms_coarse = rl_ms_since(t0);
  // ---- refinement: lslam_loc_match's solve over the scan prepared above, candidates in the order of their sensor cube ----
  t0 = std::chrono::steady_clock::now();
  int order[64];
  long long cube_key[64];
  for (int c = 0; c < nc; ++c) {
    lslam_reloc_candidate &cd = result->candidates[c];
    const int64_t h = top_idx[keep[c]];
    cd.hypothesis = (int32_t)h;
    cd.coarse_score = top_score[keep[c]];
    const size_t r = (size_t)(h / (int64_t)n_pos), j = (size_t)(h % (int64_t)n_pos);
    for (int d = 0; d < 3; ++d) {
      cd.pose[d] = rot_xyz[3 * r + d];
      cd.pose[3 + d] = pos_xyz[3 * j + d];
    }
    int g[3];
    cube_of(loc, cd.pose + 3, g);
    cube_key[c] = ((long long)g[2] * 1000003LL + g[1]) * 1000003LL + g[0];
    order[c] = c;
  }
  std::stable_sort(order, order + nc, [&](int x, int y) { return cube_key[x] < cube_key[y]; });
  const bool grid_was_valid = loc->grid_valid;
  const int64_t grid_builds = loc->grid_builds;
  const int grid_reach = loc->grid_reach;
  const int grid_cube[3] = {loc->grid_cube[0], loc->grid_cube[1], loc->grid_cube[2]};
  int err = 0;
  for (int k = 0; k < nc && !err; ++k) {
    lslam_reloc_candidate &cd = result->candidates[order[k]];
    cd.status = LSLAM_NOT_CONVERGED;
    while (cd.rounds < o.rounds && cd.status == LSLAM_NOT_CONVERGED) {
      lslam_stats st;
      bool refilter = false;
      begin_sweep_counts(loc);
      rc = solve_scan(loc, n_corner, n_surf, cd.pose, &st, &refilter);
      end_sweep_counts(loc);
      if (rc < 0 || refilter) {
        err = rc < 0 ? rc : LSLAM_ERR_INVALID;
        if (refilter) lslam::set_error("lslam_reloc_relocalize: the scan filter's key range changed under the refinement");
        break;
      }
      cd.rounds++;
      cd.status = rc;
      cd.n_rows = st.n_rows;
    }
  }
  // the node's grids and their counters as they were
  if (!err && grid_was_valid) {
    rc = ensure_grids(loc, grid_cube);
    if (rc) err = rc;
  } else {
    loc->grid_valid = false;
    for (int d = 0; d < 3; ++d) loc->grid_cube[d] = grid_cube[d];
    loc->grid_reach = grid_reach;
  }
  loc->grid_builds = grid_builds;
  if (err) {
    (void)hipStreamSynchronize(loc->stream);
    return err;
  }
  auto better = [&](int x, int y) {  // x before y: more rows, then the better coarse rank
    const lslam_reloc_candidate &a = result->candidates[x], &b = result->candidates[y];
    return a.n_rows != b.n_rows ? a.n_rows > b.n_rows : x < y;
  };
  int win = -1;
  for (int c = 0; c < nc; ++c)
    if (result->candidates[c].status == LSLAM_OK && (win < 0 || better(c, win))) win = c;
  result->winner = win;
  result->ms_refine = rl_ms_since(t0);
  if (win < 0) return LSLAM_NOT_CONVERGED;
  const lslam_reloc_candidate &w = result->candidates[win];
  int ru = -1;
  for (int c = 0; c < nc; ++c) {
    const lslam_reloc_candidate &cd = result->candidates[c];
    if (c == win || cd.status != LSLAM_OK) continue;
    const float d = std::max(std::fabs(cd.pose[3] - w.pose[3]), std::max(std::fabs(cd.pose[4] - w.pose[4]), std::fabs(cd.pose[5] - w.pose[5])));
    if (d > o.nms_m && (ru < 0 || better(c, ru))) ru = c;
  }
  result->runner_up = ru;
  lslam_pose_to_isometry(w.pose, result->T);
  const int denom = result->n_points[0] + result->n_points[1];
  result->fraction = denom > 0 ? (float)w.n_rows / (float)denom : 0.0f;
  if (!(result->fraction >= o.min_fraction)) return LSLAM_TOO_FEW_MATCHES;
  result->accepted = 1;
  if (o.apply) {  // lslam_loc_set_initial_pose(T)
    std::memcpy(loc->reset_pose, result->T, sizeof(loc->reset_pose));
    loc->reset_pending = true;
    loc->initialized = true;
  }
  return LSLAM_OK;
}

int lslam_reloc_scores(lslam_loc *loc, const void *corner, size_t n_corner, const void *surf, size_t n_surf, size_t stride_bytes,
                       const float *rot_xyz, size_t n_rot, const float *pos_xyz, size_t n_pos, const lslam_reloc_opts *opts,
                       int32_t *scores_out, int32_t *top_idx, int32_t *top_score, int32_t *n_top, lslam_reloc_result *result) {
  const char *fn = "lslam_reloc_scores";
  if (n_top) *n_top = 0;
  if (result) {
    std::memset(result, 0, sizeof(*result));
    result->winner = result->runner_up = -1;
  }
  int rc = rl_check_node(loc, fn);
  if (rc) return rc;
  if (!scores_out || (top_idx != nullptr) != (top_score != nullptr)) return invalid(fn, "bad arguments");
  rc = rl_check_args(fn, corner, n_corner, surf, n_surf, stride_bytes, rot_xyz, n_rot, pos_xyz, n_pos);
  if (rc) return rc;
  RlOpts o;
  rc = rl_read_opts(fn, opts, o);
  if (rc) return rc;
  rc = rl_ensure_occ(loc, o.voxel);
  if (rc) return rc;
  int64_t skipped = 0;
  rc = rl_coarse(loc, fn, corner, n_corner, surf, n_surf, stride_bytes, rot_xyz, n_rot, pos_xyz, n_pos, o, false, &skipped);
  if (rc) {
    (void)hipStreamSynchronize(loc->stream);
    return rc;
  }
  const size_t H = n_rot * n_pos;
  LOC_TRY(hipMemcpyAsync(scores_out, loc->rl_scores.p, H * sizeof(int32_t), hipMemcpyDeviceToHost, loc->stream));
  LOC_TRY(hipStreamSynchronize(loc->stream));
  const int32_t *out = loc->rl_out_pin.p;
  if (top_idx) {
    std::memcpy(top_idx, out + RL_OUT_HEAD, (size_t)out[0] * sizeof(int32_t));
    std::memcpy(top_score, out + RL_OUT_HEAD + RL_TOP_MAX, (size_t)out[0] * sizeof(int32_t));
  }
  if (n_top) *n_top = out[0];
  if (result) rl_fill_coarse_result(loc, result, H, skipped);
  return LSLAM_OK;
}

int lslam_reloc_nms(const int32_t *top_idx, int32_t n_top, const float *pos_xyz, size_t n_rot, size_t n_pos, const lslam_reloc_opts *opts,
                    int32_t *keep_out) {
  const char *fn = "lslam_reloc_nms";
  if (n_top < 0 || (n_top && !top_idx) || !pos_xyz || !keep_out || n_rot == 0 || n_pos == 0) return invalid(fn, "bad arguments");
  RlOpts o;
  int rc = rl_read_opts(fn, opts, o);
  if (rc) return rc;
  for (int i = 0; i < n_top; ++i)
    if (top_idx[i] < 0 || (size_t)top_idx[i] >= n_rot * n_pos) return invalid(fn, "a hypothesis index is out of range");
  return rl_nms(top_idx, n_top, pos_xyz, n_rot, n_pos, o, keep_out);
}

int lslam_reloc_occupied(lslam_loc *loc, int32_t which, float voxel, const void *queries, size_t nq, size_t stride_bytes, uint8_t *out) {
  const char *fn = "lslam_reloc_occupied";
  int rc = rl_check_node(loc, fn);
  if (rc) return rc;
  if ((which != 0 && which != 1) || (nq && (!queries || !out)) || stride_bytes < 12 || (stride_bytes & 3) || nq > ((size_t)1 << 26) ||
      !(voxel >= 0.0f) || !std::isfinite(voxel))
    return invalid(fn, "bad arguments");
  const float vx = voxel == 0.0f ? 2.0f : voxel;
  rc = rl_ensure_occ(loc, vx);
  if (rc) return rc;
  if (nq == 0) return LSLAM_OK;
  hipStream_t s = loc->stream;
  LOC_TRY(loc->rl_pos_pin.reserve(nq));
  LOC_TRY(loc->rl_pos.reserve(nq));
  const char *p = static_cast<const char *>(queries);
  for (size_t i = 0; i < nq; ++i) {
    float v[3];
    std::memcpy(v, p + i * stride_bytes, 12);
    loc->rl_pos_pin.p[i] = make_float4(v[0], v[1], v[2], 0.0f);
  }
  DevBuf<uint8_t> d_out;
  LOC_TRY(d_out.reserve(nq));
  LOC_TRY(hipMemcpyAsync(loc->rl_pos.p, loc->rl_pos_pin.p, nq * sizeof(float4), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(rl_occupied_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s, (const float4 *)loc->rl_pos.p, (int)nq, 1.0f / vx,
                     (const unsigned long long *)(loc->occ_tab.p + (which ? loc->occ_cap : 0)), (uint32_t)loc->occ_cap, d_out.p);
  LOC_TRY(hipGetLastError());
  LOC_TRY(hipMemcpyAsync(out, d_out.p, nq, hipMemcpyDeviceToHost, s));
  LOC_TRY(hipStreamSynchronize(s));
  return LSLAM_OK;
}

int lslam_reloc_info(lslam_loc *loc, lslam_reloc_map_stats *out) {
  if (out) std::memset(out, 0, sizeof(*out));
  int rc = check_loc(loc, "lslam_reloc_info");
  if (rc) return rc;
  if (!out) return invalid("lslam_reloc_info", "null output");
  const bool valid = loc->have_map && !loc->pg.on && loc->occ_cap && loc->occ_epoch == loc->structure_builds;
  out->occupied_voxels[0] = valid ? loc->occ_voxels[0] : 0;
  out->occupied_voxels[1] = valid ? loc->occ_voxels[1] : 0;
  out->table_slots = loc->occ_tab.cap;
  out->builds = loc->occ_builds;
  out->voxel = loc->occ_voxel;
  out->valid = valid ? 1 : 0;
  return LSLAM_OK;
}

}  // extern "C"
