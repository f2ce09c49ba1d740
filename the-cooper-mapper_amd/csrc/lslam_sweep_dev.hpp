// lslam_sweep_dev.hpp -- the per-point and per-block steps every sweep kernel shares: the cube of a point (variant C), the
// residual chain of a point whose five neighbours are known, and the block's normal-equation sums.  Used by the sweep kernels
// of lslam_kernels.hip and by the localisation node's (lslam_loc.hip).
#pragma once

#include "lslam_internal.hpp"
#include "lslam_odom_dev.hpp"

namespace lslam {

// ---------------------------------------------------------------------------
// J^T J by MFMA (jtj_mode 1): the wave's 64 rows [J | b] (7 of 16 columns used)
// are staged through LDS and contracted with v_mfma_f32_16x16x4_f32, 4 scan
// points per instruction, 16 instructions per wave.  For J^T J the A operand
// (16 x 4: A[i][k] = J[k][i]) and the B operand (4 x 16: B[k][j] = J[k][j]) hold
// the SAME value in lane l = 16*k + i, so one ds_read feeds both.  The MFMA is an
// exact fp32 fma chain in k order (no reduced precision).
// ---------------------------------------------------------------------------
using f32x4 = __attribute__((ext_vector_type(4))) float;

// worldToCube + isIndexValid + toIndex (util/FeatureMap.h:475-487,102-108,146-148)
// A coordinate that is not a number has no cube: the reference's (int) cast makes INT_MIN of it and isIndexValid fails, the
// device's conversion makes 0 -- a valid index.  (Infinite and huge values saturate and fail the range test by themselves.)
LSLAM_DEV int cube_tree_of(const CubeGridDev &g, float x, float y, float z) {
  if (!(x == x && y == y && z == z)) return -1;
  const int gi = (int)(roundf(x / g.cube_size) + (float)g.origin[0]);
  const int gj = (int)(roundf(y / g.cube_size) + (float)g.origin[1]);
  const int gk = (int)(roundf(z / g.cube_size) + (float)g.origin[2]);
  if (0 <= gi && gi < g.dims[0] && 0 <= gj && gj < g.dims[1] && 0 <= gk && gk < g.dims[2])
    return g.cell_tree[gi + gj * g.dims[0] + gk * g.dims[0] * g.dims[1]];
  return -1;
}

// ScanMatch.cpp:102-139 for one point whose five neighbours are known: the acceptance gate, findLine / findPlane on the five
// (fetched from P, the array the neighbour ids p[] index), the coefficient, the Jacobian row; the optional per-point taps.
// Shared by the tree sweep (P = the tree's permuted points) and the grid sweep (P = the cell-sorted points).
// GIVEN (the lean grid sweep): the search has the five points in registers already -- (*given)[3 j ..] = x, y, z of P[p[j]]
// when `use_given` (wave-uniform; knn5_grid<.., true>) -- and they are not gathered again (findLine / findPlane read x, y, z only).
// INR (the lean kernels): the in-range fit first, the fit as everybody has it only for a wavefront with an operand outside the range.
template <bool GIVEN = false, bool INR = false>
LSLAM_DEV void point_residual(const SweepArgs &a, const BlockDesc &bd, const bool is_surf, const float4 *P, const float4 &q,
                              const float (&sel)[3], const float (&d)[5], const int (&p)[5], const float (&sc)[6],
                              float (&row)[6], float &rb, float &kept, float &matched, float &score,
                              const float (*given)[15] = nullptr, const bool use_given = false) {
  float coeff[4] = {0, 0, 0, 0};
  unsigned flag = 0;
  float4 nb[5];
  // ScanMatch.cpp:102,120; the _fineScore re-sweep gates on the nearest neighbour instead (:282,302)
  const bool gate = a.fine_gate_c >= 0.0f ? d[0] < (is_surf ? a.fine_gate_s : a.fine_gate_c) : d[4] < 5.0f;
  if (gate) {
    flag |= 1u;
    bool fetch = true;
    if constexpr (GIVEN) {
      if (use_given) {
        fetch = false;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
          // (through an empty asm: two arms that both end in plain loads are merged into ONE load through a pointer chosen
          // between `given` and P -- and `given` then lives in scratch memory instead of registers)
          float gx = (*given)[3 * j], gy = (*given)[3 * j + 1], gz = (*given)[3 * j + 2];
          asm("" : "+v"(gx), "+v"(gy), "+v"(gz));
          nb[j] = make_float4(gx, gy, gz, 0.0f);
        }
      }
    }
    if (!GIVEN || fetch) {
#pragma unroll
      for (int j = 0; j < 5; ++j) nb[j] = P[p[j]];
    }
    if constexpr (INR) {
      // the in-range fit (lslam_device.hpp): division and square root without their range steps, the operands tested; one
      // lane with an operand outside the range and the whole wavefront divides, or fits, again as everybody does (rare; a
      // ballot is over the lanes that are there, so the branches are uniform)
      if (!is_surf) {
        float A[3], B[3];
        if (find_line<true>(nb, A, B)) {  // (findLine's and the coefficient's divisions guard themselves)
          flag |= 2u;
          if (corner_coeff<true>(A, B, sel, coeff)) flag |= 4u;
        }
      } else {
        float plane[4];
        FitRange fr;
        bool ok = find_plane<true>(nb, 0.2f, plane, &fr);
        // (findPlane reads the five to its last statement: they are still here)
        if (__builtin_amdgcn_ballot_w64(fr.bad) != 0) ok = find_plane(nb, 0.2f, plane);
        if (ok) {
          flag |= 2u;
          if (surf_coeff<true>(plane, sel, coeff)) flag |= 4u;  // (|X| guards itself)
        }
      }
    } else if (!is_surf) {
      float A[3], B[3];
      if (find_line(nb, A, B)) {  // ScanMatch.cpp:105-112
        flag |= 2u;
        if (corner_coeff(A, B, sel, coeff)) flag |= 4u;
      }
    } else {
      float plane[4];
#ifdef LSLAM_EXP_NO_FIT  // TIMING EXPERIMENT ONLY (wrong results): no plane fit -- what the fit costs
      plane[0] = 0.0f; plane[1] = 0.0f; plane[2] = 1.0f; plane[3] = -nb[0].z;
      if (nb[1].x < 1.0e30f) {
#else
      if (find_plane(nb, 0.2f, plane)) {  // ScanMatch.cpp:122-130
#endif
        flag |= 2u;
        if (surf_coeff(plane, sel, coeff)) flag |= 4u;
      }
    }
  }
#ifdef LSLAM_FIT_TWICE  // profiling only: the fit and the coefficient once more with no effect -> their share of the kernel time
  if (gate) {
    float4 nb2[5];
    float off = 0.0f;
    asm volatile("" : "+v"(off));
#pragma unroll
    for (int j = 0; j < 5; ++j) nb2[j] = make_float4(nb[j].x + off, nb[j].y, nb[j].z, nb[j].w);
    float c2[4] = {0, 0, 0, 0};
    bool any2 = false;
    if (!is_surf) {
      float A[3], B[3];
      if (find_line(nb2, A, B)) any2 = corner_coeff(A, B, sel, c2);
    } else {
      float plane[4];
      if (find_plane(nb2, 0.2f, plane)) any2 = surf_coeff(plane, sel, c2);
    }
    if (any2 && c2[3] == off + 1e30f) coeff[3] = c2[0];  // never
  }
#endif
  if (flag & 2u) matched = 1.0f;
  if (flag & 4u) {
    jacobian_row(sc, q.x, q.y, q.z, coeff, row, rb);
    kept = 1.0f;
    score = expf(-fabsf(coeff[3]));
  }
  if (a.flags_out) {  // parity taps
    const int gi = bd.out_base + __float_as_int(q.w);  // caller's index of this point
    a.flags_out[gi] = (uint8_t)flag;
    if (a.coeff_out) a.coeff_out[gi] = make_float4(coeff[0], coeff[1], coeff[2], coeff[3]);
    if (a.idx_out) {
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        a.idx_out[gi * 5 + j] = p[j] >= 0 ? __float_as_int(P[p[j]].w) : -1;
        a.d2_out[gi * 5 + j] = d[j];
      }
    }
  }
}

// The block's 27 normal-equation sums and counters from its lanes' rows (ScanMatch.cpp:206-208 products): per-wave contraction
// (MFMA f32 16x16x4 through `stage`, eight word rows of BLOCK lanes that the wavefront owns, or VALU + wave shuffles), then a
// fixed-order sum over the block's waves.  ADD: onto the record another launch left (pass 2 of a two-pass sweep).
// PAD: words added to the staging rows' stride of BLOCK.  With the stride a multiple of the 64 banks the eight lanes that fetch
// the eight rows' entries of one point for an MFMA step share a bank (an eight-way conflict in every one of the sixteen steps);
// with PAD = 4 the 32 words of a step lie in 32 banks.  Same words to the same lanes: same bits.  Only for a caller whose `stage`
// is free of other wavefronts' data (a padded row reaches into the neighbouring wavefronts' columns): the grid sweep, behind
// its workgroup barrier; the tree sweeps stage in the columns of their own traversal stacks, without one.
// FRESH_TID: the thread's number is laundered here, so that nothing worked out from it alone is hoisted out of a caller's loop
// over work items and kept in registers through the searches (sweep_queue_kernel<.., LEAN>).
template <int BLOCK, bool ADD, int PAD = 0, bool FRESH_TID = false>
LSLAM_DEV void block_accumulate(const int jtj_mode, const bool is_surf, const float (&row)[6], const float rb, const float kept,
                                const float matched, const float score, uint32_t *stage, float (*red)[NCOL], float *partial_out) {
  constexpr int NWAVE = BLOCK / 64;
  int tid_v = threadIdx.x;
  if constexpr (FRESH_TID) asm volatile("" : "+v"(tid_v));
  const int tid = tid_v;
  const int lane = tid & 63, wave = tid >> 6;
  // ---- normal equations: per-wave reduction --------------------------------
  float v[NCOL];
#pragma unroll
  for (int i = 0; i < NCOL; ++i) v[i] = 0.0f;

#ifdef LSLAM_EXP_NO_ACC  // TIMING EXPERIMENT ONLY (wrong results): no contraction -- what the per-wave J^T J costs
  if (false) {
#else
  if (jtj_mode == 1) {
#endif
    // stage [J | b] rows; rows of rejected points are zero
    constexpr int ST = BLOCK + PAD;
    float *jr = reinterpret_cast<float *>(stage) + wave * 64;  // [c * ST + p]
#pragma unroll
    for (int c = 0; c < 6; ++c) jr[c * ST + lane] = row[c];
    jr[6 * ST + lane] = rb;
    jr[7 * ST + lane] = 0.0f;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    const int i16 = lane & 15, k4 = lane >> 4;
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const float op = (i16 < 8) ? jr[i16 * ST + 4 * s + k4] : 0.0f;
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(op, op, acc, 0, 0, 0);
    }
    // C/D layout: col = lane&15, row = (lane>>4)*4 + reg.  Entry (r,c), r<=c<7.
    // Scatter the 27 needed entries back to column slots through LDS.
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {
      const int rr = k4 * 4 + r4, cc = i16;
      if (rr < 6 && cc < 7 && cc >= rr) {
        int col;
        if (cc == 6) col = COL_ATB + rr;
        else col = COL_ATA + (rr * 6 - (rr * (rr - 1)) / 2) + (cc - rr);
        red[wave][col] = acc[r4];
      }
    }
    // counters still go through the shuffle reduction
    const float s_rows = wave_sum(kept), s_match = wave_sum(matched), s_score = wave_sum(score);
    if (lane == 0) {
      red[wave][COL_ROWS] = s_rows;
      red[wave][COL_LINE] = is_surf ? 0.0f : s_match;
      red[wave][COL_PLANE] = is_surf ? s_match : 0.0f;
      red[wave][COL_SCORE] = s_score;
      red[wave][31] = 0.0f;
    }
  } else {
    // ScanMatch.cpp:206-208 products, then gfx950 wave-shuffle reduction
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = i; j < 6; ++j) v[k++] = row[i] * row[j];
#pragma unroll
    for (int i = 0; i < 6; ++i) v[COL_ATB + i] = row[i] * rb;
    v[COL_ROWS] = kept;
    v[COL_LINE] = is_surf ? 0.0f : matched;
    v[COL_PLANE] = is_surf ? matched : 0.0f;
    v[COL_SCORE] = score;
#pragma unroll
    for (int i = 0; i < 31; ++i) v[i] = wave_sum(v[i]);
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < NCOL; ++i) red[wave][i] = v[i];
    }
  }
  __syncthreads();
  // LDS-staged per-block accumulation: fixed order over the block's waves
  if (tid < NCOL) {
    float s = red[0][tid];
#pragma unroll
    for (int w = 1; w < NWAVE; ++w) s += red[w][tid];
    if (ADD) partial_out[tid] += s;  // onto the record pass 1 left (this thread alone touches the word)
    else partial_out[tid] = s;
  }
}

}  // namespace lslam
