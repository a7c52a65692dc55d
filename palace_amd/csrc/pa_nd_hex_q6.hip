// Fused E -> B/G -> D -> B^T/G^T -> E^T for Nedelec hexahedra at six points per direction (gfx950, FP64): the pairs (p, 6),
// p = 1 ... 5 of PA_HEX_Q6_LIST -- the order-5 operator and the coarser levels of its p-multigrid hierarchy, which reuse the
// fine level's quadrature data.  Same chain, same sum-factorised passes (pa_nd_hex_core.hpp) and same pointwise D
// (pa_device.hpp) as the one-shot kernel of pa_nd_hex.hip; what differs is how the kernel is fitted to the machine:
//
//   * One element per wave: 64 / 36 = 1.  Lanes 0 ... 35 own the 36 lines of a pass; lanes 36 ... 63 own nothing and
//     leave before the first memory access -- no global access, no LDS store.  A wave past the last element leaves as a
//     whole: there is no workgroup barrier anywhere.
//   * The 1-D tables do not travel as kernel arguments (51 doubles at p = 5, the whole SGPR budget): every wave copies the
//     operator's device tables into its own LDS strip and the passes read them from there (broadcast reads into VGPRs).
//     The price is registers: the kernel is bound to one wave per SIMD (see the launch bound below).
//   * The D stage walks the lane's qz column point by point with the next point's data requested one point ahead (the first
//     point before the forward contraction), instead of holding the column: 7 ... 12 doubles in flight instead of 42 ... 72.
//
// The exclusive-dof store and the two right-hand-side form of pa_nd_hex.hip do not exist here (they stop at four points).
#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

#include "pa_nd_hex_core.hpp"

namespace pa {

constexpr int kQ6Waves = 4;  // waves = elements per workgroup: 4 x 8.6 KiB of LDS at p = 5

struct NDQ6Tab {  // what the shared passes read as a.tab: the full row-major tables, whose first rows are the half tables
  const double *Bo, *Bc, *Gc;
};
struct NDQ6View {
  NDQ6Tab tab;
};

// LDS of one wave: the contraction buffers of its element (NDLayout), then its copy of the 1-D tables [Bo | Bc | Gc]
template <int P1, int Q1>
struct NDQ6Strip {
  static constexpr int ELEM = NDLayout<P1, Q1>::ELEM_PAD;
  static constexpr int TAB = Q1 * (P1 + 2 * (P1 + 1));
  static constexpr int STRIDE = ELEM + ((TAB + 1) & ~1);
};

template <int P1, int Q1>
struct NDQ6Args {
  int ne;
  const int32_t *sidx;     // signed sorted index (atomic scatter)
  const int32_t *sidx_in;  // the same with kEssBit on the dofs to be read as zero
  const uint16_t *perm;    // [ne][P] tensor-order slot of sorted entry m
  const double *geom;
  const double *qdata;     // packed symmetric D or the metric form (QD)
  const double *x;
  double *y;               // L-vector target of the atomic scatter (EVEC == false)
  double *ye;              // E-vector target [ne][P], sorted order, unsigned (EVEC == true)
  int xcd_chunk;           // > 0: workgroups are dealt to the 8 XCDs round-robin; give each XCD one contiguous element range
  int cross;               // 1 / 2: the mixed curl forms of hcurlhdiv_33_qf.h (matrix-free D, coefficient in c_mass)
  CoeffDev c_mass, c_curl;
  const double *tab;       // the operator's device copy of the full 1-D tables, [Bo | Bc | Gc]
  const int32_t *attr_e;   // metric form: element attributes
};

// D-stage data of one quadrature point
template <bool USE_U, bool USE_C, bool ISO, bool QD>
struct NDQ6Point {
  static constexpr bool METRIC = QD && ISO;  // q-data = G = J^T J (6 per point) and |detJ| / w, coefficients applied here
  static constexpr int NG = QD ? (METRIC ? (USE_U ? 7 : 6) : (USE_U ? 6 : 0) + (USE_C ? 6 : 0)) : 10;
  static constexpr int NSTORED = QD ? (METRIC ? 7 : NG) : 11;  // components per element as stored
  double g[NG];
  int attr;
  // src: the element's data at the lane's (qx, qy); QS: points per element
  template <int QS>
  __device__ __forceinline__ void load(const double *__restrict__ src, const int qoff) {
    attr = QD ? 0 : (int)src[qoff];
#pragma unroll
    for (int c = 0; c < NG; c++) g[c] = src[(QD ? c : 1 + c) * QS + qoff];
  }
};

// D at one point (hcurl_33 / hdiv_33 / hdivmass_33 / hcurlhdiv_33): u = values, cu = curls, in place
template <bool USE_U, bool USE_C, bool ISO, bool QD, class Args>
__device__ __forceinline__ void nd_q6_point(const Args &a, const NDQ6Point<USE_U, USE_C, ISO, QD> &pt, const int attr_m,
                                            double (&u)[3], double (&cu)[3]) {
  constexpr bool METRIC = QD && ISO;
  if (METRIC) {
    // (w / detJ) J^T c J = c H,   w detJ adj^T c adj = c (|detJ| / w) adj(H)   (pa_nd_hex.hip)
    const double *H = pt.g;
    if (USE_U) {
      const double cm = pt.g[USE_U ? 6 : 0] * a.c_mass.mat[9 * coeff_index(a.c_mass, attr_m)];
      const double m[6] = {cm * (H[3] * H[5] - H[4] * H[4]), cm * (H[2] * H[4] - H[1] * H[5]), cm * (H[1] * H[4] - H[2] * H[3]),
                           cm * (H[0] * H[5] - H[2] * H[2]), cm * (H[1] * H[2] - H[0] * H[4]), cm * (H[0] * H[3] - H[1] * H[1])};
      sym_mv(m, u[0], u[1], u[2], u[0], u[1], u[2]);
    }
    if (USE_C) {
      const double cc = a.c_curl.mat[9 * coeff_index(a.c_curl, attr_m)];
      const double m[6] = {cc * H[0], cc * H[1], cc * H[2], cc * H[3], cc * H[4], cc * H[5]};
      sym_mv(m, cu[0], cu[1], cu[2], cu[0], cu[1], cu[2]);
    }
  } else if (QD) {
    if (USE_U) sym_mv(&pt.g[0], u[0], u[1], u[2], u[0], u[1], u[2]);
    if (USE_C) sym_mv(&pt.g[(USE_U && USE_C) ? 6 : 0], cu[0], cu[1], cu[2], cu[0], cu[1], cu[2]);
  } else {
    const double wdetJ = pt.g[0];
    const double *adj = &pt.g[QD ? 0 : 1];
    if (ISO) {
      if (USE_U) mult_AtAx33(adj, u[0], u[1], u[2], wdetJ * a.c_mass.mat[9 * coeff_index(a.c_mass, pt.attr)], u[0], u[1], u[2]);
      if (USE_C) {
        double Jl[9];
        adjJt33(adj, Jl);
        mult_AtAx33(Jl, cu[0], cu[1], cu[2], wdetJ * a.c_curl.mat[9 * coeff_index(a.c_curl, pt.attr)], cu[0], cu[1], cu[2]);
      }
    } else if (USE_U && USE_C && a.cross) {
      // cross 1 = f_apply_hcurlhdiv_33 (values in, curl test functions out), 2 = f_apply_hdivhcurl_33
      double Cm[9], Jl[9], o0, o1, o2;
      coeff_unpack3(a.c_mass, pt.attr, Cm);
      adjJt33(adj, Jl);
      if (a.cross == 1) {
        mult_AtBCx33(Jl, Cm, adj, u[0], u[1], u[2], wdetJ, o0, o1, o2);
        cu[0] = o0, cu[1] = o1, cu[2] = o2;
        u[0] = u[1] = u[2] = 0.0;
      } else {
        mult_AtBCx33(adj, Cm, Jl, cu[0], cu[1], cu[2], wdetJ, o0, o1, o2);
        u[0] = o0, u[1] = o1, u[2] = o2;
        cu[0] = cu[1] = cu[2] = 0.0;
      }
    } else {
      double Cm[9];
      if (USE_U) {
        coeff_unpack3(a.c_mass, pt.attr, Cm);
        mult_AtBCx33(adj, Cm, adj, u[0], u[1], u[2], wdetJ, u[0], u[1], u[2]);
      }
      if (USE_C) {
        double Jl[9];
        coeff_unpack3(a.c_curl, pt.attr, Cm);
        adjJt33(adj, Jl);
        mult_AtBCx33(Jl, Cm, Jl, cu[0], cu[1], cu[2], wdetJ, cu[0], cu[1], cu[2]);
      }
    }
  }
}

// Launch bound: one wave per SIMD, i.e. the whole register file (512 per lane) if the compiler wants it.  Under the bound of
// two waves the table operands, which now live in VGPRs, pushed the metric curl-curl + mass form to 788 B of scratch per lane
// at p = 5; the forms that need fewer registers still run at the occupancy their own count allows.
template <int P1, int Q1, bool USE_U, bool USE_C, bool ISO, bool EVEC, bool QD>
__global__ __launch_bounds__(64 * kQ6Waves, 1) void nd_hex_q6_kernel(const NDQ6Args<P1, Q1> a) {
  using L = NDLayout<P1, Q1>;
  using Pt = NDQ6Point<USE_U, USE_C, ISO, QD>;
  static_assert(L::EPW == 1 && L::T <= 64, "one element per wave");
  constexpr int Q = Q1 * Q1 * Q1;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int bid = a.xcd_chunk > 0 ? (int)(blockIdx.x & 7) * a.xcd_chunk + (int)(blockIdx.x >> 3) : (int)blockIdx.x;
  const int e = bid * kQ6Waves + wave;
  if (e >= a.ne) return;  // the whole wave: waves never wait for each other
  if (lane >= L::T) return;  // the lanes without a line: masked off for the rest of the wave's life
  constexpr bool lane_ok = true;  // (what the shared passes guard their stores with: every lane left owns a line)
  const int t = lane, ta = t % Q1, tb = t / Q1;
  using S = NDQ6Strip<P1, Q1>;
  double *sm = smem + (size_t)wave * S::STRIDE;
  for (int i = t; i < S::TAB; i += L::T) sm[S::ELEM + i] = a.tab[i];  // (visible to the wave at the first wave_sync())
  NDQ6View v;
  v.tab.Bo = sm + S::ELEM, v.tab.Bc = v.tab.Bo + Q1 * P1, v.tab.Gc = v.tab.Bc + Q1 * (P1 + 1);

  // D-stage data of the first point of this lane's column: requested now, consumed after the forward contraction
  const double *dsrc = (QD ? a.qdata : a.geom) + (size_t)e * Pt::NSTORED * Q + t;
  Pt pt[2];
#pragma unroll
  for (int c = 0; c < Pt::NG; c++) pt[0].g[c] = 0.0, pt[1].g[c] = 0.0;
  pt[0].attr = pt[1].attr = 1;
  pt[0].template load<Q>(dsrc, 0);

  // E: sorted-order gather, staged through LDS into tensor order
  constexpr int NC = P1 + 1, PP = 3 * P1 * NC * NC, NPL = (PP + L::T - 1) / L::T;
  int lp[NPL];
#pragma unroll
  for (int r = 0; r < NPL; r++) {
    const int m = t + L::T * r;
    lp[r] = 0;
    if (L::T * (r + 1) <= PP || m < PP) {  // (only the last round can be partial)
      lp[r] = a.perm[(size_t)e * PP + m];
      const int s = a.sidx_in[(size_t)e * PP + m];
      const int d = s >= 0 ? s : -1 - s;
      const double xv = (d & kEssBit) ? 0.0 : a.x[d & ~kEssBit];  // essential dofs read as zero (ParOperator's tx[ess] = 0)
      sm[lp[r]] = s >= 0 ? xv : -xv;
    }
  }
  wave_sync();
  double uin[3][NC];
#pragma unroll
  for (int C = 0; C < 3; C++) {
    const int ni = (C == 0) ? P1 : NC, nj = (C == 1) ? P1 : NC, nk = (C == 2) ? P1 : NC;
    const bool act = ta < nj && tb < nk;
#pragma unroll
    for (int i = 0; i < NC; i++) uin[C][i] = (act && i < ni) ? sm[C * P1 * NC * NC + i + ni * (ta + nj * tb)] : 0.0;
  }
  wave_sync();

  double U[3][Q1], CU[3][Q1];
#pragma unroll
  for (int c = 0; c < 3; c++)
#pragma unroll
    for (int q = 0; q < Q1; q++) U[c][q] = 0.0, CU[c][q] = 0.0;

  nd_fwd_comp<0, P1, Q1, USE_U, USE_C>(v, e, lane_ok, lane_ok, ta, tb, 0, sm, uin[0], U, CU);
  nd_fwd_comp<1, P1, Q1, USE_U, USE_C>(v, e, lane_ok, lane_ok, ta, tb, 0, sm, uin[1], U, CU);
  nd_fwd_comp<2, P1, Q1, USE_U, USE_C>(v, e, lane_ok, lane_ok, ta, tb, 0, sm, uin[2], U, CU);

  // D, point by point along qz; the next point's data is on its way while this one is applied
  {
    const int attr_m = Pt::METRIC ? a.attr_e[e] : 1;
#pragma unroll
    for (int qz = 0; qz < Q1; qz++) {
      if (qz + 1 < Q1) pt[(qz + 1) & 1].template load<Q>(dsrc, Q1 * Q1 * (qz + 1));
      double u[3] = {U[0][qz], U[1][qz], U[2][qz]}, cu[3] = {CU[0][qz], CU[1][qz], CU[2][qz]};
      nd_q6_point<USE_U, USE_C, ISO, QD>(a, pt[qz & 1], attr_m, u, cu);
      U[0][qz] = u[0], U[1][qz] = u[1], U[2][qz] = u[2];
      CU[0][qz] = cu[0], CU[1][qz] = cu[1], CU[2][qz] = cu[2];
      __builtin_amdgcn_sched_barrier(0);  // one point at a time: the loads stay one point ahead, no further
    }
  }

  nd_bwd_comp<0, P1, Q1, USE_U, USE_C>(v, e, lane_ok, lane_ok, ta, tb, 0, sm, uin[0], U, CU);
  nd_bwd_comp<1, P1, Q1, USE_U, USE_C>(v, e, lane_ok, lane_ok, ta, tb, 0, sm, uin[1], U, CU);
  nd_bwd_comp<2, P1, Q1, USE_U, USE_C>(v, e, lane_ok, lane_ok, ta, tb, 0, sm, uin[2], U, CU);

  // E^T, first half: element-local results back into tensor order in LDS, then out in sorted order (coalesced E-vector
  // store; signs and the sum over elements happen in et_gather_kernel) or, in the atomic form, straight into y
#pragma unroll
  for (int C = 0; C < 3; C++) {
    const int ni = (C == 0) ? P1 : NC, nj = (C == 1) ? P1 : NC, nk = (C == 2) ? P1 : NC;
    const bool act = ta < nj && tb < nk;
#pragma unroll
    for (int i = 0; i < NC; i++)
      if (act && i < ni) sm[C * P1 * NC * NC + i + ni * (ta + nj * tb)] = uin[C][i];
  }
  wave_sync();
#pragma unroll
  for (int r = 0; r < NPL; r++) {
    const int m = t + L::T * r;
    if (L::T * (r + 1) <= PP || m < PP) {  // (only the last round can be partial)
      const double v = sm[lp[r]];
      if (EVEC) {
        a.ye[(size_t)e * PP + m] = v;
      } else {
        const int s = a.sidx[(size_t)e * PP + m];
        unsafeAtomicAdd(&a.y[s >= 0 ? s : -1 - s], s >= 0 ? v : -v);
      }
    }
  }
}

template <int P1, int Q1, bool U, bool C>
static void q6_launch_forms(const NDQ6Args<P1, Q1> &a, bool iso, dim3 grid, dim3 block, size_t lds, hipStream_t s) {
  const bool evec = a.ye != nullptr;
  // (more dynamic LDS than the default limit needs the attribute; 4 x 8.6 KiB at p = 5 does not, kept for other wave counts)
#define PA_Q6_LAUNCH(ISO, EVEC, QD)                                                                                     \
  {                                                                                                                     \
    auto *k = nd_hex_q6_kernel<P1, Q1, U, C, ISO, EVEC, QD>;                                                            \
    if (lds > 64 * 1024) PA_HIP(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
    hipLaunchKernelGGL(k, grid, block, lds, s, a);                                                                      \
  }
  if (a.qdata && a.attr_e) {  // metric form of the q-data
    if (evec) PA_Q6_LAUNCH(true, true, true) else PA_Q6_LAUNCH(true, false, true)
  } else if (a.qdata) {
    if (evec) PA_Q6_LAUNCH(false, true, true) else PA_Q6_LAUNCH(false, false, true)
  } else if (iso) {
    if (evec) PA_Q6_LAUNCH(true, true, false) else PA_Q6_LAUNCH(true, false, false)
  } else {
    if (evec) PA_Q6_LAUNCH(false, true, false) else PA_Q6_LAUNCH(false, false, false)
  }
#undef PA_Q6_LAUNCH
}

template <int P1, int Q1>
static void q6_launch_pq(const SubOp &so, const double *x, double *y, double *ye, bool masked, hipStream_t s) {
  NDQ6Args<P1, Q1> a;
  a.ne = so.ne;
  a.sidx = so.d_sidx;
  a.sidx_in = (masked && so.d_sidx_bc) ? so.d_sidx_bc : so.d_sidx;
  a.perm = so.d_perm;
  a.geom = so.geom->d_geom;
  a.qdata = so.qd ? so.qd->d : nullptr;
  a.attr_e = (so.qd && so.qd->metric) ? so.geom->d_attr_e : nullptr;
  a.x = x, a.y = y, a.ye = ye;
  a.tab = so.d_tab;
  const int nblk = (so.ne + kQ6Waves - 1) / kQ6Waves;
  a.xcd_chunk = nblk >= 64 ? (nblk + 7) / 8 : 0;
  const dim3 grid(a.xcd_chunk > 0 ? 8 * a.xcd_chunk : nblk), block(64 * kQ6Waves);
  const size_t lds = sizeof(double) * (size_t)kQ6Waves * NDQ6Strip<P1, Q1>::STRIDE;
  bool use_u, use_c;
  nd_terms(so, use_u, use_c, a.c_mass, a.c_curl, a.cross);
  if (a.cross) {  // as in pa_nd_hex.hip: both fields, general coefficient; the transpose of one form is the other
    a.c_curl = a.c_mass;
    if (TransposeScope::active()) a.cross = 3 - a.cross;
  }
  const bool both = a.cross || (use_u && use_c);
  if (!both && use_c)
    q6_launch_forms<P1, Q1, false, true>(a, so.iso, grid, block, lds, s);
  else if (!both)
    q6_launch_forms<P1, Q1, true, false>(a, so.iso, grid, block, lds, s);
  else
    q6_launch_forms<P1, Q1, true, true>(a, so.iso && !a.cross, grid, block, lds, s);
  PA_HIP(hipGetLastError());
}

void launch_nd_hex_q6(const SubOp &so, const double *x, double *y, double *ye, bool masked, hipStream_t s) {
  PA_REQUIRE(so.d_tab, "1-D tables missing on the device");
  switch (so.p * 16 + so.q1d) {
    PA_HEX_Q6_LIST(PA_HEX_PQ_CALL, q6_launch_pq, so, x, y, ye, masked, s)
    default: throw hex_pq_error("H(curl)", so.p, so.q1d);
  }
}

}  // namespace pa
