// Fused E -> B -> D -> B^T for Raviart-Thomas tensor-product hexahedra (gfx950, FP64): the H(div) mass, div-div and
// div-div + mass operators (reference integrators fem/integ/{vecfemass,divdiv,divdivmass}.cpp on an RT space; D from
// fem/qfunctions/33/hdiv_33_qf.h, fem/qfunctions/1/l2_1_qf.h and fem/qfunctions/33/l2mass_33_qf.h).
//
// Element (fem/rthex.py): component c of the order-p element is closed (Gauss-Lobatto, p + 1 nodes) along c and open
// (Gauss-Legendre, p nodes) along the other two directions; its value is  Bc (along c) x Bo x Bo,  its divergence the same
// product with Gc along c, so the two share the two open passes.
//
// Same mapping as pa_h1_hex.hip / pa_nd_hex.hip: Q1^2 lanes per element, 64 / Q1^2 elements per wave, passes X -> Y -> Z
// through LDS inside the wave (wave-level syncs only), lane (qx, qy) ends with its qz column of the three values and the
// divergence; E is the sorted gather through d_sidx / d_perm, E^T the E-vector + gather form.
#include "pa_rt_hex_core.hpp"

namespace pa {

// USE_V: mass term (values), USE_DIV: div-div term; QD: packed pre-assembled D, else matrix-free from the geometry rows
template <int P1, int Q1, bool USE_V, bool USE_DIV, bool QD>
__global__ __launch_bounds__(64 * kRTWaves, 2) void rt_hex_apply_kernel(const RTArgs<P1, Q1> a) {
  using L = RTLayout<P1, Q1>;
  constexpr int Q = Q1 * Q1 * Q1, P = L::BASE;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane / L::T, t = lane - sub * L::T;
  const int ta = t % Q1, tb = t / Q1;
  const bool lane_ok = sub < L::EPW;
  const int e = (blockIdx.x * kRTWaves + wave) * L::EPW + sub;
  const bool active = lane_ok && e < a.ne;
  double *sm = smem + (size_t)(wave * L::EPW + (lane_ok ? sub : 0)) * L::ELEM_PAD;
  const size_t eg = active ? e : 0;  // idle lanes read element 0 and store nothing

  // packed D of this lane's Q1 points, requested up front
  constexpr int NG = (USE_V ? 6 : 0) + (USE_DIV ? 1 : 0);
  double gd[Q1][NG];
  if (QD) {
    const double *g = a.qdata + eg * NG * Q + ta + Q1 * tb;
#pragma unroll
    for (int qz = 0; qz < Q1; qz++)
#pragma unroll
      for (int c = 0; c < NG; c++) gd[qz][c] = g[c * Q + Q1 * Q1 * qz];
  }

  // E: sorted-order gather staged through LDS into tensor order (orientation signs applied here)
  constexpr int NPL = (P + L::T - 1) / L::T;
  int lp[NPL];
  bool neg[NPL];
#pragma unroll
  for (int r = 0; r < NPL; r++) {
    const int m = t + L::T * r;
    lp[r] = 0, neg[r] = false;
    if (active && m < P) {
      const int s = a.sidx_in[(size_t)e * P + m];
      neg[r] = s < 0;
      const int d = s >= 0 ? s : -1 - s;
      lp[r] = a.perm[(size_t)e * P + m];
      const double v = (d & kEssBit) ? 0.0 : a.x[d & ~kEssBit];
      sm[lp[r]] = neg[r] ? -v : v;
    }
  }
  wave_sync();

  double V[3][Q1], DV[Q1];
#pragma unroll
  for (int qz = 0; qz < Q1; qz++) DV[qz] = 0.0;
  rt_fwd_comp<P1, Q1, 0, USE_V, USE_DIV>(a.tab, sm, ta, tb, lane_ok, V[0], DV);
  rt_fwd_comp<P1, Q1, 1, USE_V, USE_DIV>(a.tab, sm, ta, tb, lane_ok, V[1], DV);
  rt_fwd_comp<P1, Q1, 2, USE_V, USE_DIV>(a.tab, sm, ta, tb, lane_ok, V[2], DV);
  wave_sync();

  // ---- D (hdiv_33 / l2_1 / l2mass_33)
#pragma unroll
  for (int qz = 0; qz < Q1; qz++) {
    if (QD) {
      if (USE_V) sym_mv(&gd[qz][0], V[0][qz], V[1][qz], V[2][qz], V[0][qz], V[1][qz], V[2][qz]);
      if (USE_DIV) DV[qz] *= gd[qz][NG - 1];
    } else {
      const double *g = a.geom + eg * 11 * Q + ta + Q1 * tb + Q1 * Q1 * qz;
      const int attr = (int)g[0];
      const double wdetJ = g[Q];
      if (USE_V) {
        double adj[9], Jl[9], Cm[9];
#pragma unroll
        for (int c = 0; c < 9; c++) adj[c] = g[(2 + c) * Q];
        adjJt33(adj, Jl);
        coeff_unpack3(a.c_mass, attr, Cm);
        mult_AtBCx33(Jl, Cm, Jl, V[0][qz], V[1][qz], V[2][qz], wdetJ, V[0][qz], V[1][qz], V[2][qz]);
      }
      if (USE_DIV) {
        const double qw = a.w1[ta] * a.w1[tb] * a.w1[qz];
        DV[qz] *= coeff_unpack1(a.c_div, attr) * qw * qw / wdetJ;
      }
    }
  }

  rt_bwd_comp<P1, Q1, 0, USE_V, USE_DIV>(a.tab, sm, ta, tb, lane_ok, V[0], DV);
  rt_bwd_comp<P1, Q1, 1, USE_V, USE_DIV>(a.tab, sm, ta, tb, lane_ok, V[1], DV);
  rt_bwd_comp<P1, Q1, 2, USE_V, USE_DIV>(a.tab, sm, ta, tb, lane_ok, V[2], DV);
  wave_sync();
  // E^T, first half: out of LDS in sorted order (coalesced).  The E-vector holds the unsigned element results: the gather
  // applies the orientation sign of the entry (d_tent).
#pragma unroll
  for (int r = 0; r < NPL; r++) {
    const int m = t + L::T * r;
    if (active && m < P) a.ye[(size_t)e * P + m] = sm[lp[r]];
  }
}

template <int P1, int Q1>
static void rt_launch_pq(const SubOp &so, const double *x, bool masked, hipStream_t s) {
  using L = RTLayout<P1, Q1>;
  constexpr int QH = RTTab<P1, Q1>::QH, NC = P1 + 1;
  RTArgs<P1, Q1> a{};
  a.ne = so.ne;
  a.sidx_in = (masked && so.d_sidx_bc) ? so.d_sidx_bc : so.d_sidx;
  a.perm = so.d_perm;
  a.geom = so.geom->d_geom;
  a.qdata = so.qd ? so.qd->d : nullptr;
  a.x = x;
  a.ye = so.d_ye;
  PA_REQUIRE((int)so.geom->w1.size() == Q1, "geometry data without its 1-D quadrature weights");
  for (int q = 0; q < Q1; q++) a.w1[q] = so.geom->w1[q];
  for (int i = 0; i < QH * P1; i++) a.tab.Bo[i] = so.Bo[i];
  for (int i = 0; i < QH * NC; i++) a.tab.Bc[i] = so.Bc[i], a.tab.Gc[i] = so.Gc[i];
  const int epb = kRTWaves * L::EPW;
  const dim3 grid((so.ne + epb - 1) / epb), block(64 * kRTWaves);
  const size_t lds = sizeof(double) * (size_t)epb * L::ELEM_PAD;
  const bool qd = a.qdata != nullptr;
#define PA_RT_LAUNCH(V, D)                                                                    \
  if (qd)                                                                                     \
    hipLaunchKernelGGL((rt_hex_apply_kernel<P1, Q1, V, D, true>), grid, block, lds, s, a);    \
  else                                                                                        \
    hipLaunchKernelGGL((rt_hex_apply_kernel<P1, Q1, V, D, false>), grid, block, lds, s, a);
  switch (so.qf) {
    case PA_QF_HDIV_33:
      a.c_mass = so.c0.dev();
      PA_RT_LAUNCH(true, false)
      break;
    case PA_QF_L2_1:
      a.c_div = so.c0.dev();
      PA_RT_LAUNCH(false, true)
      break;
    case PA_QF_L2MASS_33:
      a.c_mass = so.c0.dev();
      a.c_div = so.c1.dev();
      PA_RT_LAUNCH(true, true)
      break;
    default:
      throw Error("QFunction not available for H(div) hexahedra");
  }
#undef PA_RT_LAUNCH
  PA_HIP(hipGetLastError());
}

// writes the E-vector so.d_ye; the caller follows with launch_et_gather
void launch_rt_hex_apply(const SubOp &so, const double *x, bool masked, hipStream_t s) {
  PA_REQUIRE(so.d_ye, "H(div) blocks use the gather form of E^T");
  PA_REQUIRE(!masked || so.d_sidx_bc, "pa_op_set_essential has not been called");
  if (so.q1d == 6) return launch_rt_hex_q6(so, x, masked, s);  // six points per direction: pa_rt_hex_q6.hip
  PA_HEX_DISPATCH(rt_launch_pq, "H(div)", so, x, masked, s)
}

// ---- packed q-data and diagonal (set-up) ----------------------------------------------------------
// [ne][ncomp][Q] per element: (w / detJ) J^T C J = w detJ Jl^T C Jl, Jl = J / detJ (six upper entries), then
// c qw^2 / (w detJ).  One thread per point.
struct RTWeights {
  double w[kMaxQ1];
};
__global__ void rt_hex_qdata_kernel(const int ne, const int q1d, const double *__restrict__ geom, const CoeffDev c_mass,
                                    const CoeffDev c_div, const RTWeights w1, const int use_v, const int use_d,
                                    double *__restrict__ qd) {
  const int Q = q1d * q1d * q1d;
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int e = (int)(gid / Q);
  if (e >= ne) return;
  const int q = (int)(gid - (long long)e * Q);
  const double *g = geom + (size_t)e * 11 * Q;
  const int ncomp = 6 * use_v + use_d;
  double *out = qd + (size_t)e * ncomp * Q + q;
  const int attr = (int)g[q];
  const double w = g[Q + q];
  int o = 0;
  if (use_v) {
    double adj[9], Jl[9], Cm[9], M[9];
    for (int c = 0; c < 9; c++) adj[c] = g[(2 + c) * Q + q];
    adjJt33(adj, Jl);
    coeff_unpack3(c_mass, attr, Cm);
    for (int col = 0; col < 3; col++)
      mult_AtBCx33(Jl, Cm, Jl, col == 0, col == 1, col == 2, w, M[0 + 3 * col], M[1 + 3 * col], M[2 + 3 * col]);
    sym_pack(M, [&](const int i, const double v) { out[i * Q] = v; });
    o = 6;
  }
  if (use_d) {
    const double qw = w1.w[q % q1d] * w1.w[(q / q1d) % q1d] * w1.w[q / (q1d * q1d)];
    out[o * Q] = coeff_unpack1(c_div, attr) * qw * qw / w;
  }
}

static void rt_terms(const SubOp &so, bool &use_v, bool &use_d, CoeffDev &cm, CoeffDev &cd) {
  use_v = so.qf == PA_QF_HDIV_33 || so.qf == PA_QF_L2MASS_33;
  use_d = so.qf == PA_QF_L2_1 || so.qf == PA_QF_L2MASS_33;
  PA_REQUIRE(use_v || use_d, "QFunction not available for H(div) hexahedra");
  cm = CoeffDev{}, cd = CoeffDev{};
  if (so.qf == PA_QF_HDIV_33) cm = so.c0.dev();
  if (so.qf == PA_QF_L2_1) cd = so.c0.dev();
  if (so.qf == PA_QF_L2MASS_33) cm = so.c0.dev(), cd = so.c1.dev();
}

void launch_rt_hex_qdata(SubOp &so, hipStream_t s) {
  bool use_v, use_d;
  CoeffDev cm, cd;
  rt_terms(so, use_v, use_d, cm, cd);
  PA_REQUIRE((int)so.geom->w1.size() == so.q1d, "geometry data without its 1-D quadrature weights");
  const Ref<QData> qd(new QData);
  qd->ncomp = 6 * (int)use_v + (int)use_d;
  qd->d = dev_alloc<double>((size_t)so.ne * qd->ncomp * so.Q);
  RTWeights w{};
  for (int q = 0; q < so.q1d; q++) w.w[q] = so.geom->w1[q];
  const long long n = (long long)so.ne * so.Q;
  hipLaunchKernelGGL(rt_hex_qdata_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, so.ne, so.q1d, so.geom->d_geom,
                     cm, cd, w, (int)use_v, (int)use_d, qd->d);
  PA_HIP(hipGetLastError());
  so.qd = qd;
}

// diag_l = sum_q [ D_cc(q) (B_x B_y B_z)^2 + d(q) (the same product with Gc along c)^2 ] for a dof l of component c: only the
// diagonal entry of the pointwise mass matrix reaches it, and the orientation signs drop out.  Both D forms: the four numbers
// per point come from the packed q-data or from the geometry rows.  One workgroup per element; sum-factorised with the SQUARED
// 1-D tables: D is contracted along x, then y (partial sums staged in LDS, shared by the dofs of a line), then z per dof.
struct RTDiagArgs {
  int ne, p, q1;
  const int32_t *sidx;
  const uint16_t *perm;
  double *ye;
  const double *geom, *qdata;
  CoeffDev c_mass, c_div;
  const double *Bo, *Bc, *Gc;  // device, full [q1][n]
  double w1[kMaxQ1];           // 1-D quadrature weights
  bool use_v, use_d;
};

__global__ void rt_hex_diag_kernel(const RTDiagArgs a) {
  extern __shared__ __attribute__((aligned(16))) double dsm[];
  const int P1 = a.p, Q1 = a.q1, NC = P1 + 1, Q = Q1 * Q1 * Q1, NB = P1 * P1 * NC, P = 3 * NB;
  double *Dm = dsm;  // [4][Q]: D_00, D_11, D_22, d
  double *Tsq = Dm + 4 * Q, *Af = Tsq + 3 * Q1 * NC, *Bf = Af + 6 * NC * Q1 * Q1;  // see below
  const int e = blockIdx.x;
  const int ncomp = 6 * (int)a.use_v + (int)a.use_d;
  for (int q = threadIdx.x; q < Q; q += blockDim.x) {
    double d0 = 0.0, d1 = 0.0, d2 = 0.0, dd = 0.0;
    if (a.qdata) {
      const double *g = a.qdata + (size_t)e * ncomp * Q + q;
      if (a.use_v) d0 = g[0], d1 = g[3 * Q], d2 = g[5 * Q];
      if (a.use_d) dd = g[(ncomp - 1) * Q];
    } else {
      const double *g = a.geom + (size_t)e * 11 * Q + q;
      const int attr = (int)g[0];
      const double w = g[Q];
      if (a.use_v) {
        double adj[9], Jl[9], Cm[9], y0, y1, y2;
        for (int c = 0; c < 9; c++) adj[c] = g[(2 + c) * Q];
        adjJt33(adj, Jl);
        coeff_unpack3(a.c_mass, attr, Cm);
        mult_AtBCx33(Jl, Cm, Jl, 1.0, 0.0, 0.0, w, d0, y1, y2);
        mult_AtBCx33(Jl, Cm, Jl, 0.0, 1.0, 0.0, w, y0, d1, y2);
        mult_AtBCx33(Jl, Cm, Jl, 0.0, 0.0, 1.0, w, y0, y1, d2);
      }
      if (a.use_d) {
        const double qw = a.w1[q % Q1] * a.w1[(q / Q1) % Q1] * a.w1[q / (Q1 * Q1)];
        dd = coeff_unpack1(a.c_div, attr) * qw * qw / w;
      }
    }
    Dm[q] = d0, Dm[Q + q] = d1, Dm[2 * Q + q] = d2, Dm[3 * Q + q] = dd;
  }
  // squared 1-D tables [Bo^2 | Bc^2 | Gc^2], each [Q1][NC] (Bo: the first P1 columns)
  for (int t = threadIdx.x; t < Q1 * NC; t += blockDim.x) {
    const int q = t / NC, i = t - q * NC;
    const double bo = i < P1 ? a.Bo[q * P1 + i] : 0.0, bc = a.Bc[t], gc = a.Gc[t];
    Tsq[t] = bo * bo, Tsq[Q1 * NC + t] = bc * bc, Tsq[2 * Q1 * NC + t] = gc * gc;
  }
  __syncthreads();
  const double *Bo2 = Tsq, *Bc2 = Tsq + Q1 * NC, *Gc2 = Tsq + 2 * Q1 * NC;
  // contraction along x: A[c][f][i][qy][qz] = sum_qx T_x(qx, i)^2 D(q), f = 0: D_cc with the value table, f = 1: d with the
  // derivative table along c
  for (int t = threadIdx.x; t < 3 * NC * Q1 * Q1; t += blockDim.x) {
    const int C = t / (NC * Q1 * Q1), r = t - C * NC * Q1 * Q1, i = r / (Q1 * Q1), qyz = r - i * Q1 * Q1;
    if (i >= ((C == 0) ? NC : P1)) continue;
    const double *TV = (C == 0) ? Bc2 : Bo2, *TD = (C == 0) ? Gc2 : Bo2;
    const double *Dc = Dm + C * Q, *Dd = Dm + 3 * Q;
    double v = 0.0, d = 0.0;
    for (int qx = 0; qx < Q1; qx++) {
      v += TV[qx * NC + i] * Dc[qx + Q1 * qyz];
      d += TD[qx * NC + i] * Dd[qx + Q1 * qyz];
    }
    // (qyz = qy + Q1 qz)
    Af[((C * 2 + 0) * NC + i) * Q1 * Q1 + qyz] = v, Af[((C * 2 + 1) * NC + i) * Q1 * Q1 + qyz] = d;
  }
  __syncthreads();
  // along y: B[c][f][i][j][qz] = sum_qy T_y(qy, j)^2 A[c][f][i][qy][qz]
  for (int t = threadIdx.x; t < 3 * NC * NC * Q1; t += blockDim.x) {
    const int C = t / (NC * NC * Q1), r = t - C * NC * NC * Q1, i = r / (NC * Q1), j = (r / Q1) % NC, qz = r % Q1;
    if (i >= ((C == 0) ? NC : P1) || j >= ((C == 1) ? NC : P1)) continue;
    const double *TV = (C == 1) ? Bc2 : Bo2, *TD = (C == 1) ? Gc2 : Bo2;
    double v = 0.0, d = 0.0;
    for (int qy = 0; qy < Q1; qy++) {
      v += TV[qy * NC + j] * Af[((C * 2 + 0) * NC + i) * Q1 * Q1 + qy + Q1 * qz];
      d += TD[qy * NC + j] * Af[((C * 2 + 1) * NC + i) * Q1 * Q1 + qy + Q1 * qz];
    }
    Bf[(((C * 2 + 0) * NC + i) * NC + j) * Q1 + qz] = v, Bf[(((C * 2 + 1) * NC + i) * NC + j) * Q1 + qz] = d;
  }
  __syncthreads();
  // along z, one thread per local dof (sorted order)
  for (int m = threadIdx.x; m < P; m += blockDim.x) {
    const int l = a.perm[(size_t)e * P + m];
    const int C = l / NB, r = l - C * NB;
    const int ni = (C == 0) ? NC : P1, nj = (C == 1) ? NC : P1;
    const int i = r % ni, j = (r / ni) % nj, k = r / (ni * nj);
    const double *TV = (C == 2) ? Bc2 : Bo2, *TD = (C == 2) ? Gc2 : Bo2;
    double acc = 0.0;
    for (int qz = 0; qz < Q1; qz++)
      acc += TV[qz * NC + k] * Bf[(((C * 2 + 0) * NC + i) * NC + j) * Q1 + qz] +
             TD[qz * NC + k] * Bf[(((C * 2 + 1) * NC + i) * NC + j) * Q1 + qz];
    // the gather applies the orientation sign of the entry: the diagonal does not have one
    a.ye[(size_t)e * P + m] = a.sidx[(size_t)e * P + m] >= 0 ? acc : -acc;
  }
}

void launch_rt_hex_diag(const SubOp &so, double *diag, hipStream_t s) {
  PA_REQUIRE(so.d_ye && so.d_tptr && so.d_perm, "H(div) blocks use the gather form of E^T");
  PA_REQUIRE(hex_pq_supported(so.p, so.q1d) || hex_q6_supported(so.p, so.q1d), "no H(div) hex kernel for this order and quadrature rule");
  RTDiagArgs a{};
  a.ne = so.ne, a.p = so.p, a.q1 = so.q1d;
  a.sidx = so.d_sidx, a.perm = so.d_perm, a.ye = so.d_ye;
  a.geom = so.geom->d_geom;
  a.qdata = so.qd ? so.qd->d : nullptr;
  rt_terms(so, a.use_v, a.use_d, a.c_mass, a.c_div);
  const int nc = so.p + 1;
  a.Bo = so.d_tab, a.Bc = so.d_tab + so.q1d * so.p, a.Gc = a.Bc + so.q1d * nc;
  PA_REQUIRE((int)so.geom->w1.size() == so.q1d, "geometry data without its 1-D quadrature weights");
  for (int q = 0; q < so.q1d; q++) a.w1[q] = so.geom->w1[q];
  const size_t lds = sizeof(double) * (4 * (size_t)so.Q + 3 * so.q1d * nc + 6 * nc * so.q1d * so.q1d + 6 * nc * nc * so.q1d);
  hipLaunchKernelGGL(rt_hex_diag_kernel, dim3(so.ne), dim3(128), lds, s, a);
  PA_HIP(hipGetLastError());
  launch_et_gather_raw(so.lsize, so.d_tptr, so.d_tent, so.d_ye, diag, true, s);
}

}  // namespace pa
