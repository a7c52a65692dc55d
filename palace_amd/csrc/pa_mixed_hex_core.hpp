// Device helpers the two-space hexahedron kernels share (pa_mixed_hex.hip: one right-hand side / one pair of inputs;
// pa_mixed_hex2.hip: both parts of a complex field per launch; pa_mixed_hex_q6.hip: six points per direction): the half tables, the LDS layout, the value passes of one
// component, E of one space and the geometry rows of a point.  The mapping is described at the top of pa_mixed_hex.hip.
#pragma once

#include "pa_hex_core.hpp"

namespace pa {

namespace {

template <int P1, int Q1>
struct MHTab {
  static constexpr int QH = (Q1 + 1) / 2;  // mirror symmetry: whole half rows, pa_hex_core.hpp
  double Bo[QH * P1];
  double Bc[QH * (P1 + 1)];
};

// value table of a direction with N nodes: the closed one (N = P1 + 1) or the open one (N = P1)
template <int P1, int Q1, int N>
__device__ __forceinline__ double mh_val(const double *Bo, const double *Bc, const int q, const int i) {
  return N == P1 + 1 ? half_even<P1 + 1, Q1, true>(Bc, q, i) : half_even<P1, Q1, true>(Bo, q, i);
}

// LDS of one element: the dofs of the larger (Nedelec) element in tensor order, one field after pass X and one after pass Y
template <int P1, int Q1>
using MHLayout = HexLayout<P1, Q1, 3 * P1 * (P1 + 1) * (P1 + 1), 1, 1>;

constexpr int kMHWaves = 4;

// nodes per direction of component C and the offset of its dofs (tensor order, x fastest)
template <int P1, int C, bool OPEN>
struct MHComp {
  static constexpr int NC = P1 + 1;
  static constexpr int NL = OPEN ? P1 : NC;  // along C
  static constexpr int NT = OPEN ? NC : P1;  // along the other two
  static constexpr int NX = C == 0 ? NL : NT, NY = C == 1 ? NL : NT, NZ = C == 2 ? NL : NT;
  static constexpr int base = C * NL * NT * NT;
};
template <int P1, bool OPEN>
constexpr int mh_ndofs() {
  return 3 * MHComp<P1, 0, OPEN>::NL * MHComp<P1, 0, OPEN>::NT * MHComp<P1, 0, OPEN>::NT;
}

// Forward value passes of component C: dofs (LDS, tensor order) -> V[qz] of lane (qx, qy) = (ta, tb).  Tab: anything with the
// half tables Bo, Bc as arrays or pointers -- MHTab (kernel arguments) or the LDS view of pa_mixed_hex_q6.hip.
template <int P1, int Q1, int C, bool OPEN, class Tab>
__device__ __forceinline__ void mh_fwd_comp(const Tab &tab, double *sm, const int ta, const int tb, const bool lane_ok,
                                            double V[Q1]) {
  using L = MHLayout<P1, Q1>;
  using D = MHComp<P1, C, OPEN>;
  constexpr int NX = D::NX, NY = D::NY, NZ = D::NZ;
  const double *Bo = tab.Bo, *Bc = tab.Bc;
  // pass X, lane (j, k)
  {
    const bool act = ta < NY && tb < NZ;
    double u[NX];
#pragma unroll
    for (int i = 0; i < NX; i++) u[i] = act ? sm[D::base + i + NX * (ta + NY * tb)] : 0.0;
#pragma unroll
    for (int qx = 0; qx < Q1; qx++) {
      double v = 0.0;
#pragma unroll
      for (int i = 0; i < NX; i++) v += mh_val<P1, Q1, NX>(Bo, Bc, qx, i) * u[i];
      if (lane_ok && act) sm[L::ia(0, qx, ta, tb)] = v;
    }
  }
  wave_sync();
  // pass Y, lane (qx, k)
  {
    const bool act = tb < NZ;
    const int kk = act ? tb : 0;
    double s0[NY];
#pragma unroll
    for (int j = 0; j < NY; j++) s0[j] = sm[L::ia(0, ta, j, kk)];
#pragma unroll
    for (int qy = 0; qy < Q1; qy++) {
      double v = 0.0;
#pragma unroll
      for (int j = 0; j < NY; j++) v += mh_val<P1, Q1, NY>(Bo, Bc, qy, j) * s0[j];
      if (lane_ok && act) sm[L::ib(0, ta, qy, tb)] = v;
    }
  }
  wave_sync();
  // pass Z, lane (qx, qy)
  {
    double s0[NZ];
#pragma unroll
    for (int k = 0; k < NZ; k++) s0[k] = sm[L::ib(0, ta, tb, k)];
#pragma unroll
    for (int qz = 0; qz < Q1; qz++) {
      double v = 0.0;
#pragma unroll
      for (int k = 0; k < NZ; k++) v += mh_val<P1, Q1, NZ>(Bo, Bc, qz, k) * s0[k];
      V[qz] = v;
    }
  }
}

// Transposed value passes of component C: W[qz] of lane (qx, qy) -> the component's dofs in tensor order (LDS)
template <int P1, int Q1, int C, bool OPEN, class Tab>
__device__ __forceinline__ void mh_bwd_comp(const Tab &tab, double *sm, const int ta, const int tb, const bool lane_ok,
                                            const double W[Q1]) {
  using L = MHLayout<P1, Q1>;
  using D = MHComp<P1, C, OPEN>;
  constexpr int NX = D::NX, NY = D::NY, NZ = D::NZ;
  const double *Bo = tab.Bo, *Bc = tab.Bc;
  // Z^T, lane (qx, qy)
  {
#pragma unroll
    for (int k = 0; k < NZ; k++) {
      double v = 0.0;
#pragma unroll
      for (int qz = 0; qz < Q1; qz++) v += mh_val<P1, Q1, NZ>(Bo, Bc, qz, k) * W[qz];
      if (lane_ok) sm[L::ib(0, ta, tb, k)] = v;
    }
  }
  wave_sync();
  // Y^T, lane (qx, k)
  {
    const bool act = tb < NZ;
    const int kk = act ? tb : 0;
    double s0[Q1];
#pragma unroll
    for (int qy = 0; qy < Q1; qy++) s0[qy] = sm[L::ib(0, ta, qy, kk)];
#pragma unroll
    for (int j = 0; j < NY; j++) {
      double v = 0.0;
#pragma unroll
      for (int qy = 0; qy < Q1; qy++) v += mh_val<P1, Q1, NY>(Bo, Bc, qy, j) * s0[qy];
      if (lane_ok && act) sm[L::ia(0, ta, j, tb)] = v;
    }
  }
  wave_sync();
  // X^T, lane (j, k) -> dofs [i][j][k] of the component
  {
    const bool act = ta < NY && tb < NZ;
    const int jj = act ? ta : 0, kk = act ? tb : 0;
    double s0[Q1];
#pragma unroll
    for (int qx = 0; qx < Q1; qx++) s0[qx] = sm[L::ia(0, qx, jj, kk)];
#pragma unroll
    for (int i = 0; i < NX; i++) {
      double r = 0.0;
#pragma unroll
      for (int qx = 0; qx < Q1; qx++) r += mh_val<P1, Q1, NX>(Bo, Bc, qx, i) * s0[qx];
      if (lane_ok && act) sm[D::base + i + NX * (ta + NY * tb)] = r;
    }
  }
}

template <int P1, int Q1>
struct MHArgs {
  int ne;
  // apply: 1 = trial space, 2 = test space; error: first and second input
  const int32_t *sidx1, *sidx2;  // sorted-order signed index
  const uint16_t *perm1, *perm2; // tensor-order slot of sorted entry m
  const double *geom;            // [ne][11][Q]
  const double *x1, *x2;
  double *ye;                    // apply: E-vector of the test space [ne][P2]
  double *out;                   // error: [ne], the caller's element order
  const int32_t *eorder;         // caller's number of internal element e, or nullptr (same order)
  CoeffDev c1, c2;
  MHTab<P1, Q1> tab;
};

// E of one space: sorted-order gather staged through LDS into tensor order (orientation signs applied here)
template <int P, int T>
__device__ __forceinline__ void mh_gather(const int32_t *__restrict__ sidx, const uint16_t *__restrict__ perm,
                                          const double *__restrict__ x, const int e, const int t, const bool active, double *sm) {
  constexpr int NPL = (P + T - 1) / T;
#pragma unroll
  for (int r = 0; r < NPL; r++) {
    const int m = t + T * r;
    if (active && m < P) {
      const int s = sidx[(size_t)e * P + m];
      const double v = x[s >= 0 ? s : -1 - s];
      sm[perm[(size_t)e * P + m]] = s < 0 ? -v : v;
    }
  }
}

// the three components of one space at the lane's Q1 points
template <int P1, int Q1, bool OPEN, class Tab>
__device__ __forceinline__ void mh_forward(const Tab &tab, double *sm, const int ta, const int tb, const bool lane_ok,
                                           double V[3][Q1]) {
  mh_fwd_comp<P1, Q1, 0, OPEN>(tab, sm, ta, tb, lane_ok, V[0]);
  mh_fwd_comp<P1, Q1, 1, OPEN>(tab, sm, ta, tb, lane_ok, V[1]);
  mh_fwd_comp<P1, Q1, 2, OPEN>(tab, sm, ta, tb, lane_ok, V[2]);
}

// the geometry rows of point q of an element (g at the point's attribute): w detJ, adj(J)^T / detJ and J / detJ
__device__ __forceinline__ void mh_point(const double *g, const int Q, int &attr, double &wdetJ, double adj[9], double Jl[9]) {
  attr = (int)g[0];
  wdetJ = g[Q];
#pragma unroll
  for (int c = 0; c < 9; c++) adj[c] = g[(2 + c) * Q];
  adjJt33(adj, Jl);
}

}  // namespace

}  // namespace pa
