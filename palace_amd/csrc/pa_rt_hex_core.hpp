// Device helpers the Raviart-Thomas hexahedron kernels share (pa_rt_hex.hip: one right-hand side; pa_rt_hex2.hip: two per
// pass; pa_rt_hex_q6.hip: six points per direction): the half tables, the kernel arguments, the LDS layout and the forward / transposed passes of one component.  The
// element and the mapping are described at the top of pa_rt_hex.hip.
#pragma once

#include "pa_hex_core.hpp"

namespace pa {

template <int P1, int Q1>
struct RTTab {
  static constexpr int QH = (Q1 + 1) / 2;  // mirror symmetry: whole half rows, pa_hex_core.hpp
  double Bo[QH * P1];
  double Bc[QH * (P1 + 1)];
  double Gc[QH * (P1 + 1)];
};

// the tables are read with the second half of an odd rule's middle row mirrored (pa_hex_core.hpp)
template <int N, int Q1>
__device__ __forceinline__ double rt_even(const double *H, const int q, const int i) {
  return half_even<N, Q1, true>(H, q, i);
}
template <int N, int Q1>
__device__ __forceinline__ double rt_odd(const double *H, const int q, const int i) {
  return half_odd<N, Q1, true>(H, q, i);
}

template <int P1, int Q1>
struct RTArgs {
  int ne;
  const int32_t *sidx_in;  // sorted-order signed index; kEssBit (on the dof number) = read as zero
  const uint16_t *perm;    // tensor-order slot of sorted entry m
  const double *geom;      // [ne][11][Q]
  const double *qdata;     // [ne][ncomp][Q]: the six upper entries of (w / detJ) J^T C J, then c qw^2 / (w detJ)
  const double *x;
  double *ye;
  CoeffDev c_mass, c_div;
  double w1[Q1];  // 1-D quadrature weights (q_w of l2_1_qf.h)
  RTTab<P1, Q1> tab;
};

// LDS of one element: the P dofs in tensor order, then two fields after pass X [Q1][NC][NC] and two after pass Y
// [Q1][Q1][NC] (field 0: the chain of values, field 1: the chain of the divergence once the pass along c has split them)
template <int P1, int Q1>
using RTLayout = HexLayout<P1, Q1, 3 * P1 * P1 * (P1 + 1), 2, 2>;

constexpr int kRTWaves = 4;

// Forward passes of component C: dofs (LDS, tensor order) -> V[qz] (value, USE_V) and DV[qz] += divergence (USE_DIV) of
// lane (qx, qy) = (ta, tb).  Before the pass along C there is one chain (field 0); that pass splits it into the value (Bc,
// field 0) and the derivative (Gc, field 1); the passes after it apply Bo to both.  Tab: anything with the half tables Bo, Bc,
// Gc as arrays or pointers -- RTTab (kernel arguments) or the LDS view of pa_rt_hex_q6.hip.
template <int P1, int Q1, int C, bool USE_V, bool USE_DIV, class Tab>
__device__ __forceinline__ void rt_fwd_comp(const Tab &tab, double *sm, const int ta, const int tb, const bool lane_ok,
                                            double V[Q1], double DV[Q1]) {
  using L = RTLayout<P1, Q1>;
  constexpr int NC = L::NC;
  constexpr int NX = C == 0 ? NC : P1, NY = C == 1 ? NC : P1, NZ = C == 2 ? NC : P1;
  constexpr int base = C * P1 * P1 * NC;
  const double *Bo = tab.Bo, *Bc = tab.Bc, *Gc = tab.Gc;
  // pass X, lane (j, k)
  {
    const bool act = ta < NY && tb < NZ;
    double u[NX];
#pragma unroll
    for (int i = 0; i < NX; i++) u[i] = act ? sm[base + i + NX * (ta + NY * tb)] : 0.0;
#pragma unroll
    for (int qx = 0; qx < Q1; qx++) {
      double v = 0.0, d = 0.0;
#pragma unroll
      for (int i = 0; i < NX; i++) {
        if (C == 0) {
          if (USE_V) v += rt_even<NC, Q1>(Bc, qx, i) * u[i];
          if (USE_DIV) d += rt_odd<NC, Q1>(Gc, qx, i) * u[i];
        } else {
          v += rt_even<P1, Q1>(Bo, qx, i) * u[i];
        }
      }
      if (lane_ok && act) {
        if (C != 0 || USE_V) sm[L::ia(0, qx, ta, tb)] = v;
        if (C == 0 && USE_DIV) sm[L::ia(1, qx, ta, tb)] = d;
      }
    }
  }
  wave_sync();
  // pass Y, lane (qx, k)
  {
    const bool act = tb < NZ;
    const int kk = act ? tb : 0;
    double s0[NY], s1[NY];
#pragma unroll
    for (int j = 0; j < NY; j++) {
      s0[j] = (C != 0 || USE_V) ? sm[L::ia(0, ta, j, kk)] : 0.0;
      s1[j] = (C == 0 && USE_DIV) ? sm[L::ia(1, ta, j, kk)] : 0.0;
    }
#pragma unroll
    for (int qy = 0; qy < Q1; qy++) {
      double v = 0.0, d = 0.0;
#pragma unroll
      for (int j = 0; j < NY; j++) {
        if (C == 1) {
          if (USE_V) v += rt_even<NC, Q1>(Bc, qy, j) * s0[j];
          if (USE_DIV) d += rt_odd<NC, Q1>(Gc, qy, j) * s0[j];
        } else if (C == 0) {
          if (USE_V) v += rt_even<P1, Q1>(Bo, qy, j) * s0[j];
          if (USE_DIV) d += rt_even<P1, Q1>(Bo, qy, j) * s1[j];
        } else {
          v += rt_even<P1, Q1>(Bo, qy, j) * s0[j];
        }
      }
      if (lane_ok && act) {
        if (C == 2 || USE_V) sm[L::ib(0, ta, qy, tb)] = v;
        if (C != 2 && USE_DIV) sm[L::ib(1, ta, qy, tb)] = d;
      }
    }
  }
  wave_sync();
  // pass Z, lane (qx, qy)
  {
    double s0[NZ], s1[NZ];
#pragma unroll
    for (int k = 0; k < NZ; k++) {
      s0[k] = (C == 2 || USE_V) ? sm[L::ib(0, ta, tb, k)] : 0.0;
      s1[k] = (C != 2 && USE_DIV) ? sm[L::ib(1, ta, tb, k)] : 0.0;
    }
#pragma unroll
    for (int qz = 0; qz < Q1; qz++) {
      double v = 0.0, d = 0.0;
#pragma unroll
      for (int k = 0; k < NZ; k++) {
        if (C == 2) {
          if (USE_V) v += rt_even<NC, Q1>(Bc, qz, k) * s0[k];
          if (USE_DIV) d += rt_odd<NC, Q1>(Gc, qz, k) * s0[k];
        } else {
          if (USE_V) v += rt_even<P1, Q1>(Bo, qz, k) * s0[k];
          if (USE_DIV) d += rt_even<P1, Q1>(Bo, qz, k) * s1[k];
        }
      }
      V[qz] = v;
      if (USE_DIV) DV[qz] += d;
    }
  }
}

// Transposed passes of component C: W[qz] (the D stage's value output of this component) and DW[qz] (its divergence
// output) of lane (qx, qy) -> the component's dofs in tensor order (LDS).  The pass along C merges the two chains.
template <int P1, int Q1, int C, bool USE_V, bool USE_DIV, class Tab>
__device__ __forceinline__ void rt_bwd_comp(const Tab &tab, double *sm, const int ta, const int tb, const bool lane_ok,
                                            const double W[Q1], const double DW[Q1]) {
  using L = RTLayout<P1, Q1>;
  constexpr int NC = L::NC;
  constexpr int NX = C == 0 ? NC : P1, NY = C == 1 ? NC : P1, NZ = C == 2 ? NC : P1;
  constexpr int base = C * P1 * P1 * NC;
  const double *Bo = tab.Bo, *Bc = tab.Bc, *Gc = tab.Gc;
  // Z^T, lane (qx, qy)
  {
#pragma unroll
    for (int k = 0; k < NZ; k++) {
      double v = 0.0, d = 0.0;
#pragma unroll
      for (int qz = 0; qz < Q1; qz++) {
        if (C == 2) {
          if (USE_V) v += rt_even<NC, Q1>(Bc, qz, k) * W[qz];
          if (USE_DIV) v += rt_odd<NC, Q1>(Gc, qz, k) * DW[qz];
        } else {
          if (USE_V) v += rt_even<P1, Q1>(Bo, qz, k) * W[qz];
          if (USE_DIV) d += rt_even<P1, Q1>(Bo, qz, k) * DW[qz];
        }
      }
      if (lane_ok) {
        if (C == 2 || USE_V) sm[L::ib(0, ta, tb, k)] = v;
        if (C != 2 && USE_DIV) sm[L::ib(1, ta, tb, k)] = d;
      }
    }
  }
  wave_sync();
  // Y^T, lane (qx, k)
  {
    const bool act = tb < NZ;
    const int kk = act ? tb : 0;
    double s0[Q1], s1[Q1];
#pragma unroll
    for (int qy = 0; qy < Q1; qy++) {
      s0[qy] = (C == 2 || USE_V) ? sm[L::ib(0, ta, qy, kk)] : 0.0;
      s1[qy] = (C != 2 && USE_DIV) ? sm[L::ib(1, ta, qy, kk)] : 0.0;
    }
#pragma unroll
    for (int j = 0; j < NY; j++) {
      double v = 0.0, d = 0.0;
#pragma unroll
      for (int qy = 0; qy < Q1; qy++) {
        if (C == 1) {
          if (USE_V) v += rt_even<NC, Q1>(Bc, qy, j) * s0[qy];
          if (USE_DIV) v += rt_odd<NC, Q1>(Gc, qy, j) * s1[qy];
        } else if (C == 0) {
          if (USE_V) v += rt_even<P1, Q1>(Bo, qy, j) * s0[qy];
          if (USE_DIV) d += rt_even<P1, Q1>(Bo, qy, j) * s1[qy];
        } else {
          v += rt_even<P1, Q1>(Bo, qy, j) * s0[qy];
        }
      }
      if (lane_ok && act) {
        if (C != 0 || USE_V) sm[L::ia(0, ta, j, tb)] = v;
        if (C == 0 && USE_DIV) sm[L::ia(1, ta, j, tb)] = d;
      }
    }
  }
  wave_sync();
  // X^T, lane (j, k) -> dofs [i][j][k] of the component
  {
    const bool act = ta < NY && tb < NZ;
    const int jj = act ? ta : 0, kk = act ? tb : 0;
    double s0[Q1], s1[Q1];
#pragma unroll
    for (int qx = 0; qx < Q1; qx++) {
      s0[qx] = (C != 0 || USE_V) ? sm[L::ia(0, qx, jj, kk)] : 0.0;
      s1[qx] = (C == 0 && USE_DIV) ? sm[L::ia(1, qx, jj, kk)] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < NX; i++) {
      double r = 0.0;
#pragma unroll
      for (int qx = 0; qx < Q1; qx++) {
        if (C == 0) {
          if (USE_V) r += rt_even<NC, Q1>(Bc, qx, i) * s0[qx];
          if (USE_DIV) r += rt_odd<NC, Q1>(Gc, qx, i) * s1[qx];
        } else {
          r += rt_even<P1, Q1>(Bo, qx, i) * s0[qx];
        }
      }
      if (lane_ok && act) sm[base + i + NX * (ta + NY * tb)] = r;
    }
  }
}

}  // namespace pa
