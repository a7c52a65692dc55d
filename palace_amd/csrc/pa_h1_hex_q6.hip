// Fused E -> B/G -> D -> B^T/G^T for H1 hexahedra at six points per direction (gfx950, FP64): the pairs of PA_HEX_Q6_LIST --
// diffusion, mass and diffusion + mass, packed or matrix-free D, for the Hiptmair smoother and AMS of an order-5 hierarchy.
// The chain and the pass order are those of pa_h1_hex.hip; the fit to the machine is that of pa_nd_hex_q6.hip: one element
// per wave (lanes 36 ... 63 leave at once), the 1-D tables in the wave's LDS strip instead of kernel arguments, the D stage
// point by point along qz with the next point's data requested one point ahead, E^T as the E-vector + gather form.
#include "pa_hex_core.hpp"

namespace pa {

constexpr int kH1Q6Waves = 4;

template <int P1, int Q1>
struct H1Q6Args {
  int ne;
  const int32_t *sidx_in;  // sorted-order index (pa_nd_hex.hip), kEssBit = read as zero
  const uint16_t *perm;    // tensor-order slot of sorted entry m
  const double *geom;
  const double *qdata;
  const double *x;
  double *ye;
  CoeffDev c_mass, c_diff;
  const double *tab;  // the operator's device tables [Bo (unused) | Bc | Gc], full rows
};

// LDS of one wave: the contraction buffers of its element (H1Layout), then its copy of Bc and Gc
template <int P1, int Q1>
struct H1Q6Strip {
  static constexpr int ELEM = H1Layout<P1, Q1>::ELEM_PAD;
  static constexpr int TAB = 2 * Q1 * (P1 + 1);
  static constexpr int STRIDE = ELEM + TAB;
};

// USE_V: mass term, USE_G: diffusion term; QD: packed pre-assembled D (mass: 1 double, diffusion: 6)
template <int P1, int Q1, bool USE_V, bool USE_G, bool QD>
__global__ __launch_bounds__(64 * kH1Q6Waves, 1) void h1_hex_q6_kernel(const H1Q6Args<P1, Q1> a) {
  using L = H1Layout<P1, Q1>;
  using S = H1Q6Strip<P1, Q1>;
  static_assert(L::EPW == 1, "one element per wave");
  constexpr int NC = L::NC, Q = Q1 * Q1 * Q1, P = NC * NC * NC;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int e = blockIdx.x * kH1Q6Waves + wave;
  if (e >= a.ne) return;     // the whole wave: waves never wait for each other
  if (lane >= L::T) return;  // the lanes without a line: no global access, no LDS store
  const int t = lane, ta = t % Q1, tb = t / Q1;
  double *__restrict__ sm = smem + (size_t)wave * S::STRIDE;
  for (int i = t; i < S::TAB; i += L::T) sm[S::ELEM + i] = a.tab[Q1 * P1 + i];  // (visible at the first wave_sync())
  const double *Bc = sm + S::ELEM, *Gc = Bc + Q1 * NC;

  // D-stage data of the first point of this lane's column, requested up front
  constexpr int NG = QD ? (USE_V ? 1 : 0) + (USE_G ? 6 : 0) : 10;
  const double *dsrc = (QD ? a.qdata + (size_t)e * NG * Q : a.geom + (size_t)e * 11 * Q) + t;
  double gd[2][NG];
  int attr[2] = {1, 1};
  auto load_point = [&](const int b, const int qz) {
    if (!QD) attr[b] = (int)dsrc[Q1 * Q1 * qz];
#pragma unroll
    for (int c = 0; c < NG; c++) gd[b][c] = dsrc[(QD ? c : 1 + c) * Q + Q1 * Q1 * qz];
  };
  load_point(0, 0);

  // E: sorted-order gather staged through LDS into tensor order
  constexpr int NPL = (P + L::T - 1) / L::T;
  int lp[NPL];
#pragma unroll
  for (int r = 0; r < NPL; r++) {
    const int m = t + L::T * r;
    lp[r] = 0;
    if (L::T * (r + 1) <= P || m < P) {  // (only the last round can be partial)
      const int s = a.sidx_in[(size_t)e * P + m];
      lp[r] = a.perm[(size_t)e * P + m];
      sm[lp[r]] = (s & kEssBit) ? 0.0 : a.x[s & ~kEssBit];
    }
  }
  wave_sync();
  const bool act_jk = ta < NC && tb < NC, act_k = tb < NC;
  double u[NC];
#pragma unroll
  for (int i = 0; i < NC; i++) u[i] = act_jk ? sm[i + NC * (ta + NC * tb)] : 0.0;
  wave_sync();

  double V[Q1], GV[3][Q1];
  // ---- forward: pass X, lane (j, k)
#pragma unroll
  for (int qx = 0; qx < Q1; qx++) {
    double v = 0.0, d = 0.0;
#pragma unroll
    for (int i = 0; i < NC; i++) {
      v += half_even<NC, Q1>(Bc, qx, i) * u[i];
      if (USE_G) d += half_odd<NC, Q1>(Gc, qx, i) * u[i];
    }
    if (act_jk) {
      sm[L::ia(0, qx, ta, tb)] = v;
      if (USE_G) sm[L::ia(1, qx, ta, tb)] = d;
    }
  }
  wave_sync();
  // pass Y, lane (qx, k)
  {
    double v[NC], d[NC];
#pragma unroll
    for (int j = 0; j < NC; j++) {
      v[j] = sm[L::ia(0, ta, j, act_k ? tb : 0)];
      if (USE_G) d[j] = sm[L::ia(1, ta, j, act_k ? tb : 0)];
    }
#pragma unroll
    for (int qy = 0; qy < Q1; qy++) {
      double vv = 0.0, vd = 0.0, dv = 0.0;
#pragma unroll
      for (int j = 0; j < NC; j++) {
        vv += half_even<NC, Q1>(Bc, qy, j) * v[j];
        if (USE_G) vd += half_odd<NC, Q1>(Gc, qy, j) * v[j];
        if (USE_G) dv += half_even<NC, Q1>(Bc, qy, j) * d[j];
      }
      if (act_k) {
        sm[L::ib(0, ta, qy, tb)] = vv;
        if (USE_G) sm[L::ib(1, ta, qy, tb)] = vd, sm[L::ib(2, ta, qy, tb)] = dv;
      }
    }
  }
  wave_sync();
  // pass Z, lane (qx, qy)
  {
    double vv[NC], vd[NC], dv[NC];
#pragma unroll
    for (int k = 0; k < NC; k++) {
      vv[k] = sm[L::ib(0, ta, tb, k)];
      if (USE_G) vd[k] = sm[L::ib(1, ta, tb, k)], dv[k] = sm[L::ib(2, ta, tb, k)];
    }
#pragma unroll
    for (int qz = 0; qz < Q1; qz++) {
      double val = 0.0, dz = 0.0, dy = 0.0, dx = 0.0;
#pragma unroll
      for (int k = 0; k < NC; k++) {
        if (USE_V) val += half_even<NC, Q1>(Bc, qz, k) * vv[k];
        if (USE_G) {
          dz += half_odd<NC, Q1>(Gc, qz, k) * vv[k];
          dy += half_even<NC, Q1>(Bc, qz, k) * vd[k];
          dx += half_even<NC, Q1>(Bc, qz, k) * dv[k];
        }
      }
      V[qz] = val, GV[0][qz] = dx, GV[1][qz] = dy, GV[2][qz] = dz;
    }
  }
  wave_sync();

  // ---- D (h1_1 / hcurl_33 on grad u / hcurlmass_33), point by point; the next point's data is on its way meanwhile
#pragma unroll
  for (int qz = 0; qz < Q1; qz++) {
    const int b = qz & 1;
    if (qz + 1 < Q1) load_point(b ^ 1, qz + 1);
    if (QD) {
      if (USE_V) V[qz] *= gd[b][0];
      if (USE_G) sym_mv(&gd[b][USE_V ? 1 : 0], GV[0][qz], GV[1][qz], GV[2][qz], GV[0][qz], GV[1][qz], GV[2][qz]);
    } else {
      const double wdetJ = gd[b][0];
      const double *adj = &gd[b][QD ? 0 : 1];
      if (USE_V) V[qz] *= coeff_unpack1(a.c_mass, attr[b]) * wdetJ;
      if (USE_G) {
        double Cm[9];
        coeff_unpack3(a.c_diff, attr[b], Cm);
        mult_AtBCx33(adj, Cm, adj, GV[0][qz], GV[1][qz], GV[2][qz], wdetJ, GV[0][qz], GV[1][qz], GV[2][qz]);
      }
    }
    __builtin_amdgcn_sched_barrier(0);  // one point at a time: the loads stay one point ahead, no further
  }

  // ---- transposed passes: Z^T lane (qx, qy)
#pragma unroll
  for (int k = 0; k < NC; k++) {
    double vv = 0.0, vd = 0.0, dv = 0.0;
#pragma unroll
    for (int qz = 0; qz < Q1; qz++) {
      if (USE_V) vv += half_even<NC, Q1>(Bc, qz, k) * V[qz];
      if (USE_G) {
        vv += half_odd<NC, Q1>(Gc, qz, k) * GV[2][qz];
        vd += half_even<NC, Q1>(Bc, qz, k) * GV[1][qz];
        dv += half_even<NC, Q1>(Bc, qz, k) * GV[0][qz];
      }
    }
    sm[L::ib(0, ta, tb, k)] = vv;
    if (USE_G) sm[L::ib(1, ta, tb, k)] = vd, sm[L::ib(2, ta, tb, k)] = dv;
  }
  wave_sync();
  // Y^T lane (qx, k)
  {
    double vv[Q1], vd[Q1], dv[Q1];
#pragma unroll
    for (int qy = 0; qy < Q1; qy++) {
      vv[qy] = sm[L::ib(0, ta, qy, act_k ? tb : 0)];
      if (USE_G) vd[qy] = sm[L::ib(1, ta, qy, act_k ? tb : 0)], dv[qy] = sm[L::ib(2, ta, qy, act_k ? tb : 0)];
    }
#pragma unroll
    for (int j = 0; j < NC; j++) {
      double v = 0.0, d = 0.0;
#pragma unroll
      for (int qy = 0; qy < Q1; qy++) {
        v += half_even<NC, Q1>(Bc, qy, j) * vv[qy];
        if (USE_G) v += half_odd<NC, Q1>(Gc, qy, j) * vd[qy];
        if (USE_G) d += half_even<NC, Q1>(Bc, qy, j) * dv[qy];
      }
      if (act_k) {
        sm[L::ia(0, ta, j, tb)] = v;
        if (USE_G) sm[L::ia(1, ta, j, tb)] = d;
      }
    }
  }
  wave_sync();
  // X^T lane (j, k) -> E-vector [i][j + NC k]
  {
    double v[Q1], d[Q1];
#pragma unroll
    for (int qx = 0; qx < Q1; qx++) {
      v[qx] = sm[L::ia(0, qx, act_jk ? ta : 0, act_jk ? tb : 0)];
      if (USE_G) d[qx] = sm[L::ia(1, qx, act_jk ? ta : 0, act_jk ? tb : 0)];
    }
#pragma unroll
    for (int i = 0; i < NC; i++) {
      double r = 0.0;
#pragma unroll
      for (int qx = 0; qx < Q1; qx++) {
        r += half_even<NC, Q1>(Bc, qx, i) * v[qx];
        if (USE_G) r += half_odd<NC, Q1>(Gc, qx, i) * d[qx];
      }
      u[i] = r;
    }
  }
  wave_sync();
  // E^T, first half: results into tensor order in LDS, then out in sorted order (coalesced)
#pragma unroll
  for (int i = 0; i < NC; i++)
    if (act_jk) sm[i + NC * (ta + NC * tb)] = u[i];
  wave_sync();
#pragma unroll
  for (int r = 0; r < NPL; r++) {
    const int m = t + L::T * r;
    if (L::T * (r + 1) <= P || m < P) a.ye[(size_t)e * P + m] = sm[lp[r]];
  }
}

template <int P1, int Q1>
static void h1_q6_launch_pq(const SubOp &so, const double *x, bool masked, hipStream_t s) {
  H1Q6Args<P1, Q1> a;
  a.ne = so.ne;
  a.sidx_in = (masked && so.d_sidx_bc) ? so.d_sidx_bc : so.d_sidx;
  a.perm = so.d_perm;
  a.geom = so.geom->d_geom;
  a.qdata = so.qd ? so.qd->d : nullptr;
  a.x = x;
  a.ye = so.d_ye;
  a.tab = so.d_tab;
  const dim3 grid((so.ne + kH1Q6Waves - 1) / kH1Q6Waves), block(64 * kH1Q6Waves);
  const size_t lds = sizeof(double) * (size_t)kH1Q6Waves * H1Q6Strip<P1, Q1>::STRIDE;
  const bool qd = a.qdata != nullptr;
#define PA_H1Q6_LAUNCH(V, G)                                                                \
  if (qd)                                                                                   \
    hipLaunchKernelGGL((h1_hex_q6_kernel<P1, Q1, V, G, true>), grid, block, lds, s, a);     \
  else                                                                                      \
    hipLaunchKernelGGL((h1_hex_q6_kernel<P1, Q1, V, G, false>), grid, block, lds, s, a);
  bool use_v, use_g;
  h1_terms(so, use_v, use_g, a.c_mass, a.c_diff);
  if (!use_v) {
    PA_H1Q6_LAUNCH(false, true)
  } else if (!use_g) {
    PA_H1Q6_LAUNCH(true, false)
  } else {
    PA_H1Q6_LAUNCH(true, true)
  }
#undef PA_H1Q6_LAUNCH
  PA_HIP(hipGetLastError());
}

// writes the E-vector so.d_ye; the caller follows with launch_et_gather
void launch_h1_hex_q6(const SubOp &so, const double *x, bool masked, hipStream_t s) {
  PA_REQUIRE(so.d_tab, "1-D tables missing on the device");
  switch (so.p * 16 + so.q1d) {
    PA_HEX_Q6_LIST(PA_HEX_PQ_CALL, h1_q6_launch_pq, so, x, masked, s)
    default: throw hex_pq_error("H1", so.p, so.q1d);
  }
}

}  // namespace pa
