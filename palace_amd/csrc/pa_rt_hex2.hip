// Two right-hand sides per pass for the Raviart-Thomas hexahedron apply of pa_rt_hex.hip on packed D (gfx950, FP64): mass,
// div-div and div-div + mass, behind pa_op_mult2 / pa_op_mult2_essential_diag -- the operator inside the PCG of the complex
// flux projector.  Same mapping, LDS layout and passes (pa_rt_hex_core.hpp) as the one-vector kernel and per vector the same
// operations in the same order: each result equals the one-vector apply to the bit.  A translation unit of its own: the
// one-vector kernels compile to the code they had without it.
#include "pa_rt_hex_core.hpp"

namespace pa {

// ---- two right-hand sides per pass (packed D) -----------------------------------------------------------------------------
// y0 = A x0, y1 = A x1: the index words, the slot permutation and the packed D of the lane's points are read once, and the point
// values of both vectors are live through one D loop.  Each vector goes through the operations of rt_hex_apply_kernel in their
// order.
template <int P1, int Q1>
struct RTArgs2 : RTArgs<P1, Q1> {
  const double *x1;
  double *ye1;
};

template <int P1, int Q1, bool USE_V, bool USE_DIV>
__global__ __launch_bounds__(64 * kRTWaves, 2) void rt_hex_apply2_kernel(const RTArgs2<P1, Q1> a) {
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

  constexpr int NG = (USE_V ? 6 : 0) + (USE_DIV ? 1 : 0);
  double gd[Q1][NG];
  {
    const double *g = a.qdata + eg * NG * Q + ta + Q1 * tb;
#pragma unroll
    for (int qz = 0; qz < Q1; qz++)
#pragma unroll
      for (int c = 0; c < NG; c++) gd[qz][c] = g[c * Q + Q1 * Q1 * qz];
  }

  // E: the signed index and the slots once for both vectors (ld < 0: this lane has no entry r, or an essential one: zero)
  constexpr int NPL = (P + L::T - 1) / L::T;
  int lp[NPL], ld[NPL];
  bool neg[NPL], own[NPL];
#pragma unroll
  for (int r = 0; r < NPL; r++) {
    const int m = t + L::T * r;
    lp[r] = 0, ld[r] = -1, neg[r] = false, own[r] = active && m < P;
    if (own[r]) {
      const int s = a.sidx_in[(size_t)e * P + m];
      neg[r] = s < 0;
      const int d = s >= 0 ? s : -1 - s;
      lp[r] = a.perm[(size_t)e * P + m];
      ld[r] = (d & kEssBit) ? -1 : (d & ~kEssBit);
    }
  }
  auto gather = [&](const double *__restrict__ x) {
#pragma unroll
    for (int r = 0; r < NPL; r++)
      if (own[r]) {
        const double v = ld[r] < 0 ? 0.0 : x[ld[r]];
        sm[lp[r]] = neg[r] ? -v : v;
      }
  };
  auto dstage = [&](double(&V)[3][Q1], double(&DV)[Q1]) {
#pragma unroll
    for (int qz = 0; qz < Q1; qz++) {
      if (USE_V) sym_mv(&gd[qz][0], V[0][qz], V[1][qz], V[2][qz], V[0][qz], V[1][qz], V[2][qz]);
      if (USE_DIV) DV[qz] *= gd[qz][NG - 1];
    }
  };
  auto forward = [&](double(&V)[3][Q1], double(&DV)[Q1]) {
#pragma unroll
    for (int qz = 0; qz < Q1; qz++) DV[qz] = 0.0;
    rt_fwd_comp<P1, Q1, 0, USE_V, USE_DIV>(a.tab, sm, ta, tb, lane_ok, V[0], DV);
    rt_fwd_comp<P1, Q1, 1, USE_V, USE_DIV>(a.tab, sm, ta, tb, lane_ok, V[1], DV);
    rt_fwd_comp<P1, Q1, 2, USE_V, USE_DIV>(a.tab, sm, ta, tb, lane_ok, V[2], DV);
  };
  auto backward = [&](double(&V)[3][Q1], double(&DV)[Q1], double *__restrict__ ye) {
    rt_bwd_comp<P1, Q1, 0, USE_V, USE_DIV>(a.tab, sm, ta, tb, lane_ok, V[0], DV);
    rt_bwd_comp<P1, Q1, 1, USE_V, USE_DIV>(a.tab, sm, ta, tb, lane_ok, V[1], DV);
    rt_bwd_comp<P1, Q1, 2, USE_V, USE_DIV>(a.tab, sm, ta, tb, lane_ok, V[2], DV);
    wave_sync();
#pragma unroll
    for (int r = 0; r < NPL; r++)
      if (own[r]) ye[(size_t)e * P + t + L::T * r] = sm[lp[r]];
    wave_sync();
  };

  double V[2][3][Q1], DV[2][Q1];
  gather(a.x);
  wave_sync();
  forward(V[0], DV[0]);
  wave_sync();
  gather(a.x1);
  wave_sync();
  forward(V[1], DV[1]);
  wave_sync();
  dstage(V[0], DV[0]);
  dstage(V[1], DV[1]);
  backward(V[0], DV[0], a.ye);
  backward(V[1], DV[1], a.ye1);
}

struct RT2Call {
  const SubOp &so;
  const double *x0, *x1;
  bool masked;
  hipStream_t s;
};

template <int P1, int Q1>
static void rt_launch2_pq(const RT2Call &c) {
  using L = RTLayout<P1, Q1>;
  constexpr int QH = RTTab<P1, Q1>::QH, NC = P1 + 1;
  const SubOp &so = c.so;
  RTArgs2<P1, Q1> a{};
  a.ne = so.ne;
  a.sidx_in = (c.masked && so.d_sidx_bc) ? so.d_sidx_bc : so.d_sidx;
  a.perm = so.d_perm;
  a.geom = so.geom->d_geom;
  a.qdata = so.qd->d;
  a.x = c.x0, a.x1 = c.x1;
  a.ye = so.d_ye, a.ye1 = so.d_ye2;
  for (int i = 0; i < QH * P1; i++) a.tab.Bo[i] = so.Bo[i];
  for (int i = 0; i < QH * NC; i++) a.tab.Bc[i] = so.Bc[i], a.tab.Gc[i] = so.Gc[i];
  const int epb = kRTWaves * L::EPW;
  const dim3 grid((so.ne + epb - 1) / epb), block(64 * kRTWaves);
  const size_t lds = sizeof(double) * (size_t)epb * L::ELEM_PAD;
  switch (so.qf) {
    case PA_QF_HDIV_33: hipLaunchKernelGGL((rt_hex_apply2_kernel<P1, Q1, true, false>), grid, block, lds, c.s, a); break;
    case PA_QF_L2_1: hipLaunchKernelGGL((rt_hex_apply2_kernel<P1, Q1, false, true>), grid, block, lds, c.s, a); break;
    case PA_QF_L2MASS_33: hipLaunchKernelGGL((rt_hex_apply2_kernel<P1, Q1, true, true>), grid, block, lds, c.s, a); break;
    default: throw Error("QFunction not available for H(div) hexahedra");
  }
  PA_HIP(hipGetLastError());
}

// The pairs the two-vector kernel is compiled for.  None has scratch or SGPR spills (profiles/r11_two_part_resources.txt): at
// orders 3 and 4 with five points per direction the three tables and the second pair of pointers no longer fit the scalar
// registers, and those blocks keep two applies.
// c == nullptr: only the question whether the pair is compiled in.
static bool rt_apply2_case(const int p, const int q1d, const RT2Call *c) {
#define PA_RT2_CASE(P, Q1D)           \
  case P * 16 + Q1D:                  \
    if (c) rt_launch2_pq<P, Q1D>(*c); \
    return true;
  switch (p * 16 + q1d) {
    PA_RT2_CASE(1, 2) PA_RT2_CASE(1, 3) PA_RT2_CASE(2, 3) PA_RT2_CASE(1, 4) PA_RT2_CASE(2, 4)
    PA_RT2_CASE(3, 4) PA_RT2_CASE(1, 5) PA_RT2_CASE(2, 5)
  }
#undef PA_RT2_CASE
  return false;
}

bool rt_hex_supports_two_rhs(const SubOp &so) {
  return so.fe_type == PA_FE_HDIV && so.qd && so.d_ye && two_part_enabled() && rt_apply2_case(so.p, so.q1d, nullptr);
}

// writes the E-vectors so.d_ye and so.d_ye2; the caller follows with the gathers
void launch_rt_hex_apply2(SubOp &so, const double *x0, const double *x1, bool masked, hipStream_t s) {
  PA_REQUIRE(rt_hex_supports_two_rhs(so), "no two-vector kernel for this H(div) block");
  PA_REQUIRE(!masked || so.d_sidx_bc, "pa_op_set_essential has not been called");
  if (!so.d_ye2) so.d_ye2 = dev_alloc<double>((size_t)so.ne * so.P);
  const RT2Call c{so, x0, x1, masked, s};
  rt_apply2_case(so.p, so.q1d, &c);
}

}  // namespace pa
