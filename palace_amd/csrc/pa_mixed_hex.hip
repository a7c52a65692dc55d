// Sum-factorised two-space forms on tensor-product hexahedra (gfx950, FP64): one Nedelec and one Raviart-Thomas space of the
// same order on the same elements and rule -- the pieces of the flux error estimators (linalg/errorestimator.cpp) that
// pa_mixed.hip runs with dense tables:
//
//  * mixed mass  (v, C u),  H(curl) trial -> H(div) test (f_apply_hcurlhdiv_33) or the other way round (f_apply_hdivhcurl_33;
//    fem/qfunctions/33/hcurlhdiv_33_qf.h:10-54, chosen by fem/integ/vecfemass.cpp:88-101): FluxProjector's `Flux` operator;
//  * element error  eta_e^2 += int_e |C_2 u_2 - C_1 u_1|^2  (f_apply_hcurlhdiv_error_33 / f_apply_hdivhcurl_error_33,
//    fem/qfunctions/33/hcurlhdiv_error_33_qf.h:10-78, through AssembleCeedElementErrorIntegrator, fem/libceed/integrator.cpp:550-626).
//
// Elements: component c of the order-p Nedelec element is open (Gauss-Legendre, p nodes) along c and closed (Gauss-Lobatto,
// p + 1 nodes) along the other two directions; the Raviart-Thomas element (fem/rthex.py) is the other way round.  Only values
// enter, so a pass of component c differs between the two in nothing but which directions read the open table: one pass,
// parameterised on that (OPEN: direction c is the open one).
//
// Mapping of pa_rt_hex.hip: Q1^2 lanes per element, 64 / Q1^2 elements per wave, four waves per block, passes X -> Y -> Z through
// LDS inside the wave (wave-level syncs only), lane (qx, qy) ends with its qz column.  E is the sorted signed gather of the input
// space(s) (d_sidx / d_perm), D pointwise and matrix-free from the 11 geometry rows (the adj(J)^T / detJ rows are the covariant
// map, J / detJ is recomputed from them for the contravariant one), E^T of the apply the E-vector of the test space + the
// fixed-order gather.  The error form sums a lane's column, then the Q1^2 lanes of the element in a fixed order, and one lane adds
// the result to the caller's entry of the element: no atomics.  Idle lanes of a partial wave read element 0 and store nothing.
#include "pa_mixed_hex_core.hpp"

namespace pa {

namespace {

// ND_IN: the trial space is the Nedelec one (f_apply_hcurlhdiv_33), else the Raviart-Thomas one (f_apply_hdivhcurl_33)
template <int P1, int Q1, bool ND_IN>
__global__ __launch_bounds__(64 * kMHWaves, 2) void mixed_hex_apply_kernel(const MHArgs<P1, Q1> a) {
  using L = MHLayout<P1, Q1>;
  constexpr int Q = Q1 * Q1 * Q1, PI = mh_ndofs<P1, ND_IN>(), PO = mh_ndofs<P1, !ND_IN>();
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane / L::T, t = lane - sub * L::T;
  const int ta = t % Q1, tb = t / Q1;
  const bool lane_ok = sub < L::EPW;
  const int e = (blockIdx.x * kMHWaves + wave) * L::EPW + sub;
  const bool active = lane_ok && e < a.ne;
  double *sm = smem + (size_t)(wave * L::EPW + (lane_ok ? sub : 0)) * L::ELEM_PAD;
  const size_t eg = active ? e : 0;  // idle lanes read element 0 and store nothing

  mh_gather<PI, L::T>(a.sidx1, a.perm1, a.x1, e, t, active, sm);
  wave_sync();
  double V[3][Q1];
  mh_forward<P1, Q1, ND_IN>(a.tab, sm, ta, tb, lane_ok, V);
  wave_sync();

  // ---- D (hcurlhdiv_33_qf.h): v = w detJ (J / detJ)^T C adj u  or  w detJ adj^T C (J / detJ) u
#pragma unroll
  for (int qz = 0; qz < Q1; qz++) {
    int attr;
    double wdetJ, adj[9], Jl[9], Cm[9];
    mh_point(a.geom + eg * 11 * Q + ta + Q1 * tb + Q1 * Q1 * qz, Q, attr, wdetJ, adj, Jl);
    coeff_unpack3(a.c1, attr, Cm);
    if (ND_IN)
      mult_AtBCx33(Jl, Cm, adj, V[0][qz], V[1][qz], V[2][qz], wdetJ, V[0][qz], V[1][qz], V[2][qz]);
    else
      mult_AtBCx33(adj, Cm, Jl, V[0][qz], V[1][qz], V[2][qz], wdetJ, V[0][qz], V[1][qz], V[2][qz]);
  }

  mh_bwd_comp<P1, Q1, 0, !ND_IN>(a.tab, sm, ta, tb, lane_ok, V[0]);
  mh_bwd_comp<P1, Q1, 1, !ND_IN>(a.tab, sm, ta, tb, lane_ok, V[1]);
  mh_bwd_comp<P1, Q1, 2, !ND_IN>(a.tab, sm, ta, tb, lane_ok, V[2]);
  wave_sync();
  // E^T, first half: out of LDS in the sorted order of the test space (coalesced).  The E-vector holds the unsigned element
  // results: the gather applies the orientation sign of the entry.
  constexpr int NPL = (PO + L::T - 1) / L::T;
#pragma unroll
  for (int r = 0; r < NPL; r++) {
    const int m = t + L::T * r;
    if (active && m < PO) a.ye[(size_t)e * PO + m] = sm[a.perm2[(size_t)e * PO + m]];
  }
}

// ND_FIRST: the first input is the Nedelec one (f_apply_hcurlhdiv_error_33), else the Raviart-Thomas one
template <int P1, int Q1, bool ND_FIRST>
__global__ __launch_bounds__(64 * kMHWaves, 2) void mixed_hex_error_kernel(const MHArgs<P1, Q1> a) {
  using L = MHLayout<P1, Q1>;
  constexpr int Q = Q1 * Q1 * Q1, T = L::T, PA = mh_ndofs<P1, ND_FIRST>(), PB = mh_ndofs<P1, !ND_FIRST>();
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane / T, t = lane - sub * T;
  const int ta = t % Q1, tb = t / Q1;
  const bool lane_ok = sub < L::EPW;
  const int e = (blockIdx.x * kMHWaves + wave) * L::EPW + sub;
  const bool active = lane_ok && e < a.ne;
  double *sm = smem + (size_t)(wave * L::EPW + (lane_ok ? sub : 0)) * L::ELEM_PAD;
  const size_t eg = active ? e : 0;  // idle lanes read element 0 and store nothing

  double V1[3][Q1], V2[3][Q1];
  mh_gather<PA, T>(a.sidx1, a.perm1, a.x1, e, t, active, sm);
  wave_sync();
  mh_forward<P1, Q1, ND_FIRST>(a.tab, sm, ta, tb, lane_ok, V1);
  wave_sync();
  mh_gather<PB, T>(a.sidx2, a.perm2, a.x2, e, t, active, sm);
  wave_sync();
  mh_forward<P1, Q1, !ND_FIRST>(a.tab, sm, ta, tb, lane_ok, V2);

  // ---- hcurlhdiv_error_33_qf.h: w detJ |C_2 M_2 u_2 - C_1 M_1 u_1|^2, M the covariant / contravariant map of each input
  // Both inputs' values are live here, and one point needs its 11 geometry rows and two 3 x 3 matrices on top: with the requests
  // of a whole column in flight the four- and five-point instantiations spilled up to 104 VGPRs.  The address of point qz is
  // therefore tied to the result of point qz - 2: two points in flight at a time.
  const size_t gq = eg * 11 * Q + ta + Q1 * tb;
  double ep[Q1];
#pragma unroll
  for (int qz = 0; qz < Q1; qz++) {
    size_t go = gq + Q1 * Q1 * qz;
    if (qz >= 2) asm volatile("" : "+v"(go) : "v"(ep[qz - 2]));
    int attr;
    double wdetJ, adj[9], Jl[9], C1[9], C2[9];
    mh_point(a.geom + go, Q, attr, wdetJ, adj, Jl);
    coeff_unpack3(a.c1, attr, C1);
    coeff_unpack3(a.c2, attr, C2);
    const double u1[3] = {V1[0][qz], V1[1][qz], V1[2][qz]}, u2[3] = {V2[0][qz], V2[1][qz], V2[2][qz]};
    double w1[3], w2[3];
    mult_BAx33(ND_FIRST ? adj : Jl, C1, u1, w1);
    mult_BAx33(ND_FIRST ? Jl : adj, C2, u2, w2);
    w2[0] -= w1[0], w2[1] -= w1[1], w2[2] -= w1[2];
    ep[qz] = wdetJ * (w2[0] * w2[0] + w2[1] * w2[1] + w2[2] * w2[2]);
  }
  double err = 0.0;  // the lane's column, bottom to top
#pragma unroll
  for (int qz = 0; qz < Q1; qz++) err += ep[qz];

  // sum over the T lanes of the element in a fixed order (the all-ones basis of integrator.cpp:560-574)
  double sum;
  if (T == 4 || T == 16) {  // the element's lanes are an aligned power-of-two group: butterfly
    sum = err;
#pragma unroll
    for (int m = T / 2; m >= 1; m >>= 1) sum += __shfl_xor(sum, m, 64);
  } else if (T == 9) {  // lane by lane, every lane of the wave taking part in each exchange
    sum = 0.0;
    const int first = lane - t;
#pragma unroll
    for (int i = 0; i < T; i++) sum += __shfl(err, min(first + i, 63), 64);
  } else {  // 25 lanes: through the element's LDS (the dofs are no longer needed)
    wave_sync();
    if (lane_ok) sm[t] = err;
    wave_sync();
    sum = 0.0;
    if (t == 0)
      for (int i = 0; i < T; i++) sum += sm[i];
  }
  // one writer per element; the estimates are in the caller's element order
  if (active && t == 0) a.out[a.eorder ? a.eorder[e] : e] += sum;
}

template <int P1, int Q1>
void mh_launch_pq(const SubOp &so, const SubOp &s2, const MixedSub &ms, const int kind, const double *x1, const double *x2,
                  double *out, hipStream_t s) {
  using L = MHLayout<P1, Q1>;
  constexpr int QH = MHTab<P1, Q1>::QH, NC = P1 + 1;
  MHArgs<P1, Q1> a{};
  a.ne = ms.ne;
  a.sidx1 = so.d_sidx, a.perm1 = so.d_perm, a.sidx2 = s2.d_sidx, a.perm2 = s2.d_perm;
  a.geom = ms.geom->d_geom;
  a.x1 = x1, a.x2 = x2, a.ye = s2.d_ye, a.out = out, a.eorder = ms.d_eorder;
  a.c1 = ms.c0.dev(), a.c2 = ms.c1.dev();
  for (int i = 0; i < QH * P1; i++) a.tab.Bo[i] = so.Bo[i];
  for (int i = 0; i < QH * NC; i++) a.tab.Bc[i] = so.Bc[i];
  const int epb = kMHWaves * L::EPW;
  const dim3 grid((ms.ne + epb - 1) / epb), block(64 * kMHWaves);
  const size_t lds = sizeof(double) * (size_t)epb * L::ELEM_PAD;
  switch (kind) {
    case 0: hipLaunchKernelGGL((mixed_hex_apply_kernel<P1, Q1, true>), grid, block, lds, s, a); break;
    case 1: hipLaunchKernelGGL((mixed_hex_apply_kernel<P1, Q1, false>), grid, block, lds, s, a); break;
    case 2: hipLaunchKernelGGL((mixed_hex_error_kernel<P1, Q1, true>), grid, block, lds, s, a); break;
    case 3: hipLaunchKernelGGL((mixed_hex_error_kernel<P1, Q1, false>), grid, block, lds, s, a); break;
    default: throw Error("not a mixed-space QFunction");
  }
  PA_HIP(hipGetLastError());
}

}  // namespace

// transpose (apply only): the two spaces change places and W^T is the other member of the QFunction pair with the transposed
// coefficient, which CoeffHost::dev() hands out inside the TransposeScope of pa_op_mult_transpose (pa_mixed.hip: launch)
void launch_mixed_hex(const MixedSub &ms, const double *x1, const double *x2, double *out, hipStream_t s, bool transpose) {
  PA_REQUIRE(ms.hex1 && ms.hex2, "not a tensor-product two-space operator");
  PA_REQUIRE(!transpose || !ms.error, "error integrators have no transposed form");
  const SubOp &so = transpose ? *ms.hex2 : *ms.hex1, &s2 = transpose ? *ms.hex1 : *ms.hex2;
  const int kind = !transpose ? ms.kind : 1 - ms.kind;
  PA_REQUIRE(ms.error || s2.d_ye, "two-space blocks use the gather form of E^T");
  if (so.q1d == 6) return launch_mixed_hex_q6(so, s2, ms, kind, x1, x2, out, s);  // six points per direction: pa_mixed_hex_q6.hip
  PA_HEX_DISPATCH(mh_launch_pq, "H(curl) - H(div)", so, s2, ms, kind, x1, x2, out, s)
}

}  // namespace pa
