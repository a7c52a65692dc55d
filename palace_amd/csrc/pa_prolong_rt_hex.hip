// p-prolongation RT(p_c) -> RT(p_f) on tensor hexahedra and its transpose: the transfer of a Raviart-Thomas p-multigrid hierarchy
// (the `rt_fespaces` hierarchy of the reference's gradient flux estimator, linalg/errorestimator.cpp:67-104, 272-280).
//
// Replaces the libCEED interpolator operator Palace builds for two Raviart-Thomas spaces (reference fem/bilinearform.cpp:203-282,
// fem/libceed/basis.cpp:116-165).  With the nodal tensor bases of fem/rthex.py the element matrix is a Kronecker product of the
// two 1-D matrices pa_interp_create takes: RT component c is closed along direction c and open along the other two, so
//     P_c = Ic along c  (x)  Io along the other two directions,
// Ic [p_f+1][p_c+1] the coarse closed Gauss-Lobatto basis at the fine closed nodes and Io [p_f][p_c] the coarse open
// Gauss-Legendre basis at the fine open nodes: the mirror image of the Nedelec block of interp_kernel_s (pa_interp.hip).
//
// Mapping as there: (p_f+1)^2 lanes per element, 64 / (p_f+1)^2 elements per wave, four waves per block, three line passes per
// component with hand-offs through LDS inside the wave, no workgroup barrier.  The memory side of the three component blocks is
// issued up front: every index word, then every input value, then the passes block by block, then the stores.  Forward stores
// the owner copy of every fine dof (kRtpOwnBit in the fine index array, set by InterpOperator; all copies are equal): no
// atomics, no memset.  The transpose reads the fine vector through the same mask and writes the coarse E-vector, which
// InterpOperator's gather sums in its fixed order: the same bits on every call.
#include "linalg.hpp"
#include "pa_device.hpp"

namespace palace {

namespace {

constexpr int kMaxN = 6;             // closed nodes per direction (p_f <= 5)
constexpr int kRtpOwnBit = 1 << 29;  // InterpOperator's owner flag (pa_interp.hip: kOwnBit)
constexpr int kIcMax = 30, kIoMax = 20;  // (p_f+1)(p_c+1) <= 6 * 5, p_f p_c <= 5 * 4

struct RtpArgs {
  int ne, pc, pf;
  const int32_t *lidx_c, *lidx_f;  // signed tensor-order index arrays [ne][P_c], [ne][P_f] (fine: owner flag)
  const double *x;
  double *y;                // forward: fine L-vector; transpose: coarse E-vector [ne][P_c]
  double Ic[20], Io[12];    // by value for the specialised forms (p_f <= 4): scalar operands
  const double *Ic_dev, *Io_dev;  // the same on the device: the generic form keeps them in LDS
};

using pa::wave_sync;

// nodes of a component block along one direction: closed (p + 1) along the component's own direction, open (p) elsewhere
__device__ __forceinline__ constexpr int rtp_n(const int p, const bool closed) { return closed ? p + 1 : p; }

// entry k of the 1-D matrix of a direction: Ic (closed) or Io (open); SPEC: from the kernel arguments, else from the wave's LDS copy
template <bool SPEC, bool CLOSED>
__device__ __forceinline__ double rtp_m(const RtpArgs &a, const double *sM, const int k) {
  if constexpr (SPEC) return CLOSED ? a.Ic[k] : a.Io[k];
  else return sM[(CLOSED ? 0 : kIcMax) + k];
}

// PC, PF > 0: the orders at compile time (loops unrolled, lines in registers); 0: any orders up to kMaxN - 1 from the arguments.
// Line buffers hold NC coarse / NF fine entries, loops run over them with the order as a guard.
template <int PC, int PF>
struct RtpLine {
  static constexpr int NC = PC > 0 ? PC + 1 : kMaxN - 1, NF = PF > 0 ? PF + 1 : kMaxN;
};

// (A) forward: the signed coarse index words of the lane's line along direction 0 (lane = (i1, i2) of the coarse block) and the
// fine index words of its output line along direction 2 (lane = (i0, i1) of the fine block)
template <int PC, int PF, int C>
__device__ __forceinline__ void rtp_idx_fwd(const RtpArgs &a, const int pc, const int pf, const size_t e, const bool active, const int ta,
                                            const int tb, int (&sc)[RtpLine<PC, PF>::NC], int (&sf)[RtpLine<PC, PF>::NF]) {
  constexpr int NC = RtpLine<PC, PF>::NC, NF = RtpLine<PC, PF>::NF;
  const int nc0 = rtp_n(pc, C == 0), nc1 = rtp_n(pc, C == 1), nc2 = rtp_n(pc, C == 2);
  const int nf0 = rtp_n(pf, C == 0), nf1 = rtp_n(pf, C == 1), nf2 = rtp_n(pf, C == 2);
  const int bc = pc * pc * (pc + 1), bf = pf * pf * (pf + 1);
  const bool actc = active && ta < nc1 && tb < nc2, actf = active && ta < nf0 && tb < nf1;
#pragma unroll
  for (int i = 0; i < NC; i++) sc[i] = (actc && i < nc0) ? a.lidx_c[e * (3 * bc) + C * bc + i + nc0 * (ta + nc1 * tb)] : 0;
#pragma unroll
  for (int k = 0; k < NF; k++) sf[k] = (actf && k < nf2) ? a.lidx_f[e * (3 * bf) + C * bf + ta + nf0 * (tb + nf1 * k)] : 0;
}
// (B) forward: the signed coarse values
template <int PC, int PF, int C>
__device__ __forceinline__ void rtp_x_fwd(const RtpArgs &a, const int pc, const bool active, const int ta, const int tb,
                                          const int (&sc)[RtpLine<PC, PF>::NC], double (&u)[RtpLine<PC, PF>::NC]) {
  constexpr int NC = RtpLine<PC, PF>::NC;
  const int nc0 = rtp_n(pc, C == 0), nc1 = rtp_n(pc, C == 1), nc2 = rtp_n(pc, C == 2);
  const bool act = active && ta < nc1 && tb < nc2;
#pragma unroll
  for (int i = 0; i < NC; i++) {
    const int s = sc[i];
    const double xv = (act && i < nc0) ? a.x[s >= 0 ? s : -1 - s] : 0.0;
    u[i] = s >= 0 ? xv : -xv;
  }
}
// (C, D) forward: the passes along directions 0, 1, 2 and the owner stores
template <int PC, int PF, int C>
__device__ __forceinline__ void rtp_apply_fwd(const RtpArgs &a, const int pc, const int pf, const bool active, const bool lane_ok,
                                              const int ta, const int tb, double *sm, const double *sM,
                                              const double (&uin)[RtpLine<PC, PF>::NC], const int (&sf)[RtpLine<PC, PF>::NF]) {
  constexpr int NC = RtpLine<PC, PF>::NC, NF = RtpLine<PC, PF>::NF;
  constexpr bool S = PF > 0;
  const int nc0 = rtp_n(pc, C == 0), nc1 = rtp_n(pc, C == 1), nc2 = rtp_n(pc, C == 2);
  const int nf0 = rtp_n(pf, C == 0), nf1 = rtp_n(pf, C == 1), nf2 = rtp_n(pf, C == 2);
  const int n1 = pf + 1;
  double *sA = sm, *sB = sm + n1 * n1 * n1;
  {  // lane (i1, i2) coarse -> fine i0
    const bool act = lane_ok && ta < nc1 && tb < nc2;
#pragma unroll
    for (int fi = 0; fi < NF; fi++) {
      if (fi < nf0) {
        double v = 0.0;
#pragma unroll
        for (int i = 0; i < NC; i++)
          if (i < nc0) v += rtp_m<S, C == 0>(a, sM, fi * nc0 + i) * uin[i];
        if (act) sA[(fi * nc1 + ta) * nc2 + tb] = v;
      }
    }
  }
  wave_sync();
  {  // lane (i0 fine, i2 coarse) -> fine i1
    const bool act = lane_ok && ta < nf0 && tb < nc2;
    double u[NC];
#pragma unroll
    for (int j = 0; j < NC; j++) u[j] = j < nc1 ? sA[((act ? ta : 0) * nc1 + j) * nc2 + (act ? tb : 0)] : 0.0;
#pragma unroll
    for (int fj = 0; fj < NF; fj++) {
      if (fj < nf1) {
        double v = 0.0;
#pragma unroll
        for (int j = 0; j < NC; j++)
          if (j < nc1) v += rtp_m<S, C == 1>(a, sM, fj * nc1 + j) * u[j];
        if (act) sB[(ta * nf1 + fj) * nc2 + tb] = v;
      }
    }
  }
  wave_sync();
  {  // lane (i0, i1) fine -> fine i2, owner copy stored
    const bool act = ta < nf0 && tb < nf1;
    double u[NC];
#pragma unroll
    for (int k = 0; k < NC; k++) u[k] = k < nc2 ? sB[((act ? ta : 0) * nf1 + (act ? tb : 0)) * nc2 + k] : 0.0;
#pragma unroll
    for (int fk = 0; fk < NF; fk++) {
      if (fk < nf2) {
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < NC; k++)
          if (k < nc2) v += rtp_m<S, C == 2>(a, sM, fk * nc2 + k) * u[k];
        if (active && act) {
          const int s = sf[fk];
          const int g = s >= 0 ? s : -1 - s;
          if (g & kRtpOwnBit) a.y[g & ~kRtpOwnBit] = s >= 0 ? v : -v;
        }
      }
    }
  }
  wave_sync();  // (sA is the next component's)
}

// (A) transpose: the fine index words of the lane's line along direction 2
template <int PC, int PF, int C>
__device__ __forceinline__ void rtp_idx_tr(const RtpArgs &a, const int pf, const size_t e, const bool active, const int ta, const int tb,
                                           int (&sf)[RtpLine<PC, PF>::NF]) {
  constexpr int NF = RtpLine<PC, PF>::NF;
  const int nf0 = rtp_n(pf, C == 0), nf1 = rtp_n(pf, C == 1), nf2 = rtp_n(pf, C == 2);
  const int bf = pf * pf * (pf + 1);
  const bool act = active && ta < nf0 && tb < nf1;
#pragma unroll
  for (int k = 0; k < NF; k++) sf[k] = (act && k < nf2) ? a.lidx_f[e * (3 * bf) + C * bf + ta + nf0 * (tb + nf1 * k)] : 0;
}
// (B) transpose: the owner-masked signed fine values
template <int PC, int PF, int C>
__device__ __forceinline__ void rtp_x_tr(const RtpArgs &a, const int pf, const bool active, const int ta, const int tb,
                                         const int (&sf)[RtpLine<PC, PF>::NF], double (&u)[RtpLine<PC, PF>::NF]) {
  constexpr int NF = RtpLine<PC, PF>::NF;
  const int nf0 = rtp_n(pf, C == 0), nf1 = rtp_n(pf, C == 1), nf2 = rtp_n(pf, C == 2);
  const bool act = active && ta < nf0 && tb < nf1;
#pragma unroll
  for (int k = 0; k < NF; k++) {
    const int s = sf[k];
    const int g = s >= 0 ? s : -1 - s;
    const double xv = (act && k < nf2 && (g & kRtpOwnBit)) ? a.x[g & ~kRtpOwnBit] : 0.0;
    u[k] = s >= 0 ? xv : -xv;
  }
}
// (C, D) transpose: the transposed passes along directions 2, 1, 0 and the lane's coarse line to the E-vector
template <int PC, int PF, int C>
__device__ __forceinline__ void rtp_apply_tr(const RtpArgs &a, const int pc, const int pf, const size_t e, const bool active,
                                             const bool lane_ok, const int ta, const int tb, double *sm, const double *sM,
                                             const double (&uin)[RtpLine<PC, PF>::NF]) {
  constexpr int NC = RtpLine<PC, PF>::NC, NF = RtpLine<PC, PF>::NF;
  constexpr bool S = PF > 0;
  const int nc0 = rtp_n(pc, C == 0), nc1 = rtp_n(pc, C == 1), nc2 = rtp_n(pc, C == 2);
  const int nf0 = rtp_n(pf, C == 0), nf1 = rtp_n(pf, C == 1), nf2 = rtp_n(pf, C == 2);
  const int n1 = pf + 1, bc = pc * pc * (pc + 1);
  double *sA = sm, *sB = sm + n1 * n1 * n1;
  {  // lane (i0, i1) fine: fine i2 -> coarse i2
    const bool act = lane_ok && ta < nf0 && tb < nf1;
#pragma unroll
    for (int k = 0; k < NC; k++) {
      if (k < nc2) {
        double v = 0.0;
#pragma unroll
        for (int fk = 0; fk < NF; fk++)
          if (fk < nf2) v += rtp_m<S, C == 2>(a, sM, fk * nc2 + k) * uin[fk];
        if (act) sB[(ta * nf1 + tb) * nc2 + k] = v;
      }
    }
  }
  wave_sync();
  {  // lane (i0 fine, i2 coarse): fine i1 -> coarse i1
    const bool act = lane_ok && ta < nf0 && tb < nc2;
    double u[NF];
#pragma unroll
    for (int fj = 0; fj < NF; fj++) u[fj] = fj < nf1 ? sB[((act ? ta : 0) * nf1 + fj) * nc2 + (act ? tb : 0)] : 0.0;
#pragma unroll
    for (int j = 0; j < NC; j++) {
      if (j < nc1) {
        double v = 0.0;
#pragma unroll
        for (int fj = 0; fj < NF; fj++)
          if (fj < nf1) v += rtp_m<S, C == 1>(a, sM, fj * nc1 + j) * u[fj];
        if (act) sA[(ta * nc1 + j) * nc2 + tb] = v;
      }
    }
  }
  wave_sync();
  {  // lane (i1, i2) coarse: fine i0 -> coarse i0, unsigned element vector stored
    const bool act = ta < nc1 && tb < nc2;
    double u[NF];
#pragma unroll
    for (int fi = 0; fi < NF; fi++) u[fi] = fi < nf0 ? sA[(fi * nc1 + (act ? ta : 0)) * nc2 + (act ? tb : 0)] : 0.0;
#pragma unroll
    for (int i = 0; i < NC; i++) {
      if (i < nc0) {
        double v = 0.0;
#pragma unroll
        for (int fi = 0; fi < NF; fi++)
          if (fi < nf0) v += rtp_m<S, C == 0>(a, sM, fi * nc0 + i) * u[fi];
        if (active && act) a.y[e * (3 * bc) + C * bc + i + nc0 * (ta + nc1 * tb)] = v;
      }
    }
  }
  wave_sync();
}

template <bool TRANSPOSE, int PC, int PF>
__global__ __launch_bounds__(256) void rt_prolong_kernel(const RtpArgs a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  constexpr int NC = RtpLine<PC, PF>::NC, NF = RtpLine<PC, PF>::NF;
  const int pc = PC > 0 ? PC : a.pc, pf = PF > 0 ? PF : a.pf, n1 = pf + 1, T = n1 * n1, EPW = 64 / T;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane / T, t = lane - sub * T;
  const int ta = t % n1, tb = t / n1;
  const bool lane_ok = sub < EPW;
  const int el = (blockIdx.x * 4 + wave) * EPW + sub;
  const bool active = lane_ok && el < a.ne;
  const size_t e = (size_t)el;
  double *sm = smem + (size_t)(wave * EPW + (lane_ok ? sub : 0)) * (2 * n1 * n1 * n1);
  // generic form: the wave's copy of Ic and Io behind the element areas
  double *sM = smem + (size_t)(4 * EPW) * (2 * n1 * n1 * n1) + wave * (kIcMax + kIoMax);
  if (PF == 0) {
    if (lane < (pf + 1) * (pc + 1)) sM[lane] = a.Ic_dev[lane];
    if (lane < pf * pc) sM[kIcMax + lane] = a.Io_dev[lane];
    wave_sync();
  }
  if (!TRANSPOSE) {
    int sc0[NC], sc1[NC], sc2[NC], sf0[NF], sf1[NF], sf2[NF];
    double u0[NC], u1[NC], u2[NC];
    rtp_idx_fwd<PC, PF, 0>(a, pc, pf, e, active, ta, tb, sc0, sf0);
    rtp_idx_fwd<PC, PF, 1>(a, pc, pf, e, active, ta, tb, sc1, sf1);
    rtp_idx_fwd<PC, PF, 2>(a, pc, pf, e, active, ta, tb, sc2, sf2);
    rtp_x_fwd<PC, PF, 0>(a, pc, active, ta, tb, sc0, u0);
    rtp_x_fwd<PC, PF, 1>(a, pc, active, ta, tb, sc1, u1);
    rtp_x_fwd<PC, PF, 2>(a, pc, active, ta, tb, sc2, u2);
    rtp_apply_fwd<PC, PF, 0>(a, pc, pf, active, lane_ok, ta, tb, sm, sM, u0, sf0);
    rtp_apply_fwd<PC, PF, 1>(a, pc, pf, active, lane_ok, ta, tb, sm, sM, u1, sf1);
    rtp_apply_fwd<PC, PF, 2>(a, pc, pf, active, lane_ok, ta, tb, sm, sM, u2, sf2);
  } else {
    int sf0[NF], sf1[NF], sf2[NF];
    double u0[NF], u1[NF], u2[NF];
    rtp_idx_tr<PC, PF, 0>(a, pf, e, active, ta, tb, sf0);
    rtp_idx_tr<PC, PF, 1>(a, pf, e, active, ta, tb, sf1);
    rtp_idx_tr<PC, PF, 2>(a, pf, e, active, ta, tb, sf2);
    rtp_x_tr<PC, PF, 0>(a, pf, active, ta, tb, sf0, u0);
    rtp_x_tr<PC, PF, 1>(a, pf, active, ta, tb, sf1, u1);
    rtp_x_tr<PC, PF, 2>(a, pf, active, ta, tb, sf2, u2);
    rtp_apply_tr<PC, PF, 0>(a, pc, pf, e, active, lane_ok, ta, tb, sm, sM, u0);
    rtp_apply_tr<PC, PF, 1>(a, pc, pf, e, active, lane_ok, ta, tb, sm, sM, u1);
    rtp_apply_tr<PC, PF, 2>(a, pc, pf, e, active, lane_ok, ta, tb, sm, sM, u2);
  }
}

}  // namespace

// The compiled pairs: S the specialised instantiations (p_f <= 4), G the pairs the generic form runs (p_f = 5).
#define PA_RT_PROLONG_LIST(S, G) S(1, 2) S(1, 3) S(2, 3) S(1, 4) S(2, 4) S(3, 4) G(1, 5) G(2, 5) G(3, 5) G(4, 5)

// lidx_f carries the owner flag on one copy of every fine dof; Ic [pf+1][pc+1], Io [pf][pc] on the host and on the device; out: the
// fine L-vector (forward) or the coarse E-vector [ne][3 pc^2 (pc+1)] (transpose)
void launch_rt_prolong_hex(const bool transpose, const int pc, const int pf, const int ne, const int32_t *lidx_c, const int32_t *lidx_f,
                           const double *Ic, const double *Io, const double *Ic_dev, const double *Io_dev, const double *x, double *out,
                           hipStream_t stream) {
  PA_REQUIRE(pc >= 1 && pc < pf && pf + 1 <= kMaxN, "Raviart-Thomas prolongation: orders 1 <= p_c < p_f <= 5");
  PA_REQUIRE(Ic && Io && Ic_dev && Io_dev, "Raviart-Thomas prolongation: 1-D interpolation matrices missing");
  RtpArgs a{ne, pc, pf, lidx_c, lidx_f, x, out, {}, {}, Ic_dev, Io_dev};
  if (pf <= 4) {
    for (int k = 0; k < (pf + 1) * (pc + 1); k++) a.Ic[k] = Ic[k];
    for (int k = 0; k < pf * pc; k++) a.Io[k] = Io[k];
  }
  const int n1 = pf + 1, epb = 4 * (64 / (n1 * n1));
  const size_t lds = sizeof(double) * ((size_t)epb * 2 * n1 * n1 * n1 + (pf > 4 ? 4 * (kIcMax + kIoMax) : 0));
  const dim3 grid((ne + epb - 1) / epb), block(256);
  bool done = false;
#define PA_RT_PROLONG_CASE(PC, PF)                                                                        \
  if (pc == PC && pf == PF) {                                                                             \
    if (transpose) hipLaunchKernelGGL((rt_prolong_kernel<true, PC, PF>), grid, block, lds, stream, a);    \
    else hipLaunchKernelGGL((rt_prolong_kernel<false, PC, PF>), grid, block, lds, stream, a);             \
    done = true;                                                                                          \
  }
#define PA_RT_PROLONG_GENERIC(PC, PF)                                                                     \
  if (pc == PC && pf == PF) {                                                                             \
    if (transpose) hipLaunchKernelGGL((rt_prolong_kernel<true, 0, 0>), grid, block, lds, stream, a);      \
    else hipLaunchKernelGGL((rt_prolong_kernel<false, 0, 0>), grid, block, lds, stream, a);               \
    done = true;                                                                                          \
  }
  PA_RT_PROLONG_LIST(PA_RT_PROLONG_CASE, PA_RT_PROLONG_GENERIC)
#undef PA_RT_PROLONG_CASE
#undef PA_RT_PROLONG_GENERIC
  PA_REQUIRE(done, "Raviart-Thomas prolongation: no kernel for this pair of orders");
  PA_HIP(hipGetLastError());
}

}  // namespace palace
