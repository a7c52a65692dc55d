// Fused E -> B -> D -> B^T for Raviart-Thomas hexahedra at six points per direction (gfx950, FP64): the pairs (p, 6),
// p = 1 ... 5 of PA_HEX_Q6_LIST -- the order-5 H(div) mass, div-div and div-div + mass operators and the coarser levels of
// an order-5 p-hierarchy, which are built on their own space with the fine rule.  Same chain, same passes
// (pa_rt_hex_core.hpp) and same pointwise D as rt_hex_apply_kernel of pa_rt_hex.hip; the fit to the machine is the one
// pa_nd_hex_q6.hip arrived at:
//
//   * One element per wave: 64 / 36 = 1.  Lanes 0 ... 35 own the 36 lines of a pass; lanes 36 ... 63 leave before the first
//     memory access.  A wave past the last element leaves as a whole: there is no workgroup barrier anywhere.
//   * The 1-D tables do not travel as kernel arguments (51 doubles at p = 5): every wave copies the operator's device tables
//     [Bo | Bc | Gc] into its own LDS strip behind the element's buffers and the passes read them from there, through a view
//     that hands the shared passes LDS pointers where the five-point kernels hand them argument arrays.
//   * The D stage walks the lane's qz column point by point with the next point's data requested one point ahead (the first
//     point before the forward contraction) instead of holding the column: 7 or 11 doubles in flight instead of 42 or 66.
//
// E^T is the E-vector + gather form, as for every H(div) block; there is no two right-hand-side form at six points.
#include "pa_rt_hex_core.hpp"

namespace pa {

constexpr int kRTQ6Waves = 4;  // waves = elements per workgroup: 4 x 11.2 KiB of LDS at p = 5

struct RTQ6Tab {  // what the shared passes read as the tables: the full row-major tables, whose first rows are the half tables
  const double *Bo, *Bc, *Gc;
};

// LDS of one wave: the contraction buffers of its element (RTLayout), then its copy of the 1-D tables [Bo | Bc | Gc]
template <int P1, int Q1>
struct RTQ6Strip {
  static constexpr int ELEM = RTLayout<P1, Q1>::ELEM_PAD;
  static constexpr int TAB = Q1 * (P1 + 2 * (P1 + 1));
  static constexpr int STRIDE = ELEM + ((TAB + 1) & ~1);
};

template <int Q1>
struct RTQ6Args {
  int ne;
  const int32_t *sidx_in;  // sorted-order signed index; kEssBit (on the dof number) = read as zero
  const uint16_t *perm;    // tensor-order slot of sorted entry m
  const double *geom;      // [ne][11][Q]
  const double *qdata;     // [ne][ncomp][Q], see RTArgs
  const double *x;
  double *ye;
  int xcd_chunk;           // > 0: workgroups are dealt to the 8 XCDs round-robin; give each XCD one contiguous element range
  CoeffDev c_mass, c_div;
  double w1[Q1];           // 1-D quadrature weights (q_w of l2_1_qf.h)
  const double *tab;       // the operator's device copy of the full 1-D tables, [Bo | Bc | Gc]
};

// D-stage data of one quadrature point: the packed entries, or the geometry rows the form reads (attribute, w detJ and, for the
// mass term, the nine of adj(J)^T / detJ)
template <bool USE_V, bool USE_DIV, bool QD>
struct RTQ6Point {
  static constexpr int NG = QD ? (USE_V ? 6 : 0) + (USE_DIV ? 1 : 0) : (USE_V ? 11 : 2);
  static constexpr int NSTORED = QD ? NG : 11;  // components per element as stored
  double g[NG];
  // src: the element's data at the lane's (qx, qy); QS: points per element
  template <int QS>
  __device__ __forceinline__ void load(const double *__restrict__ src, const int qoff) {
#pragma unroll
    for (int c = 0; c < NG; c++) g[c] = src[c * QS + qoff];
  }
};

// Launch bound: one wave per SIMD, as in pa_nd_hex_q6.hip -- the table operands live in VGPRs here.
template <int P1, int Q1, bool USE_V, bool USE_DIV, bool QD>
__global__ __launch_bounds__(64 * kRTQ6Waves, 1) void rt_hex_q6_kernel(const RTQ6Args<Q1> a) {
  using L = RTLayout<P1, Q1>;
  using S = RTQ6Strip<P1, Q1>;
  using Pt = RTQ6Point<USE_V, USE_DIV, QD>;
  static_assert(L::EPW == 1 && L::T <= 64 && L::NC <= Q1, "one element per wave, a line per lane");
  constexpr int Q = Q1 * Q1 * Q1, P = L::BASE;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int bid = a.xcd_chunk > 0 ? (int)(blockIdx.x & 7) * a.xcd_chunk + (int)(blockIdx.x >> 3) : (int)blockIdx.x;
  const int e = bid * kRTQ6Waves + wave;
  if (e >= a.ne) return;     // the whole wave: waves never wait for each other
  if (lane >= L::T) return;  // the lanes without a line: masked off for the rest of the wave's life
  constexpr bool lane_ok = true;  // (what the shared passes guard their stores with: every lane left owns a line)
  const int t = lane, ta = t % Q1, tb = t / Q1;
  double *sm = smem + (size_t)wave * S::STRIDE;
  for (int i = t; i < S::TAB; i += L::T) sm[S::ELEM + i] = a.tab[i];  // (visible to the wave at the first wave_sync())
  RTQ6Tab tab;
  tab.Bo = sm + S::ELEM, tab.Bc = tab.Bo + Q1 * P1, tab.Gc = tab.Bc + Q1 * (P1 + 1);

  // D-stage data of the first point of this lane's column: requested now, consumed after the forward contraction
  const double *dsrc = (QD ? a.qdata : a.geom) + (size_t)e * Pt::NSTORED * Q + t;
  Pt pt[2];
  pt[0].template load<Q>(dsrc, 0);
  double wab = 0.0;  // w(qx) w(qy) of the matrix-free divergence term, selected from the scalar arguments
  if (!QD && USE_DIV) {
    double wa = 0.0, wb = 0.0;
#pragma unroll
    for (int q = 0; q < Q1; q++) wa = ta == q ? a.w1[q] : wa, wb = tb == q ? a.w1[q] : wb;
    wab = wa * wb;
  }

  // E: sorted-order gather staged through LDS into tensor order (orientation signs applied here)
  constexpr int NPL = (P + L::T - 1) / L::T;
  int lp[NPL];
#pragma unroll
  for (int r = 0; r < NPL; r++) {
    const int m = t + L::T * r;
    lp[r] = 0;
    if (L::T * (r + 1) <= P || m < P) {  // (only the last round can be partial)
      const int s = a.sidx_in[(size_t)e * P + m];
      const int d = s >= 0 ? s : -1 - s;
      lp[r] = a.perm[(size_t)e * P + m];
      const double v = (d & kEssBit) ? 0.0 : a.x[d & ~kEssBit];
      sm[lp[r]] = s < 0 ? -v : v;
    }
  }
  wave_sync();

  double V[3][Q1], DV[Q1];
#pragma unroll
  for (int qz = 0; qz < Q1; qz++) DV[qz] = 0.0;
  rt_fwd_comp<P1, Q1, 0, USE_V, USE_DIV>(tab, sm, ta, tb, lane_ok, V[0], DV);
  rt_fwd_comp<P1, Q1, 1, USE_V, USE_DIV>(tab, sm, ta, tb, lane_ok, V[1], DV);
  rt_fwd_comp<P1, Q1, 2, USE_V, USE_DIV>(tab, sm, ta, tb, lane_ok, V[2], DV);
  wave_sync();

  // ---- D (hdiv_33 / l2_1 / l2mass_33), point by point along qz; the next point's data is on its way while this one is applied
#pragma unroll
  for (int qz = 0; qz < Q1; qz++) {
    if (qz + 1 < Q1) pt[(qz + 1) & 1].template load<Q>(dsrc, Q1 * Q1 * (qz + 1));
    const double *g = pt[qz & 1].g;
    if (QD) {
      if (USE_V) sym_mv(&g[0], V[0][qz], V[1][qz], V[2][qz], V[0][qz], V[1][qz], V[2][qz]);
      if (USE_DIV) DV[qz] *= g[Pt::NG - 1];
    } else {
      const int attr = (int)g[0];
      const double wdetJ = g[1];
      if (USE_V) {
        double Jl[9], Cm[9];
        adjJt33(&g[USE_V ? 2 : 0], Jl);
        coeff_unpack3(a.c_mass, attr, Cm);
        mult_AtBCx33(Jl, Cm, Jl, V[0][qz], V[1][qz], V[2][qz], wdetJ, V[0][qz], V[1][qz], V[2][qz]);
      }
      if (USE_DIV) {
        const double qw = wab * a.w1[qz];
        DV[qz] *= coeff_unpack1(a.c_div, attr) * qw * qw / wdetJ;
      }
    }
    __builtin_amdgcn_sched_barrier(0);  // one point at a time: the loads stay one point ahead, no further
  }

  rt_bwd_comp<P1, Q1, 0, USE_V, USE_DIV>(tab, sm, ta, tb, lane_ok, V[0], DV);
  rt_bwd_comp<P1, Q1, 1, USE_V, USE_DIV>(tab, sm, ta, tb, lane_ok, V[1], DV);
  rt_bwd_comp<P1, Q1, 2, USE_V, USE_DIV>(tab, sm, ta, tb, lane_ok, V[2], DV);
  wave_sync();
  // E^T, first half: out of LDS in sorted order (coalesced).  The E-vector holds the unsigned element results: the gather
  // applies the orientation sign of the entry (d_tent).
#pragma unroll
  for (int r = 0; r < NPL; r++) {
    const int m = t + L::T * r;
    if (L::T * (r + 1) <= P || m < P) a.ye[(size_t)e * P + m] = sm[lp[r]];
  }
}

template <int P1, int Q1>
static void rt_q6_launch_pq(const SubOp &so, const double *x, bool masked, hipStream_t s) {
  RTQ6Args<Q1> a{};
  a.ne = so.ne;
  a.sidx_in = (masked && so.d_sidx_bc) ? so.d_sidx_bc : so.d_sidx;
  a.perm = so.d_perm;
  a.geom = so.geom->d_geom;
  a.qdata = so.qd ? so.qd->d : nullptr;
  a.x = x;
  a.ye = so.d_ye;
  a.tab = so.d_tab;
  PA_REQUIRE((int)so.geom->w1.size() == Q1, "geometry data without its 1-D quadrature weights");
  for (int q = 0; q < Q1; q++) a.w1[q] = so.geom->w1[q];
  const int nblk = (so.ne + kRTQ6Waves - 1) / kRTQ6Waves;
  a.xcd_chunk = nblk >= 64 ? (nblk + 7) / 8 : 0;
  const dim3 grid(a.xcd_chunk > 0 ? 8 * a.xcd_chunk : nblk), block(64 * kRTQ6Waves);
  const size_t lds = sizeof(double) * (size_t)kRTQ6Waves * RTQ6Strip<P1, Q1>::STRIDE;
  const bool qd = a.qdata != nullptr;
#define PA_RT_Q6_LAUNCH(V, D)                                                               \
  if (qd)                                                                                   \
    hipLaunchKernelGGL((rt_hex_q6_kernel<P1, Q1, V, D, true>), grid, block, lds, s, a);     \
  else                                                                                      \
    hipLaunchKernelGGL((rt_hex_q6_kernel<P1, Q1, V, D, false>), grid, block, lds, s, a);
  switch (so.qf) {
    case PA_QF_HDIV_33:
      a.c_mass = so.c0.dev();
      PA_RT_Q6_LAUNCH(true, false)
      break;
    case PA_QF_L2_1:
      a.c_div = so.c0.dev();
      PA_RT_Q6_LAUNCH(false, true)
      break;
    case PA_QF_L2MASS_33:
      a.c_mass = so.c0.dev();
      a.c_div = so.c1.dev();
      PA_RT_Q6_LAUNCH(true, true)
      break;
    default:
      throw Error("QFunction not available for H(div) hexahedra");
  }
#undef PA_RT_Q6_LAUNCH
  PA_HIP(hipGetLastError());
}

// writes the E-vector so.d_ye; the caller follows with launch_et_gather (launch_rt_hex_apply has checked so.d_ye and the mask)
void launch_rt_hex_q6(const SubOp &so, const double *x, bool masked, hipStream_t s) {
  PA_REQUIRE(so.d_tab, "1-D tables missing on the device");
  switch (so.p * 16 + so.q1d) {
    PA_HEX_Q6_LIST(PA_HEX_PQ_CALL, rt_q6_launch_pq, so, x, masked, s)
    default: throw hex_pq_error("H(div)", so.p, so.q1d);
  }
}

}  // namespace pa
