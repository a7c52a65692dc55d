// Sum-factorised two-space forms on tensor-product hexahedra at six points per direction (gfx950, FP64): the pairs (p, 6),
// p = 1 ... 5 of PA_HEX_Q6_LIST -- the mixed mass (v, C u) between the Nedelec and the Raviart-Thomas space both ways round and
// the element error integrator in both input orders, at order 5 and on the coarser pairs of the same rule.  Same passes
// (pa_mixed_hex_core.hpp), same pointwise D and same fixed-order element sum as pa_mixed_hex.hip; the fit to the machine is
// that of pa_nd_hex_q6.hip / pa_rt_hex_q6.hip:
//
//   * One element per wave (64 / 36 = 1), 36 working lanes; lanes 36 ... 63 leave before the first memory access, a wave past
//     the last element leaves as a whole, wave-level syncs only.
//   * The value tables [Bo | Bc] are copied from the operator's device tables into the wave's LDS strip behind the element's
//     buffers and read from there through a view.
//   * D is matrix-free from the 11 geometry rows, walked point by point along the lane's qz column with the next point
//     requested one ahead: two points in flight at the most, which is also what keeps the error form, with both inputs'
//     values live, out of scratch.
//   * The error form adds the element's 36 partial sums in lane order through the element's LDS; lane 0 is the one writer of
//     the element's entry (the caller's element order), without atomics: the result is the same bits from run to run.
#include "pa_mixed_hex_core.hpp"

namespace pa {

namespace {

constexpr int kMHQ6Waves = 4;  // waves = elements per workgroup: 4 x 8.1 KiB of LDS at p = 5

struct MHQ6Tab {  // what the shared passes read as the tables: the full row-major tables, whose first rows are the half tables
  const double *Bo, *Bc;
};

// LDS of one wave: the contraction buffers of its element (MHLayout), then its copy of the value tables [Bo | Bc]
template <int P1, int Q1>
struct MHQ6Strip {
  static constexpr int ELEM = MHLayout<P1, Q1>::ELEM_PAD;
  static constexpr int TAB = Q1 * (P1 + (P1 + 1));
  static constexpr int STRIDE = ELEM + ((TAB + 1) & ~1);
};

struct MHQ6Args {
  int ne;
  // apply: 1 = trial space, 2 = test space; error: first and second input
  const int32_t *sidx1, *sidx2;   // sorted-order signed index
  const uint16_t *perm1, *perm2;  // tensor-order slot of sorted entry m
  const double *geom;             // [ne][11][Q]
  const double *x1, *x2;
  double *ye;                     // apply: E-vector of the test space [ne][P2]
  double *out;                    // error: [ne], the caller's element order
  const int32_t *eorder;          // caller's number of internal element e, or nullptr (same order)
  int xcd_chunk;                  // > 0: workgroups are dealt to the 8 XCDs round-robin; give each XCD one contiguous element range
  CoeffDev c1, c2;
  const double *tab;              // the operator's device copy of the full 1-D tables, [Bo | Bc | Gc]
};

// the 11 geometry rows of one quadrature point
struct MHQ6Point {
  double g[11];
  // src: the element's rows at the lane's (qx, qy); QS: points per element
  template <int QS>
  __device__ __forceinline__ void load(const double *__restrict__ src, const int qoff) {
#pragma unroll
    for (int c = 0; c < 11; c++) g[c] = src[c * QS + qoff];
  }
};

// what the two kernels start with: the wave's element, its strip with the table copy in place, and the lane's line
template <int P1, int Q1>
struct MHQ6Wave {
  int e, t;
  double *sm;
  MHQ6Tab tab;
  // false: this lane has nothing to do (a wave past the last element, or a lane without a line)
  __device__ __forceinline__ bool init(const MHQ6Args &a, double *smem) {
    using L = MHLayout<P1, Q1>;
    using S = MHQ6Strip<P1, Q1>;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bid = a.xcd_chunk > 0 ? (int)(blockIdx.x & 7) * a.xcd_chunk + (int)(blockIdx.x >> 3) : (int)blockIdx.x;
    e = bid * kMHQ6Waves + wave;
    if (e >= a.ne) return false;     // the whole wave: waves never wait for each other
    if (lane >= L::T) return false;  // the lanes without a line: masked off for the rest of the wave's life
    t = lane;
    sm = smem + (size_t)wave * S::STRIDE;
    for (int i = t; i < S::TAB; i += L::T) sm[S::ELEM + i] = a.tab[i];  // (visible to the wave at the first wave_sync())
    tab.Bo = sm + S::ELEM, tab.Bc = tab.Bo + Q1 * P1;
    return true;
  }
};

// ND_IN: the trial space is the Nedelec one (f_apply_hcurlhdiv_33), else the Raviart-Thomas one (f_apply_hdivhcurl_33)
template <int P1, int Q1, bool ND_IN>
__global__ __launch_bounds__(64 * kMHQ6Waves, 1) void mixed_hex_q6_apply_kernel(const MHQ6Args a) {
  using L = MHLayout<P1, Q1>;
  static_assert(L::EPW == 1 && L::T <= 64 && L::NC <= Q1, "one element per wave, a line per lane");
  constexpr int Q = Q1 * Q1 * Q1, PI = mh_ndofs<P1, ND_IN>(), PO = mh_ndofs<P1, !ND_IN>();
  extern __shared__ __attribute__((aligned(16))) double smem[];
  MHQ6Wave<P1, Q1> w;
  if (!w.init(a, smem)) return;
  constexpr bool lane_ok = true;  // (what the shared passes guard their stores with: every lane left owns a line)
  const int e = w.e, t = w.t, ta = t % Q1, tb = t / Q1;
  double *sm = w.sm;

  // geometry rows of the first point of this lane's column: requested now, consumed after the forward contraction
  const double *dsrc = a.geom + (size_t)e * 11 * Q + t;
  MHQ6Point pt[2];
  pt[0].template load<Q>(dsrc, 0);

  mh_gather<PI, L::T>(a.sidx1, a.perm1, a.x1, e, t, true, sm);
  wave_sync();
  double V[3][Q1];
  mh_forward<P1, Q1, ND_IN>(w.tab, sm, ta, tb, lane_ok, V);
  wave_sync();

  // ---- D (hcurlhdiv_33_qf.h): v = w detJ (J / detJ)^T C adj u  or  w detJ adj^T C (J / detJ) u
#pragma unroll
  for (int qz = 0; qz < Q1; qz++) {
    if (qz + 1 < Q1) pt[(qz + 1) & 1].template load<Q>(dsrc, Q1 * Q1 * (qz + 1));
    const double *g = pt[qz & 1].g;
    const int attr = (int)g[0];
    const double wdetJ = g[1], *adj = &g[2];
    double Jl[9], Cm[9];
    adjJt33(adj, Jl);
    coeff_unpack3(a.c1, attr, Cm);
    if (ND_IN)
      mult_AtBCx33(Jl, Cm, adj, V[0][qz], V[1][qz], V[2][qz], wdetJ, V[0][qz], V[1][qz], V[2][qz]);
    else
      mult_AtBCx33(adj, Cm, Jl, V[0][qz], V[1][qz], V[2][qz], wdetJ, V[0][qz], V[1][qz], V[2][qz]);
    __builtin_amdgcn_sched_barrier(0);  // one point at a time: the loads stay one point ahead, no further
  }

  mh_bwd_comp<P1, Q1, 0, !ND_IN>(w.tab, sm, ta, tb, lane_ok, V[0]);
  mh_bwd_comp<P1, Q1, 1, !ND_IN>(w.tab, sm, ta, tb, lane_ok, V[1]);
  mh_bwd_comp<P1, Q1, 2, !ND_IN>(w.tab, sm, ta, tb, lane_ok, V[2]);
  wave_sync();
  // E^T, first half: out of LDS in the sorted order of the test space (coalesced).  The E-vector holds the unsigned element
  // results: the gather applies the orientation sign of the entry.
  constexpr int NPL = (PO + L::T - 1) / L::T;
#pragma unroll
  for (int r = 0; r < NPL; r++) {
    const int m = t + L::T * r;
    if (L::T * (r + 1) <= PO || m < PO) a.ye[(size_t)e * PO + m] = sm[a.perm2[(size_t)e * PO + m]];
  }
}

// ND_FIRST: the first input is the Nedelec one (f_apply_hcurlhdiv_error_33), else the Raviart-Thomas one
template <int P1, int Q1, bool ND_FIRST>
__global__ __launch_bounds__(64 * kMHQ6Waves, 1) void mixed_hex_q6_error_kernel(const MHQ6Args a) {
  using L = MHLayout<P1, Q1>;
  static_assert(L::EPW == 1 && L::T <= 64 && L::NC <= Q1, "one element per wave, a line per lane");
  constexpr int Q = Q1 * Q1 * Q1, T = L::T, PA = mh_ndofs<P1, ND_FIRST>(), PB = mh_ndofs<P1, !ND_FIRST>();
  extern __shared__ __attribute__((aligned(16))) double smem[];
  MHQ6Wave<P1, Q1> w;
  if (!w.init(a, smem)) return;
  constexpr bool lane_ok = true;
  const int e = w.e, t = w.t, ta = t % Q1, tb = t / Q1;
  double *sm = w.sm;

  double V1[3][Q1], V2[3][Q1];
  mh_gather<PA, T>(a.sidx1, a.perm1, a.x1, e, t, true, sm);
  wave_sync();
  mh_forward<P1, Q1, ND_FIRST>(w.tab, sm, ta, tb, lane_ok, V1);
  wave_sync();
  // geometry rows of the first point of this lane's column: on their way during the second input's contraction
  const double *dsrc = a.geom + (size_t)e * 11 * Q + t;
  MHQ6Point pt[2];
  pt[0].template load<Q>(dsrc, 0);
  mh_gather<PB, T>(a.sidx2, a.perm2, a.x2, e, t, true, sm);
  wave_sync();
  mh_forward<P1, Q1, !ND_FIRST>(w.tab, sm, ta, tb, lane_ok, V2);

  // ---- hcurlhdiv_error_33_qf.h: w detJ |C_2 M_2 u_2 - C_1 M_1 u_1|^2, M the covariant / contravariant map of each input.
  // Both inputs' values are live here: two points in flight at the most (this one and the next one's rows).  The arithmetic
  // of a point is free to sink below every later request, and with all six points' rows in flight the order-3 to -5
  // instantiations spilled 28 ... 233 VGPRs: the address of point qz + 1 is therefore tied to the sum through point qz - 1,
  // as mixed_hex_error_kernel ties its own.
  double err = 0.0;  // the lane's column, bottom to top
#pragma unroll
  for (int qz = 0; qz < Q1; qz++) {
    if (qz + 1 < Q1) {
      int qoff = Q1 * Q1 * (qz + 1);
      if (qz >= 1) asm volatile("" : "+v"(qoff) : "v"(err));
      pt[(qz + 1) & 1].template load<Q>(dsrc, qoff);
    }
    const double *g = pt[qz & 1].g;
    const int attr = (int)g[0];
    const double wdetJ = g[1], *adj = &g[2];
    double Jl[9], C1[9], C2[9];
    adjJt33(adj, Jl);
    coeff_unpack3(a.c1, attr, C1);
    coeff_unpack3(a.c2, attr, C2);
    const double u1[3] = {V1[0][qz], V1[1][qz], V1[2][qz]}, u2[3] = {V2[0][qz], V2[1][qz], V2[2][qz]};
    double w1[3], w2[3];
    mult_BAx33(ND_FIRST ? adj : Jl, C1, u1, w1);
    mult_BAx33(ND_FIRST ? Jl : adj, C2, u2, w2);
    w2[0] -= w1[0], w2[1] -= w1[1], w2[2] -= w1[2];
    err += wdetJ * (w2[0] * w2[0] + w2[1] * w2[1] + w2[2] * w2[2]);
    __builtin_amdgcn_sched_barrier(0);
  }

  // sum over the 36 lanes of the element in lane order, through the element's LDS (the dofs are no longer needed; the all-ones
  // basis of integrator.cpp:560-574); one writer per element, the estimates are in the caller's element order
  wave_sync();
  sm[t] = err;
  wave_sync();
  if (t == 0) {
    double sum = 0.0;
    for (int i = 0; i < T; i++) sum += sm[i];
    a.out[a.eorder ? a.eorder[e] : e] += sum;
  }
}

template <int P1, int Q1>
void mh_q6_launch_pq(const SubOp &so, const SubOp &s2, const MixedSub &ms, const int kind, const double *x1, const double *x2,
                     double *out, hipStream_t s) {
  MHQ6Args a{};
  a.ne = ms.ne;
  a.sidx1 = so.d_sidx, a.perm1 = so.d_perm, a.sidx2 = s2.d_sidx, a.perm2 = s2.d_perm;
  a.geom = ms.geom->d_geom;
  a.x1 = x1, a.x2 = x2, a.ye = s2.d_ye, a.out = out, a.eorder = ms.d_eorder;
  a.c1 = ms.c0.dev(), a.c2 = ms.c1.dev();
  a.tab = so.d_tab;  // (make_mixed_hex_sub has checked that the two spaces carry the same value tables)
  const int nblk = (ms.ne + kMHQ6Waves - 1) / kMHQ6Waves;
  a.xcd_chunk = nblk >= 64 ? (nblk + 7) / 8 : 0;
  const dim3 grid(a.xcd_chunk > 0 ? 8 * a.xcd_chunk : nblk), block(64 * kMHQ6Waves);
  const size_t lds = sizeof(double) * (size_t)kMHQ6Waves * MHQ6Strip<P1, Q1>::STRIDE;
  switch (kind) {
    case 0: hipLaunchKernelGGL((mixed_hex_q6_apply_kernel<P1, Q1, true>), grid, block, lds, s, a); break;
    case 1: hipLaunchKernelGGL((mixed_hex_q6_apply_kernel<P1, Q1, false>), grid, block, lds, s, a); break;
    case 2: hipLaunchKernelGGL((mixed_hex_q6_error_kernel<P1, Q1, true>), grid, block, lds, s, a); break;
    case 3: hipLaunchKernelGGL((mixed_hex_q6_error_kernel<P1, Q1, false>), grid, block, lds, s, a); break;
    default: throw Error("not a mixed-space QFunction");
  }
  PA_HIP(hipGetLastError());
}

}  // namespace

// so: the input (first) space's block, s2: the other one; kind as launch_mixed_hex has resolved it (transpose included)
void launch_mixed_hex_q6(const SubOp &so, const SubOp &s2, const MixedSub &ms, int kind, const double *x1, const double *x2,
                         double *out, hipStream_t s) {
  PA_REQUIRE(so.d_tab, "1-D tables missing on the device");
  switch (so.p * 16 + so.q1d) {
    PA_HEX_Q6_LIST(PA_HEX_PQ_CALL, mh_q6_launch_pq, so, s2, ms, kind, x1, x2, out, s)
    default: throw hex_pq_error("H(curl) - H(div)", so.p, so.q1d);
  }
}

}  // namespace pa
