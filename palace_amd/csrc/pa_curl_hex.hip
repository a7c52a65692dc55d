// Discrete curl ND(p) -> RT(p) on tensor hexahedra and its transpose: the flux B = curl A.
//
// Replaces the libCEED interpolator operator Palace builds for the pair (Nedelec, Raviart-Thomas) with mfem::CurlInterpolator
// (reference fem/fespace.cpp:199-206, fem/libceed/basis.cpp:139-150, fem/bilinearform.cpp:203-282).  With the nodal tensor
// bases of fem/fespace.py (ND) and fem/rthex.py (RT) the element matrix has no dense block: RT component c is
//     RT_c = D_d ND_e - D_e ND_d        (c, d, e) a cyclic triple,
// where D_d is the 1-D matrix Dg [p][p+1] (derivative of the closed Gauss-Lobatto basis at the open Gauss-Legendre nodes) along
// direction d and the identity along the other two, because the node sets of the two elements coincide there.  Every row has
// 2 (p + 1) non-zeros; the dense form of the same operator multiplies a 3 p^2 (p+1) x 3 p (p+1)^2 matrix per element.
//
// Mapping as in interp_kernel_s (pa_interp.hip): (p+1)^2 lanes per element, 64 / (p+1)^2 elements per wave, four waves per
// block, hand-offs through LDS inside the wave, no workgroup barrier.  The signed input element vector is staged in LDS in
// tensor order (every value and every index word is read from memory once per element); the two terms of a component are
// formed by two lane assignments -- each term is a set of whole lines along ITS differentiated direction, so Dg stays a scalar
// operand -- and meet in a one-component LDS buffer.  Forward stores the owner copy of every RT dof (kCurlOwnBit in the RT
// index array, set by InterpOperator): no atomics, no memset.  The transpose reads RT through the same mask and writes the
// unsigned ND element vector to the domain E-vector, which InterpOperator's gather sums in its fixed order.
#include "linalg.hpp"
#include "pa_device.hpp"

namespace palace {

namespace {

constexpr int kMaxN = 6;            // closed nodes per direction (p <= 5)
constexpr int kCurlOwnBit = 1 << 29;  // InterpOperator's owner flag (pa_interp.hip: kOwnBit)

struct CurlArgs {
  int ne, p;
  const int32_t *lidx_nd, *lidx_rt;  // signed tensor-order index arrays [ne][P_ND], [ne][P_RT] (RT: owner flag)
  const double *x;
  double *y;      // forward: RT L-vector; transpose: ND E-vector [ne][P_ND]
  double Dg[36];  // [p][p+1] by value: scalar operands of the specialised forms
  const double *Dg_dev;  // the same on the device: the generic form keeps it in LDS (30 doubles as scalars spill SGPRs there)
};

using pa::wave_sync;

template <int P>
__device__ __forceinline__ double dg_at(const CurlArgs &a, const double *sDg, const int k) {
  if constexpr (P > 0) return a.Dg[k];
  else return sDg[k];
}

// tensor-order position inside a component block: ND block `open` has p nodes along `open` and p + 1 along the others, RT
// block `closed` p + 1 along `closed` and p along the others
template <int OPEN>
__device__ __forceinline__ int nd_pos(const int p, const int i0, const int i1, const int i2) {
  const int n0 = OPEN == 0 ? p : p + 1, n1 = OPEN == 1 ? p : p + 1;
  return i0 + n0 * (i1 + n1 * i2);
}
template <int CLOSED>
__device__ __forceinline__ int rt_pos(const int p, const int i0, const int i1, const int i2) {
  const int n0 = CLOSED == 0 ? p + 1 : p, n1 = CLOSED == 1 ? p + 1 : p;
  return i0 + n0 * (i1 + n1 * i2);
}
// (value along axis A, B, C) -> (i0, i1, i2)
template <int A, int B, int C>
__device__ __forceinline__ void axes(const int va, const int vb, const int vc, int (&i)[3]) {
  i[A] = va, i[B] = vb, i[C] = vc;
}

// Forward, RT component C with (C, D, E) cyclic; lane (ta, tb), ta < p + 1 the closed index along C.
//   term 1: tb = i_E, line of ND_E along D  ->  + D_D ND_E into sT for i_D = 0 .. p
//   term 2: tb = i_D, line of ND_D along E  ->  sT - D_E ND_D, owner copy stored, for i_E = 0 .. p
template <int P, int C>
__device__ __forceinline__ void curl_fwd_comp(const CurlArgs &a, const int p, const bool active, const bool lane_ok, const int ta,
                                              const int tb, const double *sX, double *sT, const double *sDg, const int (&sf)[kMaxN - 1]) {
  constexpr int D = (C + 1) % 3, E = (C + 2) % 3, NM = P > 0 ? P + 1 : kMaxN;
  const int n1 = p + 1, bnd = p * n1 * n1;
  const bool act = tb < p;
  int i[3];
  {
    double u[NM];
#pragma unroll
    for (int k = 0; k < NM; k++) {
      axes<C, D, E>(ta, k < n1 ? k : 0, act ? tb : 0, i);
      u[k] = k < n1 ? sX[E * bnd + nd_pos<E>(p, i[0], i[1], i[2])] : 0.0;
    }
#pragma unroll
    for (int o = 0; o < NM - 1; o++) {
      if (o < p) {
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < NM; k++)
          if (k < n1) v += dg_at<P>(a, sDg, o * n1 + k) * u[k];
        axes<C, D, E>(ta, o, tb, i);
        if (lane_ok && act) sT[rt_pos<C>(p, i[0], i[1], i[2])] = v;
      }
    }
  }
  wave_sync();
  {
    double u[NM];
#pragma unroll
    for (int k = 0; k < NM; k++) {
      axes<C, D, E>(ta, act ? tb : 0, k < n1 ? k : 0, i);
      u[k] = k < n1 ? sX[D * bnd + nd_pos<D>(p, i[0], i[1], i[2])] : 0.0;
    }
#pragma unroll
    for (int o = 0; o < NM - 1; o++) {
      if (o < p) {
        axes<C, D, E>(ta, act ? tb : 0, o, i);
        double v = sT[rt_pos<C>(p, i[0], i[1], i[2])];
#pragma unroll
        for (int k = 0; k < NM; k++)
          if (k < n1) v -= dg_at<P>(a, sDg, o * n1 + k) * u[k];
        if (active && act) {
          const int s = sf[o];
          const int g = s >= 0 ? s : -1 - s;
          if (g & kCurlOwnBit) a.y[g & ~kCurlOwnBit] = s >= 0 ? v : -v;
        }
      }
    }
  }
  wave_sync();  // (sT is the next component's)
}

// the lane's RT index words of component C: (ta, tb) = (i_C, i_D), one per i_E
template <int P, int C>
__device__ __forceinline__ void curl_fwd_idx(const CurlArgs &a, const int p, const size_t e, const bool active, const int ta,
                                             const int tb, int (&sf)[kMaxN - 1]) {
  constexpr int D = (C + 1) % 3, E = (C + 2) % 3, NM = P > 0 ? P + 1 : kMaxN;
  const int Prt = 3 * p * p * (p + 1);
  int i[3];
#pragma unroll
  for (int o = 0; o < NM - 1; o++) {
    axes<C, D, E>(ta, tb, o < p ? o : 0, i);  // (one lane mask for all words: a word beyond the order repeats the first)
    sf[o] = (active && tb < p) ? a.lidx_rt[e * Prt + C * p * p * (p + 1) + rt_pos<C>(p, i[0], i[1], i[2])] : 0;
  }
}

// Transpose, ND component N with (C, D, N) cyclic: ND_N appears in RT_C = + D_D ND_N ... and in RT_D = ... - D_C ND_N.
//   term 1: (ta, tb) = (i_C closed, i_N), line of RT_C along D  ->  + D_D^T RT_C into sT for a_D = 0 .. p + 1
//   term 2: (ta, tb) = (j_D closed, i_N), line of RT_D along C  ->  sT - D_C^T RT_D to the E-vector, for a_C = 0 .. p + 1
template <int P, int N>
__device__ __forceinline__ void curl_tr_comp(const CurlArgs &a, const int p, const size_t e, const bool active, const bool lane_ok,
                                             const int ta, const int tb, const double *sX, double *sT, const double *sDg) {
  constexpr int C = (N + 1) % 3, D = (N + 2) % 3, NM = P > 0 ? P + 1 : kMaxN;
  const int n1 = p + 1, brt = p * p * n1, bnd = p * n1 * n1;
  const bool act = tb < p;
  int i[3];
  {
    double z[NM - 1];
#pragma unroll
    for (int k = 0; k < NM - 1; k++) {
      axes<C, D, N>(ta, k < p ? k : 0, act ? tb : 0, i);
      z[k] = k < p ? sX[C * brt + rt_pos<C>(p, i[0], i[1], i[2])] : 0.0;
    }
#pragma unroll
    for (int o = 0; o < NM; o++) {
      if (o < n1) {
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < NM - 1; k++)
          if (k < p) v += dg_at<P>(a, sDg, k * n1 + o) * z[k];
        axes<C, D, N>(ta, o, tb, i);
        if (lane_ok && act) sT[nd_pos<N>(p, i[0], i[1], i[2])] = v;
      }
    }
  }
  wave_sync();
  {
    double z[NM - 1];
#pragma unroll
    for (int k = 0; k < NM - 1; k++) {
      axes<C, D, N>(k < p ? k : 0, ta, act ? tb : 0, i);
      z[k] = k < p ? sX[D * brt + rt_pos<D>(p, i[0], i[1], i[2])] : 0.0;
    }
#pragma unroll
    for (int o = 0; o < NM; o++) {
      if (o < n1) {
        axes<C, D, N>(o, ta, act ? tb : 0, i);
        const int pos = nd_pos<N>(p, i[0], i[1], i[2]);
        double v = sT[pos];
#pragma unroll
        for (int k = 0; k < NM - 1; k++)
          if (k < p) v -= dg_at<P>(a, sDg, k * n1 + o) * z[k];
        if (active && act) a.y[e * (size_t)(3 * bnd) + N * bnd + pos] = v;
      }
    }
  }
  wave_sync();
}

// P > 0: the order at compile time (loops unrolled, lines in registers); P == 0: any order up to kMaxN - 1 from the arguments
template <bool TRANSPOSE, int P>
__global__ __launch_bounds__(256) void curl_hex_kernel(const CurlArgs a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  constexpr int NM = P > 0 ? P + 1 : kMaxN;
  const int p = P > 0 ? P : a.p, n1 = p + 1, T = n1 * n1, EPW = 64 / T;
  const int Pnd = 3 * p * T, Prt = 3 * p * p * n1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane / T, t = lane - sub * T;
  const int ta = t % n1, tb = t / n1;
  const bool lane_ok = sub < EPW;
  const int el = (blockIdx.x * 4 + wave) * EPW + sub;
  const bool active = lane_ok && el < a.ne;
  const size_t e = (size_t)el;
  // per element: the staged input element vector (P_ND or P_RT doubles), then one component block of the other space
  double *sX = smem + (size_t)(wave * EPW + (lane_ok ? sub : 0)) * (Pnd + p * p * n1);
  double *sT = sX + (TRANSPOSE ? Prt : Pnd);
  // generic form: the wave's copy of Dg behind the element areas (written before the first hand-off below)
  double *sDg = smem + (size_t)(4 * EPW) * (Pnd + p * p * n1) + wave * 36;
  if (P == 0 && lane < p * n1) sDg[lane] = a.Dg_dev[lane];
  if (!TRANSPOSE) {
    // (A) every index word of the element, (B) the ND values, (C) the components out of LDS, stores as they complete
    int sc[3 * (NM - 1)], sf0[kMaxN - 1], sf1[kMaxN - 1], sf2[kMaxN - 1];
#pragma unroll
    for (int m = 0; m < 3 * (NM - 1); m++) sc[m] = active ? a.lidx_nd[e * Pnd + t + T * (m < 3 * p ? m : 0)] : 0;
    curl_fwd_idx<P, 0>(a, p, e, active, ta, tb, sf0);
    curl_fwd_idx<P, 1>(a, p, e, active, ta, tb, sf1);
    curl_fwd_idx<P, 2>(a, p, e, active, ta, tb, sf2);
#pragma unroll
    for (int m = 0; m < 3 * (NM - 1); m++) {
      const int s = sc[m];
      const double xv = active ? a.x[s >= 0 ? s : -1 - s] : 0.0;
      if (lane_ok && m < 3 * p) sX[t + T * m] = s >= 0 ? xv : -xv;
    }
    wave_sync();
    curl_fwd_comp<P, 0>(a, p, active, lane_ok, ta, tb, sX, sT, sDg, sf0);
    curl_fwd_comp<P, 1>(a, p, active, lane_ok, ta, tb, sX, sT, sDg, sf1);
    curl_fwd_comp<P, 2>(a, p, active, lane_ok, ta, tb, sX, sT, sDg, sf2);
  } else {
    // the owner-masked signed RT element vector: entry t + T m (3 p^2 / (p + 1) words per lane, the last one partial)
    int sr[3 * (NM - 1)];
#pragma unroll
    for (int m = 0; m < 3 * (NM - 1); m++) sr[m] = (active && t + T * m < Prt) ? a.lidx_rt[e * Prt + t + T * m] : 0;
#pragma unroll
    for (int m = 0; m < 3 * (NM - 1); m++) {
      const int s = sr[m];
      const int g = s >= 0 ? s : -1 - s;
      const bool in = t + T * m < Prt;
      const double xv = (active && in && (g & kCurlOwnBit)) ? a.x[g & ~kCurlOwnBit] : 0.0;
      if (lane_ok && in) sX[t + T * m] = s >= 0 ? xv : -xv;
    }
    wave_sync();
    curl_tr_comp<P, 0>(a, p, e, active, lane_ok, ta, tb, sX, sT, sDg);
    curl_tr_comp<P, 1>(a, p, e, active, lane_ok, ta, tb, sX, sT, sDg);
    curl_tr_comp<P, 2>(a, p, e, active, lane_ok, ta, tb, sX, sT, sDg);
  }
}

}  // namespace

// lidx_rt carries the owner flag on one copy of every RT dof; Dg [p][p+1] on the host and on the device; out: the RT L-vector (forward) or the
// ND E-vector [ne][3 p (p+1)^2] (transpose)
void launch_curl_hex(const bool transpose, const int p, const int ne, const int32_t *lidx_nd, const int32_t *lidx_rt, const double *Dg,
                     const double *Dg_dev, const double *x, double *out, hipStream_t stream) {
  PA_REQUIRE(p >= 1 && p + 1 <= kMaxN, "discrete curl: order above 5");
  CurlArgs a{ne, p, lidx_nd, lidx_rt, x, out, {}, Dg_dev};
  for (int k = 0; k < p * (p + 1); k++) a.Dg[k] = Dg[k];
  const int n1 = p + 1, epb = 4 * (64 / (n1 * n1));
  const size_t lds = sizeof(double) * ((size_t)epb * (3 * p * n1 * n1 + p * p * n1) + (p > 4 ? 4 * 36 : 0));
  const dim3 grid((ne + epb - 1) / epb), block(256);
#define PA_CURL_CASE(P)                                                                    \
  case P:                                                                                  \
    if (transpose) hipLaunchKernelGGL((curl_hex_kernel<true, P>), grid, block, lds, stream, a);   \
    else hipLaunchKernelGGL((curl_hex_kernel<false, P>), grid, block, lds, stream, a);     \
    break;
  switch (p) {
    PA_CURL_CASE(1) PA_CURL_CASE(2) PA_CURL_CASE(3) PA_CURL_CASE(4)
    default:
      if (transpose) hipLaunchKernelGGL((curl_hex_kernel<true, 0>), grid, block, lds, stream, a);
      else hipLaunchKernelGGL((curl_hex_kernel<false, 0>), grid, block, lds, stream, a);
  }
#undef PA_CURL_CASE
  PA_HIP(hipGetLastError());
}

}  // namespace palace
