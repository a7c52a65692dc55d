// Both parts of a complex field per launch for the two-space forms of pa_mixed_hex.hip (gfx950, FP64): the mixed mass
// y_r = W x_r, y_i = W x_i and the element error eta_e^2(F_r, G_r) + eta_e^2(F_i, G_i) of the flux error estimators'
// ComplexVector instantiation (linalg/errorestimator.cpp:183-268).  Same mapping, LDS layout and device helpers
// (pa_mixed_hex_core.hpp) as the one-part kernels, and per part the same operations in the same order, so each part equals the
// one-part result to the bit.  A translation unit of its own: the one-part kernels compile to the code they had without it.
#include "pa_mixed_hex_core.hpp"

namespace pa {

namespace {

// ---- both parts of a complex field in one launch --------------------------------------------------------------------------
// y_r = W x_r and y_i = W x_i (apply), eta_e^2 += eta_e^2(F_r, G_r) + eta_e^2(F_i, G_i) (error): the geometry rows, the index
// words and the point matrices are the same for the two parts.  Three forms, chosen per (order, points) pair by the registers
// and, for the apply, by what keeps each part equal to the one-part result to the bit:
//  * fused: the values of both parts are live through one D loop, which reads the geometry rows and builds the matrices once
//    per point;
//  * paired (apply): bit 3 of blockIdx.x is the part (both parts of an element group on one XCD) and each block runs the one-part kernel's body, the two blocks of an element group
//    dispatched next to each other; the E-vectors of both parts then go through one gather;
//  * sequential (error): part r runs completely, then part i over the same element (the one-part kernel's live set; the
//    second read of the element's rows follows the first within the wave).
// A sequential apply was tried and is not here: inside its loop the compiler contracts the products that two mirrored table
// rows share (the middle column of an odd node count) into mul + add where the one-part kernel has two fmas, at orders >= 2
// (DESIGN.md 3.3d), and the results differ in the last bit.
template <int P1, int Q1>
struct MHArgs2 : MHArgs<P1, Q1> {
  const double *x1i, *x2i;  // the imaginary parts of x1, x2
  double *ye2;              // apply: second E-vector of the test space
};

template <int P1, int Q1, bool ND_IN>
__global__ __launch_bounds__(64 * kMHWaves, 2) void mixed_hex_apply2_kernel(const MHArgs2<P1, Q1> a) {
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
  constexpr int NPL = (PO + L::T - 1) / L::T;
  const size_t gq = eg * 11 * Q + ta + Q1 * tb;

  double V[2][3][Q1];
  mh_gather<PI, L::T>(a.sidx1, a.perm1, a.x1, e, t, active, sm);
  wave_sync();
  mh_forward<P1, Q1, ND_IN>(a.tab, sm, ta, tb, lane_ok, V[0]);
  wave_sync();
  mh_gather<PI, L::T>(a.sidx1, a.perm1, a.x1i, e, t, active, sm);
  wave_sync();
  mh_forward<P1, Q1, ND_IN>(a.tab, sm, ta, tb, lane_ok, V[1]);
  wave_sync();
#pragma unroll
  for (int qz = 0; qz < Q1; qz++) {
    // both parts' values are live here: the address of point qz is tied to the result of point qz - 2, two points in flight at
    // a time (as in mixed_hex_error_kernel)
    size_t go = gq + Q1 * Q1 * qz;
    if (qz >= 2) asm volatile("" : "+v"(go) : "v"(V[1][2][qz - 2]));
    int attr;
    double wdetJ, adj[9], Jl[9], Cm[9];
    mh_point(a.geom + go, Q, attr, wdetJ, adj, Jl);
    coeff_unpack3(a.c1, attr, Cm);
#pragma unroll
    for (int part = 0; part < 2; part++) {
      double(&W)[3][Q1] = V[part];
      if (ND_IN)
        mult_AtBCx33(Jl, Cm, adj, W[0][qz], W[1][qz], W[2][qz], wdetJ, W[0][qz], W[1][qz], W[2][qz]);
      else
        mult_AtBCx33(adj, Cm, Jl, W[0][qz], W[1][qz], W[2][qz], wdetJ, W[0][qz], W[1][qz], W[2][qz]);
    }
  }
#pragma unroll
  for (int part = 0; part < 2; part++) {
    mh_bwd_comp<P1, Q1, 0, !ND_IN>(a.tab, sm, ta, tb, lane_ok, V[part][0]);
    mh_bwd_comp<P1, Q1, 1, !ND_IN>(a.tab, sm, ta, tb, lane_ok, V[part][1]);
    mh_bwd_comp<P1, Q1, 2, !ND_IN>(a.tab, sm, ta, tb, lane_ok, V[part][2]);
    wave_sync();
    double *ye = part ? a.ye2 : a.ye;
#pragma unroll
    for (int r = 0; r < NPL; r++) {
      const int m = t + L::T * r;
      if (active && m < PO) ye[(size_t)e * PO + m] = sm[a.perm2[(size_t)e * PO + m]];
    }
    wave_sync();
  }
}

// The same in the paired form: bit 3 of blockIdx.x is the part, and each block runs the one-part kernel's body on its part.
// Workgroups go round-robin over the eight XCDs, so blocks b and b + 8 -- the two parts of one element group -- run on the same
// XCD eight dispatches apart.  Whether the second one's geometry rows and index words are then served from that XCD's L2 has
// not been measured.  The grid is padded to whole groups of sixteen blocks; the blocks past the last element store nothing.
template <int P1, int Q1, bool ND_IN>
__global__ __launch_bounds__(64 * kMHWaves, 2) void mixed_hex_apply_pair_kernel(const MHArgs2<P1, Q1> a) {
  using L = MHLayout<P1, Q1>;
  constexpr int Q = Q1 * Q1 * Q1, PI = mh_ndofs<P1, ND_IN>(), PO = mh_ndofs<P1, !ND_IN>();
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane / L::T, t = lane - sub * L::T;
  const int ta = t % Q1, tb = t / Q1;
  const bool lane_ok = sub < L::EPW;
  const int part = (blockIdx.x >> 3) & 1;
  const int e = ((((blockIdx.x >> 4) << 3) | (blockIdx.x & 7)) * kMHWaves + wave) * L::EPW + sub;
  const bool active = lane_ok && e < a.ne;
  double *sm = smem + (size_t)(wave * L::EPW + (lane_ok ? sub : 0)) * L::ELEM_PAD;
  const size_t eg = active ? e : 0;  // idle lanes read element 0 and store nothing
  const double *x = part ? a.x1i : a.x1;
  double *ye = part ? a.ye2 : a.ye;

  mh_gather<PI, L::T>(a.sidx1, a.perm1, x, e, t, active, sm);
  wave_sync();
  double V[3][Q1];
  mh_forward<P1, Q1, ND_IN>(a.tab, sm, ta, tb, lane_ok, V);
  wave_sync();
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
  constexpr int NPL = (PO + L::T - 1) / L::T;
#pragma unroll
  for (int r = 0; r < NPL; r++) {
    const int m = t + L::T * r;
    if (active && m < PO) ye[(size_t)e * PO + m] = sm[a.perm2[(size_t)e * PO + m]];
  }
}

// sum of a lane's value over the T lanes of its element in the fixed order of mixed_hex_error_kernel (valid on lane t == 0 at
// least); the 25-lane form goes through the element's LDS
template <int P1, int Q1>
__device__ __forceinline__ double mh_element_sum(const double err, double *sm, const int lane, const int t, const bool lane_ok) {
  constexpr int T = Q1 * Q1;
  double sum;
  if (T == 4 || T == 16) {
    sum = err;
#pragma unroll
    for (int m = T / 2; m >= 1; m >>= 1) sum += __shfl_xor(sum, m, 64);
  } else if (T == 9) {
    sum = 0.0;
    const int first = lane - t;
#pragma unroll
    for (int i = 0; i < T; i++) sum += __shfl(err, min(first + i, 63), 64);
  } else {
    wave_sync();
    if (lane_ok) sm[t] = err;
    wave_sync();
    sum = 0.0;
    if (t == 0)
      for (int i = 0; i < T; i++) sum += sm[i];
  }
  return sum;
}

// the error form of one point (hcurlhdiv_error_33_qf.h), as in mixed_hex_error_kernel
template <bool ND_FIRST>
__device__ __forceinline__ double mh_error_point(const double wdetJ, const double adj[9], const double Jl[9], const double C1[9],
                                                 const double C2[9], const double (&u1)[3], const double (&u2)[3]) {
  double w1[3], w2[3];
  mult_BAx33(ND_FIRST ? adj : Jl, C1, u1, w1);
  mult_BAx33(ND_FIRST ? Jl : adj, C2, u2, w2);
  w2[0] -= w1[0], w2[1] -= w1[1], w2[2] -= w1[2];
  return wdetJ * (w2[0] * w2[0] + w2[1] * w2[1] + w2[2] * w2[2]);
}

// Which form of the error kernel a pair runs (profiles/r11_two_part_resources.txt): at (2, 3) the fused form is 4 to 8 VGPRs over
// the budget of two waves per SIMD, with two points in flight as with one
constexpr bool mh_error2_fused(int p1, int q1) { return p1 == 1 && q1 <= 3; }

template <int P1, int Q1, bool ND_FIRST, bool FUSED>
__global__ __launch_bounds__(64 * kMHWaves, 2) void mixed_hex_error2_kernel(const MHArgs2<P1, Q1> a) {
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
  const size_t gq = eg * 11 * Q + ta + Q1 * tb;

  double sum[2];
  if (FUSED) {
    double V1[2][3][Q1], V2[2][3][Q1];
#pragma unroll
    for (int part = 0; part < 2; part++) {
      mh_gather<PA, T>(a.sidx1, a.perm1, part ? a.x1i : a.x1, e, t, active, sm);
      wave_sync();
      mh_forward<P1, Q1, ND_FIRST>(a.tab, sm, ta, tb, lane_ok, V1[part]);
      wave_sync();
      mh_gather<PB, T>(a.sidx2, a.perm2, part ? a.x2i : a.x2, e, t, active, sm);
      wave_sync();
      mh_forward<P1, Q1, !ND_FIRST>(a.tab, sm, ta, tb, lane_ok, V2[part]);
      wave_sync();
    }
    double ep[2][Q1];
#pragma unroll
    for (int qz = 0; qz < Q1; qz++) {
      size_t go = gq + Q1 * Q1 * qz;
      if (qz >= 2) asm volatile("" : "+v"(go) : "v"(ep[1][qz - 2]));  // two points in flight, as in the one-part kernel
      int attr;
      double wdetJ, adj[9], Jl[9], C1[9], C2[9];
      mh_point(a.geom + go, Q, attr, wdetJ, adj, Jl);
      coeff_unpack3(a.c1, attr, C1);
      coeff_unpack3(a.c2, attr, C2);
#pragma unroll
      for (int part = 0; part < 2; part++) {
        const double u1[3] = {V1[part][0][qz], V1[part][1][qz], V1[part][2][qz]};
        const double u2[3] = {V2[part][0][qz], V2[part][1][qz], V2[part][2][qz]};
        ep[part][qz] = mh_error_point<ND_FIRST>(wdetJ, adj, Jl, C1, C2, u1, u2);
      }
    }
#pragma unroll
    for (int part = 0; part < 2; part++) {
      double err = 0.0;  // the lane's column, bottom to top
#pragma unroll
      for (int qz = 0; qz < Q1; qz++) err += ep[part][qz];
      sum[part] = mh_element_sum<P1, Q1>(err, sm, lane, t, lane_ok);
    }
  } else {
#pragma unroll 1
    for (int part = 0; part < 2; part++) {
      double V1[3][Q1], V2[3][Q1];
      mh_gather<PA, T>(a.sidx1, a.perm1, part ? a.x1i : a.x1, e, t, active, sm);
      wave_sync();
      mh_forward<P1, Q1, ND_FIRST>(a.tab, sm, ta, tb, lane_ok, V1);
      wave_sync();
      mh_gather<PB, T>(a.sidx2, a.perm2, part ? a.x2i : a.x2, e, t, active, sm);
      wave_sync();
      mh_forward<P1, Q1, !ND_FIRST>(a.tab, sm, ta, tb, lane_ok, V2);
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
        ep[qz] = mh_error_point<ND_FIRST>(wdetJ, adj, Jl, C1, C2, u1, u2);
      }
      double err = 0.0;
#pragma unroll
      for (int qz = 0; qz < Q1; qz++) err += ep[qz];
      const double s = mh_element_sum<P1, Q1>(err, sm, lane, t, lane_ok);
      if (part == 0)
        sum[0] = s;
      else
        sum[1] = s;
      wave_sync();  // the next part's gather overwrites the LDS the sum may have gone through
    }
  }
  // one writer per element; the two parts are added one after the other, as two ApplyAdd calls add them
  if (active && t == 0) {
    double *o = a.out + (a.eorder ? a.eorder[e] : e);
    *o = (*o + sum[0]) + sum[1];
  }
}

// Which form of the two-part kernels a pair runs (profiles/r11_two_part_resources.txt): the fused D loop where both parts'
// values fit at two waves per SIMD without scratch (and, for the apply, at order 1, where it gives the one-part kernel's bits),
// else the paired form (apply) or the sequential form (error).
constexpr bool mh_apply2_fused(int p1, int q1, bool nd_in) { return p1 == 1 && q1 <= (nd_in ? 4 : 3); }

struct MH2Call {
  const SubOp &so, &s2;
  const MixedSub &ms;
  int kind;
  const double *x1, *x2, *x1i, *x2i;
  double *out;
  hipStream_t s;
};

template <int P1, int Q1>
MHArgs2<P1, Q1> mh_args2(const MH2Call &c) {
  constexpr int QH = MHTab<P1, Q1>::QH, NC = P1 + 1;
  MHArgs2<P1, Q1> a{};
  a.ne = c.ms.ne;
  a.sidx1 = c.so.d_sidx, a.perm1 = c.so.d_perm, a.sidx2 = c.s2.d_sidx, a.perm2 = c.s2.d_perm;
  a.geom = c.ms.geom->d_geom;
  a.x1 = c.x1, a.x2 = c.x2, a.x1i = c.x1i, a.x2i = c.x2i;
  a.ye = c.s2.d_ye, a.ye2 = c.s2.d_ye2, a.out = c.out, a.eorder = c.ms.d_eorder;
  a.c1 = c.ms.c0.dev(), a.c2 = c.ms.c1.dev();
  for (int i = 0; i < QH * P1; i++) a.tab.Bo[i] = c.so.Bo[i];
  for (int i = 0; i < QH * NC; i++) a.tab.Bc[i] = c.so.Bc[i];
  return a;
}

// each launcher instantiates the kernels of its own list only
template <int P1, int Q1, bool ND_IN>
void mh_launch_apply2(const MH2Call &c) {
  using L = MHLayout<P1, Q1>;
  const MHArgs2<P1, Q1> a = mh_args2<P1, Q1>(c);
  const int epb = kMHWaves * L::EPW, nb = (c.ms.ne + epb - 1) / epb;
  const dim3 block(64 * kMHWaves);
  const size_t lds = sizeof(double) * (size_t)epb * L::ELEM_PAD;
  if constexpr (mh_apply2_fused(P1, Q1, ND_IN))
    hipLaunchKernelGGL((mixed_hex_apply2_kernel<P1, Q1, ND_IN>), dim3(nb), block, lds, c.s, a);
  else
    hipLaunchKernelGGL((mixed_hex_apply_pair_kernel<P1, Q1, ND_IN>), dim3(16 * ((nb + 7) / 8)), block, lds, c.s, a);
  PA_HIP(hipGetLastError());
}
template <int P1, int Q1>
void mh_launch_apply2_pq(const MH2Call &c) {
  PA_REQUIRE(c.kind == 0 || c.kind == 1, "not a two-space mass");
  c.kind == 0 ? mh_launch_apply2<P1, Q1, true>(c) : mh_launch_apply2<P1, Q1, false>(c);
}
template <int P1, int Q1>
void mh_launch_error2_pq(const MH2Call &c) {
  using L = MHLayout<P1, Q1>;
  constexpr bool FE = mh_error2_fused(P1, Q1);
  PA_REQUIRE(c.kind == 2 || c.kind == 3, "not an error integrator");
  const MHArgs2<P1, Q1> a = mh_args2<P1, Q1>(c);
  const int epb = kMHWaves * L::EPW;
  const dim3 grid((c.ms.ne + epb - 1) / epb), block(64 * kMHWaves);
  const size_t lds = sizeof(double) * (size_t)epb * L::ELEM_PAD;
  if (c.kind == 2)
    hipLaunchKernelGGL((mixed_hex_error2_kernel<P1, Q1, true, FE>), grid, block, lds, c.s, a);
  else
    hipLaunchKernelGGL((mixed_hex_error2_kernel<P1, Q1, false, FE>), grid, block, lds, c.s, a);
  PA_HIP(hipGetLastError());
}

// The pairs the two-part kernels are compiled for, apply and error.  No instantiation with scratch or SGPR spills is on a list
// (profiles/r11_two_part_resources.txt): the error kernel of orders 3 and 4 at five points per direction spills in either form
// and keeps two one-part launches.  c == nullptr: only the question whether the pair is compiled in.
bool mh_apply2_case(const int p, const int q1d, const MH2Call *c) {
#define PA_MIXED2_CASE(P, Q1D)               \
  case P * 16 + Q1D:                         \
    if (c) mh_launch_apply2_pq<P, Q1D>(*c);  \
    return true;
  switch (p * 16 + q1d) {
    PA_MIXED2_CASE(1, 2) PA_MIXED2_CASE(1, 3) PA_MIXED2_CASE(2, 3) PA_MIXED2_CASE(1, 4) PA_MIXED2_CASE(2, 4)
    PA_MIXED2_CASE(3, 4) PA_MIXED2_CASE(1, 5) PA_MIXED2_CASE(2, 5) PA_MIXED2_CASE(3, 5) PA_MIXED2_CASE(4, 5)
  }
#undef PA_MIXED2_CASE
  return false;
}
bool mh_error2_case(const int p, const int q1d, const MH2Call *c) {
#define PA_ERROR2_CASE(P, Q1D)               \
  case P * 16 + Q1D:                         \
    if (c) mh_launch_error2_pq<P, Q1D>(*c);  \
    return true;
  switch (p * 16 + q1d) {
    PA_ERROR2_CASE(1, 2) PA_ERROR2_CASE(1, 3) PA_ERROR2_CASE(2, 3) PA_ERROR2_CASE(1, 4) PA_ERROR2_CASE(2, 4)
    PA_ERROR2_CASE(3, 4) PA_ERROR2_CASE(1, 5) PA_ERROR2_CASE(2, 5)
  }
#undef PA_ERROR2_CASE
  return false;
}

}  // namespace

// one launch for both parts of a complex field: this pair of the operator's family is compiled in and PALACE_AMD_TWO_PART != 0
bool mixed_hex_two_part(const MixedSub &ms) {
  if (!ms.hex1 || !ms.hex2 || !two_part_enabled()) return false;
  return ms.error ? mh_error2_case(ms.hex1->p, ms.hex1->q1d, nullptr) : mh_apply2_case(ms.hex1->p, ms.hex1->q1d, nullptr);
}

// apply: x1, x1i -> the two E-vectors (d_ye, d_ye2) of the output block; error: (x1, x2), (x1i, x2i) -> out.  No transposed
// form: pa_op_mult2 has none, a transposed apply of both parts is two one-part applies (launch_mixed_hex).
void launch_mixed_hex2(const MixedSub &ms, const double *x1, const double *x2, const double *x1i, const double *x2i, double *out,
                       hipStream_t s) {
  PA_REQUIRE(mixed_hex_two_part(ms), "no two-part kernel for this two-space operator");
  SubOp &so = *ms.hex1, &s2 = *ms.hex2;
  PA_REQUIRE(ms.error || s2.d_ye, "two-space blocks use the gather form of E^T");
  if (!ms.error && !s2.d_ye2) s2.d_ye2 = dev_alloc<double>((size_t)s2.ne * s2.P);
  const MH2Call c{so, s2, ms, ms.kind, x1, x2, x1i, x2i, out, s};
  const bool ok = ms.error ? mh_error2_case(so.p, so.q1d, &c) : mh_apply2_case(so.p, so.q1d, &c);
  PA_REQUIRE(ok, "no two-part kernel for this order and quadrature rule");
}

}  // namespace pa
