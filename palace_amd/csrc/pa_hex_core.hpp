// What the tensor-product hexahedron kernel families share (H(curl): pa_nd_hex*.hip, H1: pa_h1_hex*.hip, H(div):
// pa_rt_hex.hip): the accessors of mirror-symmetric half tables stored as whole rows, the dense LDS layout of the contraction
// buffers and the list of supported (order, points per direction) pairs with its dispatch.  The mapping of elements and lines
// to lanes is described at the top of pa_nd_hex.hip.
#pragma once

#include <string>

#include "pa_internal.hpp"
#include "pa_device.hpp"

namespace pa {

// The 1-D tables are mirror-symmetric (Gauss-Legendre / Gauss-Lobatto nodes and points):
//   B[q][i] = B[Q1-1-q][N-1-i],  G[q][i] = -G[Q1-1-q][N-1-i],
// so only the first (Q1+1)/2 rows travel as kernel arguments (scalar operands of the FMAs) and rows q >= (Q1+1)/2 are read
// from their mirror image.  q and i are compile-time constants after unrolling.
//
// There are two storage forms.  The H(curl) kernels truncate the middle row of an odd rule to its first half (HalfTab,
// tab_even / tab_odd in pa_nd_hex_core.hpp); the H1 and H(div) kernels store whole rows and read them with half_even /
// half_odd below, where MIRROR_MID says whether the second half of that middle row is read from its first half (H(div)) or
// as stored (H1; the two agree for even Q1).  The forms are not interchangeable for free: with the truncated form 53 of 62
// H1 and 48 of 62 H(div) instantiations compiled to different code, and with MIRROR_MID the 36 odd-Q1 H1 instantiations did
// (h1_hex_apply_kernel<1, 5, V, G, packed>: 116 -> 130 VGPRs, across the occupancy step at 128), so each family keeps its own.
template <int N, int Q1, bool MIRROR_MID = false>
__device__ __forceinline__ double half_even(const double *H, const int q, const int i) {
  const bool flip = q >= (Q1 + 1) / 2 || (MIRROR_MID && (Q1 & 1) && q == Q1 / 2 && 2 * i > N - 1);
  return flip ? H[(Q1 - 1 - q) * N + (N - 1 - i)] : H[q * N + i];
}
template <int N, int Q1, bool MIRROR_MID = false>
__device__ __forceinline__ double half_odd(const double *H, const int q, const int i) {
  const bool flip = q >= (Q1 + 1) / 2 || (MIRROR_MID && (Q1 & 1) && q == Q1 / 2 && 2 * i > N - 1);
  return flip ? -H[(Q1 - 1 - q) * N + (N - 1 - i)] : H[q * N + i];
}

// Dense LDS layout of one element: BASE doubles of the family's own (the H(div) kernel keeps its dofs there), then NA fields
// A[f][qx][j][k] (after pass X) and NB fields B[f][qx][qy][k] (after pass Y).  The element stride is an odd multiple of 16
// doubles, so the two elements of a 32-lane read group land on opposite halves of the 64 banks.  (The H(curl) kernels have
// padded and swizzled layouts of their own: NDLayout in pa_nd_hex_core.hpp.)
template <int P1, int Q1, int BASE_, int NA, int NB>
struct HexLayout {
  static constexpr int NC = P1 + 1;
  static constexpr int T = Q1 * Q1;
  static constexpr int EPW = 64 / T;
  static constexpr int BASE = BASE_;
  static constexpr int A_FIELD = Q1 * NC * NC;
  static constexpr int B_FIELD = Q1 * Q1 * NC;
  static constexpr int ELEM = BASE + NA * A_FIELD + NB * B_FIELD;
  static constexpr int ELEM_PAD = ((ELEM + 15) / 16 * 16) | 16;
  __device__ static __forceinline__ int ia(int f, int qx, int j, int k) { return BASE + f * A_FIELD + (qx * NC + j) * NC + k; }
  __device__ static __forceinline__ int ib(int f, int qx, int qy, int k) {
    return BASE + NA * A_FIELD + f * B_FIELD + (qx * Q1 + qy) * NC + k;
  }
};

// H1 (pa_h1_hex.hip, pa_h1_hex_stream.hip): value and x-derivative chains after pass X; value, y- and x-derivative after Y
template <int P1, int Q1>
using H1Layout = HexLayout<P1, Q1, 0, 2, 3>;

// The (order, points per direction) pairs the element kernels are instantiated for: X(p, q1d, ...) for each.
#define PA_HEX_PQ_LIST(X, ...)                                                                                       \
  X(1, 2, __VA_ARGS__) X(1, 3, __VA_ARGS__) X(2, 3, __VA_ARGS__) X(1, 4, __VA_ARGS__) X(2, 4, __VA_ARGS__)           \
  X(3, 4, __VA_ARGS__) X(1, 5, __VA_ARGS__) X(2, 5, __VA_ARGS__) X(3, 5, __VA_ARGS__) X(4, 5, __VA_ARGS__)
#define PA_HEX_PQ_LABEL(P, Q, ...) case P * 16 + Q:
#define PA_HEX_PQ_CALL(P, Q, FN, ...) case P * 16 + Q: FN<P, Q>(__VA_ARGS__); break;

// Six points per direction: the order-5 operators and the coarser levels of their p-multigrid hierarchy.  A list of its own
// -- every family serves these pairs with kernels fitted to 36 lanes per element (pa_nd_hex_q6.hip, pa_h1_hex_q6.hip,
// pa_rt_hex_q6.hip, pa_mixed_hex_q6.hip); the both-parts-per-pass kernels (pa_rt_hex2.hip, pa_mixed_hex2.hip) stop at five points.
#define PA_HEX_Q6_LIST(X, ...) \
  X(1, 6, __VA_ARGS__) X(2, 6, __VA_ARGS__) X(3, 6, __VA_ARGS__) X(4, 6, __VA_ARGS__) X(5, 6, __VA_ARGS__)

inline bool hex_pq_supported(int p, int q1d) {
  switch (p * 16 + q1d) {
    PA_HEX_PQ_LIST(PA_HEX_PQ_LABEL, ) return true;
  }
  return false;
}
inline bool hex_q6_supported(int p, int q1d) {
  switch (p * 16 + q1d) {
    PA_HEX_Q6_LIST(PA_HEX_PQ_LABEL, ) return true;
  }
  return false;
}
// what: the family as the message names it ("H(curl)", "H1", "H(div)")
inline Error hex_pq_error(const char *what, int p, int q1d) {
  return Error(std::string("no ") + what + " hex kernel for order " + std::to_string(p) + " with " + std::to_string(q1d) +
               " points per direction");
}
// FN<p, q1d>(...) for the pair of the SubOp `so` in scope
#define PA_HEX_DISPATCH(FN, what, ...)                           \
  switch (so.p * 16 + so.q1d) {                                  \
    PA_HEX_PQ_LIST(PA_HEX_PQ_CALL, FN, __VA_ARGS__)              \
    default: throw hex_pq_error(what, so.p, so.q1d);             \
  }

}  // namespace pa
