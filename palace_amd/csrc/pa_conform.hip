// Conforming prolongation P = [I; C] of a space with hanging-entity constraints and its transpose (linalg.hpp: Conforming).
//
// The reference applies P as a sparse matrix product wherever a ParOperator, a transfer or a diagonal needs it
// (linalg/rap.cpp:163-175, :195-361).  Here both products are one launch each.  The rows of C are short and ragged -- 1 to 36
// entries forward (p or p (p + 1) for H(curl), up to (p + 1)^2 for H1), up to about 2 p (2 p + 1) transposed -- so one
// power-of-two group of lanes shares a row, sized once from the longest row of the object, and adds its partial sums with a
// fixed butterfly: the result does not depend on the launch.  The head of either product (the identity block) is plain
// coalesced double2 traffic in the same launch: the first blocks of the grid copy, the others do the rows.
//
//   Prolongate: lx[i] = x[i] (0 where masked), lx[n_true + r] = sum_j C[r, j] x[j] (masked the same way)
//   Restrict:   y[i] = ly[i] + sum_r C[r, i] ly[n_true + r], gathered through the inverted index (per touched true dof the
//               (slave, value) pairs in ascending slave order): no atomics, no memset, bitwise reproducible; the epilogue adds
//               into y, takes |C| (the diagonal: the reference uses AbsMultTranspose for an AMR mesh, rap.cpp:163-175, because
//               the signed product does not give a convergent diagonal) and sets the essential rows of ParOperator::Mult.
//               The copy part leaves the touched dofs to the gather part, so every entry of y is written by one thread.
//
// Across ranks the object owns P = [I; C] P_halo (the reference's one parallel matrix, rap.cpp:195-234): the products come apart
// around the halo's exchange -- masked copy / exchange / rows in place, fold into a scratch prefix / exchange / epilogue -- with
// the same lane groups and the same order of operations.
//
// Six kernels: k_conform_prolongate<L, VEC, TWO> and k_conform_restrict<L, VEC, TWO> (one rank, one launch per product) and the
// pieces k_conform_copy_masked<VEC, TWO>, k_conform_rows<L, TWO>, k_conform_fold<L, VEC, TWO>, k_conform_epilogue<VEC, TWO>.
// L lanes share one row; VEC: every vector of the call is 16-byte aligned (double2 traffic); TWO: the second vector of a
// complex field rides in the same launch -- the index arrays, the values, `touched` and the mask are read once -- and goes
// through the operations of a one-vector launch in the same order, so either part is bit-identical to a one-vector launch on
// it.  A TWO = false kernel never dereferences its second pointers.  The arithmetic is written once, in the four device
// functions the kernels share: copy_masked_pair, row_sums, gather_sums and epilogue_pair.
#include <algorithm>
#include <cmath>
#include <string>
#include <type_traits>
#include <vector>

#include "comm.hpp"
#include "linalg.hpp"

namespace palace {

namespace {

constexpr int kBlock = 256;

template <int L>
__device__ __forceinline__ double group_sum(double s) {
#pragma unroll
  for (int o = L / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, L);
  return s;
}

template <bool VEC>
__device__ __forceinline__ double2 load2(const double *p, const int i) {
  if (VEC) return *reinterpret_cast<const double2 *>(p + i);
  double2 v;
  v.x = p[i], v.y = p[i + 1];
  return v;
}

template <bool VEC>
__device__ __forceinline__ void store2(double *p, const int i, const double2 v) {
  if (VEC) {
    *reinterpret_cast<double2 *>(p + i) = v;
  } else {
    p[i] = v.x, p[i + 1] = v.y;
  }
}

// The thread's two entries i, i + 1 of a head (i even; with an odd n_true the last thread has one entry), masked copy:
// lx[i] = x[i], 0 where the mask is set
template <bool VEC, bool TWO>
__device__ __forceinline__ void copy_masked_pair(const int n_true, const double *x0, const double *x1, const uint8_t *mask,
                                                 double *lx0, double *lx1) {
  const int i = 2 * ((int)blockIdx.x * kBlock + (int)threadIdx.x);
  if (i + 1 < n_true) {
    double2 v0 = load2<VEC>(x0, i), v1 = v0;
    if (TWO) v1 = load2<VEC>(x1, i);
    if (mask) {
      if (mask[i] & 1) v0.x = 0.0, v1.x = 0.0;
      if (mask[i + 1] & 1) v0.y = 0.0, v1.y = 0.0;
    }
    store2<VEC>(lx0, i, v0);
    if (TWO) store2<VEC>(lx1, i, v1);
  } else if (i < n_true) {
    const bool m = mask && (mask[i] & 1);
    lx0[i] = m ? 0.0 : x0[i];
    if (TWO) lx1[i] = m ? 0.0 : x1[i];
  }
}

// s = sum_j C[r, j] x[j] (x read as zero where the mask is set) on every lane of the group that shares row r: lane l adds the
// entries l, l + L, ... of the row in that order, then the butterfly.  Whole groups share r, so every lane of a group comes
// here, also with r >= n_con.  x carries no __restrict__: k_conform_rows reads the vector it writes.
template <int L, bool TWO>
__device__ __forceinline__ double2 row_sums(const int r, const int lane, const int n_con, const int *row_ptr, const int32_t *col,
                                            const double *val, const double *x0, const double *x1, const uint8_t *mask) {
  double s0 = 0.0, s1 = 0.0;
  if (r < n_con) {
    const int e = row_ptr[r + 1];
    for (int k = row_ptr[r] + lane; k < e; k += L) {
      const int j = col[k];
      const bool m = mask && (mask[j] & 1);
      const double v = val[k];
      const double xj0 = m ? 0.0 : x0[j];
      s0 += v * xj0;
      if (TWO) {
        const double xj1 = m ? 0.0 : x1[j];
        s1 += v * xj1;
      }
    }
  }
  s0 = group_sum<L>(s0);
  if (TWO) s1 = group_sum<L>(s1);
  return make_double2(s0, s1);
}

// s = sum_r C[r, i] ly[n_head + r] (|C| with abs_values) for the t-th touched dof i, through the inverted index: the same lane
// order and butterfly as row_sums
template <int L, bool TWO>
__device__ __forceinline__ double2 gather_sums(const int t, const int lane, const int n_touched, const int n_head, const int *t_ptr,
                                               const int32_t *t_slave, const double *t_val, const double *ly0, const double *ly1,
                                               const bool abs_values) {
  double s0 = 0.0, s1 = 0.0;
  if (t < n_touched) {
    const int e = t_ptr[t + 1];
    const double *tail0 = ly0 + n_head, *tail1 = TWO ? ly1 + n_head : nullptr;
    if (abs_values) {
      for (int k = t_ptr[t] + lane; k < e; k += L) {
        const double v = fabs(t_val[k]);
        const int sl = t_slave[k];
        s0 += v * tail0[sl];
        if (TWO) s1 += v * tail1[sl];
      }
    } else {
      for (int k = t_ptr[t] + lane; k < e; k += L) {
        const double v = t_val[k];
        const int sl = t_slave[k];
        s0 += v * tail0[sl];
        if (TWO) s1 += v * tail1[sl];
      }
    }
  }
  s0 = group_sum<L>(s0);
  if (TWO) s1 = group_sum<L>(s1);
  return make_double2(s0, s1);
}

__device__ __forceinline__ double restrict_value(const double v, const int i, const int flags, const double a,
                                                 const uint8_t *__restrict__ mask, const double *__restrict__ x_ess,
                                                 const double *__restrict__ y) {
  double out = v;
  if (mask && (mask[i] & 1) && (flags & (Conforming::FIX_ONE | Conforming::FIX_ZERO)))
    out = (flags & Conforming::FIX_ONE) ? x_ess[i] : 0.0;
  return (flags & Conforming::ADD) ? y[i] + a * out : out;
}

// The thread's two entries of a head, epilogue: y[i] = restrict_value(t[i]).  UNTOUCHED: only where `touched` is zero (the head
// blocks of k_conform_restrict leave the other entries to the gather part); otherwise `touched` is not read.  y may be x_ess:
// a thread reads x_ess[i] and y[i] before it writes y[i], and no other thread touches entry i.
template <bool VEC, bool TWO, bool UNTOUCHED>
__device__ __forceinline__ void epilogue_pair(const int n_true, const double *t0, const double *t1, const uint8_t *touched,
                                              const int flags, const double a, const uint8_t *mask, const double *x_ess0,
                                              const double *x_ess1, double *y0, double *y1) {
  const int i = 2 * ((int)blockIdx.x * kBlock + (int)threadIdx.x);
  if (i + 1 < n_true) {
    double2 v0 = load2<VEC>(t0, i), v1 = v0;
    if (TWO) v1 = load2<VEC>(t1, i);
    const bool w0 = !UNTOUCHED || touched[i] == 0, w1 = !UNTOUCHED || touched[i + 1] == 0;
    if (w0) v0.x = restrict_value(v0.x, i, flags, a, mask, x_ess0, y0);
    if (w1) v0.y = restrict_value(v0.y, i + 1, flags, a, mask, x_ess0, y0);
    if (TWO && w0) v1.x = restrict_value(v1.x, i, flags, a, mask, x_ess1, y1);
    if (TWO && w1) v1.y = restrict_value(v1.y, i + 1, flags, a, mask, x_ess1, y1);
    if (!UNTOUCHED || (VEC && w0 && w1)) {
      store2<VEC>(y0, i, v0);
      if (TWO) store2<VEC>(y1, i, v1);
    } else {
      if (w0) y0[i] = v0.x;
      if (w1) y0[i + 1] = v0.y;
      if (TWO && w0) y1[i] = v1.x;
      if (TWO && w1) y1[i + 1] = v1.y;
    }
  } else if (i < n_true) {
    if (!UNTOUCHED || !touched[i]) {
      y0[i] = restrict_value(t0[i], i, flags, a, mask, x_ess0, y0);
      if (TWO) y1[i] = restrict_value(t1[i], i, flags, a, mask, x_ess1, y1);
    }
  }
}

// ---- one rank: either product in one launch ---------------------------------------------------------------------------------
// blocks [0, head_blocks): two true dofs per thread; blocks after them: kBlock / L rows of C (of the inverted index) per block

template <int L, bool VEC, bool TWO>
__global__ __launch_bounds__(kBlock) void k_conform_prolongate(const int n_true, const int n_con, const int head_blocks,
                                                                const int *__restrict__ row_ptr, const int32_t *__restrict__ col,
                                                                const double *__restrict__ val, const double *__restrict__ x0,
                                                                const double *__restrict__ x1, const uint8_t *__restrict__ mask,
                                                                double *__restrict__ lx0, double *__restrict__ lx1) {
  if ((int)blockIdx.x < head_blocks) {
    copy_masked_pair<VEC, TWO>(n_true, x0, x1, mask, lx0, lx1);
    return;
  }
  const int lane = (int)threadIdx.x % L;
  const int r = ((int)blockIdx.x - head_blocks) * (kBlock / L) + (int)threadIdx.x / L;
  const double2 s = row_sums<L, TWO>(r, lane, n_con, row_ptr, col, val, x0, x1, mask);
  if (r < n_con && lane == 0) {
    lx0[n_true + r] = s.x;
    if (TWO) lx1[n_true + r] = s.y;
  }
}

// (y and x_ess carry no __restrict__: y may be x_ess)
template <int L, bool VEC, bool TWO>
__global__ __launch_bounds__(kBlock) void k_conform_restrict(const int n_true, const int n_touched, const int head_blocks,
                                                              const int *__restrict__ t_ptr, const int32_t *__restrict__ t_dof,
                                                              const int32_t *__restrict__ t_slave, const double *__restrict__ t_val,
                                                              const uint8_t *__restrict__ touched, const double *__restrict__ ly0,
                                                              const double *__restrict__ ly1, const int flags, const double a,
                                                              const uint8_t *__restrict__ mask, const double *x_ess0,
                                                              const double *x_ess1, double *y0, double *y1) {
  if ((int)blockIdx.x < head_blocks) {
    epilogue_pair<VEC, TWO, true>(n_true, ly0, ly1, touched, flags, a, mask, x_ess0, x_ess1, y0, y1);
    return;
  }
  const int lane = (int)threadIdx.x % L;
  const int t = ((int)blockIdx.x - head_blocks) * (kBlock / L) + (int)threadIdx.x / L;
  const double2 s = gather_sums<L, TWO>(t, lane, n_touched, n_true, t_ptr, t_slave, t_val, ly0, ly1, (flags & Conforming::ABS) != 0);
  if (t < n_touched && lane == 0) {
    const int i = t_dof[t];
    y0[i] = restrict_value(ly0[i] + s.x, i, flags, a, mask, x_ess0, y0);
    if (TWO) y1[i] = restrict_value(ly1[i] + s.y, i, flags, a, mask, x_ess1, y1);
  }
}

// ---- across ranks: P = [I; C] P_halo in pieces around the halo's exchange ---------------------------------------------------
// Local vector: owned true dofs [0, n_true), ghost true dofs [n_true, n_shared), constrained dofs [n_shared, n_local); C has
// n_shared columns.  The pieces are the parts of the one-launch kernels above as launches of their own (the same device
// functions), so with an empty halo they reproduce them bit for bit.

// masked copy x -> lx[0, n_true): the head blocks of k_conform_prolongate (the halo runs behind it)
template <bool VEC, bool TWO>
__global__ __launch_bounds__(kBlock) void k_conform_copy_masked(const int n_true, const double *__restrict__ x0,
                                                                 const double *__restrict__ x1, const uint8_t *__restrict__ mask,
                                                                 double *__restrict__ lx0, double *__restrict__ lx1) {
  copy_masked_pair<VEC, TWO>(n_true, x0, x1, mask, lx0, lx1);
}

// in-place rows: lx[n_shared + r] = sum_j C[r, j] lx[j]; reads the prefix only (col < n_shared, checked at set-up), writes the
// tail only, so lx carries no __restrict__.  No copy, no mask: the prefix was masked before the exchange, so the ghost copies
// of essential dofs are zero too.
template <int L, bool TWO>
__global__ __launch_bounds__(kBlock) void k_conform_rows(const int n_shared, const int n_con, const int *__restrict__ row_ptr,
                                                          const int32_t *__restrict__ col, const double *__restrict__ val,
                                                          double *lx0, double *lx1) {
  const int lane = (int)threadIdx.x % L;
  const int r = (int)blockIdx.x * (kBlock / L) + (int)threadIdx.x / L;
  const double2 s = row_sums<L, TWO>(r, lane, n_con, row_ptr, col, val, lx0, lx1, nullptr);
  if (r < n_con && lane == 0) {
    lx0[n_shared + r] = s.x;
    if (TWO) lx1[n_shared + r] = s.y;
  }
}

// fold into the prefix: t[j] = ly[j] + sum_r C[r, j] ly[n_shared + r] for every j < n_shared, ghost columns included (their
// sums travel to the owners with the halo's P^T); head blocks copy the columns nothing hangs on (a plain copy into the
// object's own scratch: no flags, no mask, t is __restrict__), one lane group per touched one
template <int L, bool VEC, bool TWO>
__global__ __launch_bounds__(kBlock) void k_conform_fold(const int n_shared, const int n_touched, const int head_blocks,
                                                          const int *__restrict__ t_ptr, const int32_t *__restrict__ t_dof,
                                                          const int32_t *__restrict__ t_slave, const double *__restrict__ t_val,
                                                          const uint8_t *__restrict__ touched, const double *__restrict__ ly0,
                                                          const double *__restrict__ ly1, const int abs_values,
                                                          double *__restrict__ t0, double *__restrict__ t1) {
  if ((int)blockIdx.x < head_blocks) {
    const int i = 2 * ((int)blockIdx.x * kBlock + (int)threadIdx.x);
    if (i + 1 < n_shared) {
      double2 v0 = load2<VEC>(ly0, i), v1 = v0;
      if (TWO) v1 = load2<VEC>(ly1, i);
      const bool c0 = touched[i] == 0, c1 = touched[i + 1] == 0;
      if (VEC && c0 && c1) {
        store2<true>(t0, i, v0);
        if (TWO) store2<true>(t1, i, v1);
      } else {
        if (c0) t0[i] = v0.x;
        if (c1) t0[i + 1] = v0.y;
        if (TWO && c0) t1[i] = v1.x;
        if (TWO && c1) t1[i + 1] = v1.y;
      }
    } else if (i < n_shared) {
      if (!touched[i]) {
        t0[i] = ly0[i];
        if (TWO) t1[i] = ly1[i];
      }
    }
    return;
  }
  const int lane = (int)threadIdx.x % L;
  const int t = ((int)blockIdx.x - head_blocks) * (kBlock / L) + (int)threadIdx.x / L;
  const double2 s = gather_sums<L, TWO>(t, lane, n_touched, n_shared, t_ptr, t_slave, t_val, ly0, ly1, abs_values != 0);
  if (t < n_touched && lane == 0) {
    const int i = t_dof[t];
    t0[i] = ly0[i] + s.x;
    if (TWO) t1[i] = ly1[i] + s.y;
  }
}

// epilogue on the owned part: y[i] = t[i] with ADD and the essential rows (what k_conform_restrict does with its sums)
template <bool VEC, bool TWO>
__global__ __launch_bounds__(kBlock) void k_conform_epilogue(const int n_true, const double *__restrict__ t0,
                                                              const double *__restrict__ t1, const int flags, const double a,
                                                              const uint8_t *__restrict__ mask, const double *x_ess0,
                                                              const double *x_ess1, double *y0, double *y1) {
  epilogue_pair<VEC, TWO, false>(n_true, t0, t1, nullptr, flags, a, mask, x_ess0, x_ess1, y0, y1);
}

int lanes_for(int longest) {
  int l = 1;
  while (l < longest && l < 32) l *= 2;
  return l;
}

// Run-time choices as the kernels' template arguments: f receives std::integral_constant objects (L() is a constant expression).
template <typename F>
void with_lanes(const int lanes, const char *product, F &&f) {
  switch (lanes) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 8: return f(std::integral_constant<int, 8>{});
    case 16: return f(std::integral_constant<int, 16>{});
    case 32: return f(std::integral_constant<int, 32>{});
    default: throw pa::Error(std::string("conforming ") + product + ": bad lane count");
  }
}

template <typename F>
void with_flag(const bool flag, F &&f) {
  flag ? f(std::true_type{}) : f(std::false_type{});
}

template <typename F>
void with_flags(const bool vec, const bool two, F &&f) {
  with_flag(vec, [&](auto vec_c) { with_flag(two, [&](auto two_c) { f(vec_c, two_c); }); });
}

int head_blocks(int n) { return ((n + 1) / 2 + kBlock - 1) / kBlock; }

int row_blocks(int n_rows, int lanes) { return (n_rows + kBlock / lanes - 1) / (kBlock / lanes); }

// the double2 forms need every vector pair of the call on a 16-byte boundary (b0, b1: the second vector, if any)
bool aligned16(const void *a0, const void *a1, const void *b0 = nullptr, const void *b1 = nullptr) {
  return (((uintptr_t)a0 | (uintptr_t)a1 | (uintptr_t)b0 | (uintptr_t)b1) & 15) == 0;
}

// true when [a, a + na) and [b, b + nb) share an element
bool overlap(const double *a, size_t na, const double *b, size_t nb) { return a && b && a < b + nb && b < a + na; }

}  // namespace

Conforming::Conforming(const Context &ctx, int n_true, int n_local, const int *row_ptr, const int32_t *col, const double *val)
    : n_true_(n_true), n_con_(n_local - n_true), n_shared_(n_true) {
  PA_REQUIRE(n_true >= 0 && n_local >= n_true, "conforming prolongation: bad sizes");
  BuildIndex(ctx, n_true, row_ptr, col, val);
}

Conforming::Conforming(const Context &ctx, int n_true, int n_shared, int n_local, const int *row_ptr, const int32_t *col,
                       const double *val, const Halo *halo)
    : n_true_(n_true), n_con_(n_local - n_shared), dist_(true), n_shared_(n_shared), halo_(halo) {
  PA_REQUIRE(n_true >= 0 && n_shared >= n_true && n_local >= n_shared, "distributed conforming prolongation: bad sizes");
  PA_REQUIRE(halo || n_shared == n_true, "distributed conforming prolongation: ghost true dofs need a halo plan");
  if (halo) halo->Validate(n_true, n_shared);  // the plan covers the prefix: constrained dofs are never communicated
  BuildIndex(ctx, n_shared, row_ptr, col, val);
  d_t_ = pa::dev_alloc<double>(2 * (((size_t)n_shared + 1) & ~(size_t)1));
}

// C by rows and C^T as an inverted index over its n_cols columns (the true dofs; across ranks the owned and the ghost ones)
void Conforming::BuildIndex(const Context &ctx, int n_cols, const int *row_ptr, const int32_t *col, const double *val) {
  PA_REQUIRE(n_cols + n_con_ < (1 << 30), "conforming prolongation: too many dofs for the 32-bit index arithmetic of the kernels");
  PA_REQUIRE(n_con_ == 0 || (row_ptr && row_ptr[0] == 0), "conforming prolongation: the row pointer must start at 0");
  const int nnz = n_con_ ? row_ptr[n_con_] : 0;
  PA_REQUIRE(nnz == 0 || (col && val), "conforming prolongation: null arrays");
  int longest = 0;
  std::vector<int> count((size_t)n_cols + 1, 0);
  for (int r = 0; r < n_con_; r++) {
    PA_REQUIRE(row_ptr[r + 1] >= row_ptr[r] && row_ptr[r + 1] <= nnz, "conforming prolongation: the row pointer must not decrease");
    longest = std::max(longest, row_ptr[r + 1] - row_ptr[r]);
    for (int k = row_ptr[r]; k < row_ptr[r + 1]; k++) {
      // one-irregular meshes: every column is a true dof (no chains of constraints)
      PA_REQUIRE(col[k] >= 0 && col[k] < n_cols, "conforming prolongation: a constraint refers to a dof that is not a true dof");
      count[col[k] + 1]++;
    }
  }
  fwd_lanes_ = lanes_for(longest);
  // C^T as an inverted index over the touched true dofs; rows of C are visited in ascending order, so every list is in
  // ascending slave order
  std::vector<int32_t> t_dof;
  std::vector<int> t_ptr{0}, slot((size_t)n_cols, -1);
  std::vector<uint8_t> touched((size_t)n_cols, 0);
  int longest_t = 0;
  for (int i = 0; i < n_cols; i++) {
    if (!count[i + 1]) continue;
    slot[i] = (int)t_dof.size();
    t_dof.push_back(i);
    t_ptr.push_back(t_ptr.back() + count[i + 1]);
    touched[i] = 1;
    longest_t = std::max(longest_t, count[i + 1]);
  }
  n_touched_ = (int)t_dof.size();
  tr_lanes_ = lanes_for(longest_t);
  std::vector<int32_t> t_slave((size_t)nnz);
  std::vector<double> t_val((size_t)nnz);
  std::vector<int> fill(t_ptr.begin(), t_ptr.end() - 1);
  for (int r = 0; r < n_con_; r++)
    for (int k = row_ptr[r]; k < row_ptr[r + 1]; k++) {
      const int at = fill[slot[col[k]]]++;
      t_slave[at] = r, t_val[at] = val[k];
    }
  const int zero = 0;
  d_row_ptr_ = pa::dev_upload(n_con_ ? row_ptr : &zero, (size_t)n_con_ + 1, ctx.stream);
  d_col_ = pa::dev_upload(col, (size_t)nnz, ctx.stream);
  d_val_ = pa::dev_upload(val, (size_t)nnz, ctx.stream);
  d_t_ptr_ = pa::dev_upload(t_ptr.data(), t_ptr.size(), ctx.stream);
  d_t_dof_ = pa::dev_upload(t_dof.data(), t_dof.size(), ctx.stream);
  d_t_slave_ = pa::dev_upload(t_slave.data(), t_slave.size(), ctx.stream);
  d_t_val_ = pa::dev_upload(t_val.data(), t_val.size(), ctx.stream);
  d_touched_ = pa::dev_upload(touched.data(), touched.size(), ctx.stream);
  d_t_slot_ = pa::dev_upload(slot.data(), slot.size(), ctx.stream);
}

Conforming::~Conforming() = default;

void Conforming::Prolongate(const double *x, double *lx, const uint8_t *ess_mask, hipStream_t stream) const {
  ProlongateParts(x, nullptr, lx, nullptr, ess_mask, stream);
}

void Conforming::Prolongate2(const double *x0, const double *x1, double *lx0, double *lx1, const uint8_t *ess_mask,
                             hipStream_t stream) const {
  ProlongateParts(x0, x1, lx0, lx1, ess_mask, stream);
}

void Conforming::Restrict(const double *ly, double *y, int flags, double a, const uint8_t *ess_mask, const double *x_ess,
                          hipStream_t stream) const {
  RestrictParts(ly, nullptr, y, nullptr, flags, a, ess_mask, x_ess, nullptr, stream);
}

void Conforming::Restrict2(const double *ly0, const double *ly1, double *y0, double *y1, int flags, double a, const uint8_t *ess_mask,
                           const double *x_ess0, const double *x_ess1, hipStream_t stream) const {
  RestrictParts(ly0, ly1, y0, y1, flags, a, ess_mask, x_ess0, x_ess1, stream);
}

// Both entry points of P.  x1 == nullptr: one vector.
void Conforming::ProlongateParts(const double *x0, const double *x1, double *lx0, double *lx1, const uint8_t *ess_mask,
                                 hipStream_t stream) const {
  const bool two = x1 != nullptr;
  if (two) {
    const size_t nt = (size_t)n_true_, nl = (size_t)n_shared_ + n_con_;
    PA_REQUIRE(!overlap(lx0, nl, lx1, nl) && !overlap(lx0, nl, x0, nt) && !overlap(lx0, nl, x1, nt) && !overlap(lx1, nl, x0, nt) &&
                   !overlap(lx1, nl, x1, nt),
               "conforming prolongation of two vectors: the outputs must not overlap each other or the inputs");
  }
  if (dist_) return ProlongateDist(x0, x1, lx0, lx1, ess_mask, stream);  // (stays collective: ProlongateDist decides what is empty)
  if (n_true_ + n_con_ == 0) return;
  const int head = head_blocks(n_true_);
  with_lanes(fwd_lanes_, "prolongation", [&](auto L) {
    with_flags(aligned16(x0, lx0, x1, lx1), two, [&](auto VEC, auto TWO) {
      hipLaunchKernelGGL((k_conform_prolongate<L(), VEC(), TWO()>), dim3(head + row_blocks(n_con_, L())), dim3(kBlock), 0, stream,
                         n_true_, n_con_, head, d_row_ptr_, d_col_, d_val_, x0, x1, ess_mask, lx0, lx1);
    });
  });
  PA_HIP(hipGetLastError());
}

// Both entry points of P^T, with their argument checks.  ly1 == nullptr: one vector.
void Conforming::RestrictParts(const double *ly0, const double *ly1, double *y0, double *y1, int flags, double a,
                               const uint8_t *ess_mask, const double *x_ess0, const double *x_ess1, hipStream_t stream) const {
  const bool two = ly1 != nullptr;
  PA_REQUIRE(!((flags & FIX_ONE) && ess_mask) || (x_ess0 && (!two || x_ess1)),
             "conforming restriction: FIX_ONE needs the vector the essential rows copy");
  PA_REQUIRE(!((flags & FIX_ONE) && (flags & FIX_ZERO)), "conforming restriction: one policy for the essential rows");
  if (two) {
    const size_t nt = (size_t)n_true_, nl = (size_t)n_shared_ + n_con_;
    PA_REQUIRE(!overlap(y0, nt, y1, nt) && !overlap(y0, nt, ly0, nl) && !overlap(y0, nt, ly1, nl) && !overlap(y1, nt, ly0, nl) &&
                   !overlap(y1, nt, ly1, nl),
               "conforming restriction of two vectors: the outputs must not overlap each other or the inputs");
  }
  if (dist_) return RestrictDist(ly0, ly1, y0, y1, flags, a, ess_mask, x_ess0, x_ess1, stream);  // (collective, as above)
  if (n_true_ == 0) return;
  const int head = head_blocks(n_true_);
  with_lanes(tr_lanes_, "restriction", [&](auto L) {
    with_flags(aligned16(ly0, y0, ly1, y1), two, [&](auto VEC, auto TWO) {
      hipLaunchKernelGGL((k_conform_restrict<L(), VEC(), TWO()>), dim3(head + row_blocks(n_touched_, L())), dim3(kBlock), 0, stream,
                         n_true_, n_touched_, head, d_t_ptr_, d_t_dof_, d_t_slave_, d_t_val_, d_touched_, ly0, ly1, flags, a, ess_mask,
                         x_ess0, x_ess1, y0, y1);
    });
  });
  PA_HIP(hipGetLastError());
}

// P = [I; C] P_halo: masked copy, the halo's exchange on the prefix, the rows of C in place.  x1 == nullptr: one vector.
void Conforming::ProlongateDist(const double *x0, const double *x1, double *lx0, double *lx1, const uint8_t *ess_mask,
                                hipStream_t stream, int pieces) const {
  if (n_shared_ + n_con_ == 0 && !halo_) return;
  const bool two = x1 != nullptr;
  if (n_true_ && (pieces & 1)) {
    with_flags(aligned16(x0, lx0, x1, lx1), two, [&](auto VEC, auto TWO) {
      hipLaunchKernelGGL((k_conform_copy_masked<VEC(), TWO()>), dim3(head_blocks(n_true_)), dim3(kBlock), 0, stream, n_true_, x0, x1,
                         ess_mask, lx0, lx1);
    });
  }
  if (halo_ && (pieces & 2)) {  // (every rank of the plan comes here, with or without dofs of its own: the exchange is collective)
    halo_->Prolongate(lx0, stream);
    if (two) halo_->Prolongate(lx1, stream);
  }
  if (n_con_ && (pieces & 4)) {
    with_lanes(fwd_lanes_, "prolongation", [&](auto L) {
      with_flag(two, [&](auto TWO) {
          hipLaunchKernelGGL((k_conform_rows<L(), TWO()>), dim3(row_blocks(n_con_, L())), dim3(kBlock), 0, stream, n_shared_, n_con_,
                           d_row_ptr_, d_col_, d_val_, lx0, lx1);
      });
    });
  }
  PA_HIP(hipGetLastError());
}

// P^T = P_halo^T [I C^T]: fold the tail into the prefix (scratch t, the caller's ly stays const), the halo sums the ghosts of t
// into their owners, the epilogue writes the owned part.  ly1 == nullptr: one vector.
void Conforming::RestrictDist(const double *ly0, const double *ly1, double *y0, double *y1, int flags, double a,
                              const uint8_t *ess_mask, const double *x_ess0, const double *x_ess1, hipStream_t stream,
                              int pieces) const {
  if (n_shared_ == 0 && !halo_) return;
  const bool two = ly1 != nullptr;
  double *t0 = d_t_, *t1 = two ? d_t_ + (((size_t)n_shared_ + 1) & ~(size_t)1) : nullptr;
  if (n_shared_ && (pieces & 1)) {
    const int head = head_blocks(n_shared_);
    const int abs_values = (flags & ABS) ? 1 : 0;
    with_lanes(tr_lanes_, "restriction", [&](auto L) {
      with_flags(aligned16(ly0, t0, ly1, t1), two, [&](auto VEC, auto TWO) {
          hipLaunchKernelGGL((k_conform_fold<L(), VEC(), TWO()>), dim3(head + row_blocks(n_touched_, L())), dim3(kBlock), 0, stream,
                           n_shared_, n_touched_, head, d_t_ptr_, d_t_dof_, d_t_slave_, d_t_val_, d_touched_, ly0, ly1, abs_values, t0,
                           t1);
      });
    });
  }
  if (halo_ && (pieces & 2)) {
    halo_->RestrictAdd(t0, stream);
    if (two) halo_->RestrictAdd(t1, stream);
  }
  if (n_true_ && (pieces & 4)) {
    with_flags(aligned16(t0, y0, t1, y1), two, [&](auto VEC, auto TWO) {
      hipLaunchKernelGGL((k_conform_epilogue<VEC(), TWO()>), dim3(head_blocks(n_true_)), dim3(kBlock), 0, stream, n_true_, t0, t1,
                         flags, a, ess_mask, x_ess0, x_ess1, y0, y1);
    });
  }
  PA_HIP(hipGetLastError());
}

void Conforming::TimePieces(const double *x, double *lx, const double *ly, double *y, const uint8_t *ess_mask, int reps, double *us,
                            hipStream_t stream) const {
  StreamGraph::RequireNotRecording("timing the pieces of a conforming prolongation");
  PA_REQUIRE(dist_ && reps > 0 && us, "the pieces are those of a conforming prolongation that carries a halo");
  hipEvent_t e0, e1;
  PA_HIP(hipEventCreate(&e0));
  PA_HIP(hipEventCreate(&e1));
  const int fix = ess_mask ? FIX_ONE : 0;
  for (int k = 0; k < 6; k++) {
    const int piece = 1 << (k % 3);
    auto run = [&] {
      if (k < 3)
        ProlongateDist(x, nullptr, lx, nullptr, ess_mask, stream, piece);
      else
        RestrictDist(ly, nullptr, y, nullptr, fix, 1.0, ess_mask, x, nullptr, stream, piece);
    };
    for (int i = 0; i < 5; i++) run();
    PA_HIP(hipEventRecord(e0, stream));
    for (int i = 0; i < reps; i++) run();
    PA_HIP(hipEventRecord(e1, stream));
    PA_HIP(hipEventSynchronize(e1));
    float ms = 0.0f;
    PA_HIP(hipEventElapsedTime(&ms, e0, e1));
    us[k] = 1e3 * (double)ms / reps;
  }
  PA_HIP(hipEventDestroy(e0));
  PA_HIP(hipEventDestroy(e1));
}

}  // namespace palace
