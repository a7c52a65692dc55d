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
#include <algorithm>
#include <cmath>
#include <vector>

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

// blocks [0, head_blocks): two true dofs per thread; blocks after them: kBlock / L rows of C per block
template <int L, bool VEC>
__global__ __launch_bounds__(kBlock) void k_conform_prolongate(const int n_true, const int n_con, const int head_blocks,
                                                                const int *__restrict__ row_ptr, const int32_t *__restrict__ col,
                                                                const double *__restrict__ val, const double *__restrict__ x,
                                                                const uint8_t *__restrict__ mask, double *__restrict__ lx) {
  if ((int)blockIdx.x < head_blocks) {
    const int i = 2 * ((int)blockIdx.x * kBlock + (int)threadIdx.x);
    if (i + 1 < n_true) {
      double2 v;
      if (VEC) {
        v = *reinterpret_cast<const double2 *>(x + i);
      } else {
        v.x = x[i], v.y = x[i + 1];
      }
      if (mask) {
        if (mask[i] & 1) v.x = 0.0;
        if (mask[i + 1] & 1) v.y = 0.0;
      }
      if (VEC) {
        *reinterpret_cast<double2 *>(lx + i) = v;
      } else {
        lx[i] = v.x, lx[i + 1] = v.y;
      }
    } else if (i < n_true) {
      lx[i] = (mask && (mask[i] & 1)) ? 0.0 : x[i];
    }
    return;
  }
  const int lane = (int)threadIdx.x % L;
  const int r = ((int)blockIdx.x - head_blocks) * (kBlock / L) + (int)threadIdx.x / L;
  double s = 0.0;
  if (r < n_con) {  // (whole groups share r: the butterfly below runs with every lane of the group)
    const int e = row_ptr[r + 1];
    for (int k = row_ptr[r] + lane; k < e; k += L) {
      const int j = col[k];
      const double xj = (mask && (mask[j] & 1)) ? 0.0 : x[j];
      s += val[k] * xj;
    }
  }
  s = group_sum<L>(s);
  if (r < n_con && lane == 0) lx[n_true + r] = s;
}

__device__ __forceinline__ double restrict_value(const double v, const int i, const int flags, const double a,
                                                 const uint8_t *__restrict__ mask, const double *__restrict__ x_ess,
                                                 const double *__restrict__ y) {
  double out = v;
  if (mask && (mask[i] & 1) && (flags & (Conforming::FIX_ONE | Conforming::FIX_ZERO)))
    out = (flags & Conforming::FIX_ONE) ? x_ess[i] : 0.0;
  return (flags & Conforming::ADD) ? y[i] + a * out : out;
}

template <int L, bool VEC>
__global__ __launch_bounds__(kBlock) void k_conform_restrict(const int n_true, const int n_touched, const int head_blocks,
                                                              const int *__restrict__ t_ptr, const int32_t *__restrict__ t_dof,
                                                              const int32_t *__restrict__ t_slave, const double *__restrict__ t_val,
                                                              const uint8_t *__restrict__ touched, const double *__restrict__ ly,
                                                              const int flags, const double a, const uint8_t *__restrict__ mask,
                                                              const double *x_ess, double *y) {
  if ((int)blockIdx.x < head_blocks) {
    const int i = 2 * ((int)blockIdx.x * kBlock + (int)threadIdx.x);
    if (i + 1 < n_true) {
      double2 v;
      if (VEC) {
        v = *reinterpret_cast<const double2 *>(ly + i);
      } else {
        v.x = ly[i], v.y = ly[i + 1];
      }
      const bool t0 = touched[i] != 0, t1 = touched[i + 1] != 0;
      if (!t0) v.x = restrict_value(v.x, i, flags, a, mask, x_ess, y);
      if (!t1) v.y = restrict_value(v.y, i + 1, flags, a, mask, x_ess, y);
      if (VEC && !t0 && !t1) {
        *reinterpret_cast<double2 *>(y + i) = v;
      } else {
        if (!t0) y[i] = v.x;
        if (!t1) y[i + 1] = v.y;
      }
    } else if (i < n_true) {
      if (!touched[i]) y[i] = restrict_value(ly[i], i, flags, a, mask, x_ess, y);
    }
    return;
  }
  const int lane = (int)threadIdx.x % L;
  const int t = ((int)blockIdx.x - head_blocks) * (kBlock / L) + (int)threadIdx.x / L;
  double s = 0.0;
  if (t < n_touched) {
    const int e = t_ptr[t + 1];
    const double *tail = ly + n_true;
    if (flags & Conforming::ABS) {
      for (int k = t_ptr[t] + lane; k < e; k += L) s += fabs(t_val[k]) * tail[t_slave[k]];
    } else {
      for (int k = t_ptr[t] + lane; k < e; k += L) s += t_val[k] * tail[t_slave[k]];
    }
  }
  s = group_sum<L>(s);
  if (t < n_touched && lane == 0) {
    const int i = t_dof[t];
    y[i] = restrict_value(ly[i] + s, i, flags, a, mask, x_ess, y);
  }
}

// ---- both parts of a complex field in one launch ---------------------------------------------------------------------------
// The same mapping (head blocks copy, one lane group per row, the butterfly of group_sum) with the index arrays, the values,
// `touched` and the mask read once for two vectors.  Either part goes through the operations of the one-vector kernel in the
// same order, so it is bit-identical to a one-vector launch on that part.
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

template <int L, bool VEC>
__global__ __launch_bounds__(kBlock) void k_conform_prolongate2(const int n_true, const int n_con, const int head_blocks,
                                                                 const int *__restrict__ row_ptr, const int32_t *__restrict__ col,
                                                                 const double *__restrict__ val, const double *__restrict__ x0,
                                                                 const double *__restrict__ x1, const uint8_t *__restrict__ mask,
                                                                 double *__restrict__ lx0, double *__restrict__ lx1) {
  if ((int)blockIdx.x < head_blocks) {
    const int i = 2 * ((int)blockIdx.x * kBlock + (int)threadIdx.x);
    if (i + 1 < n_true) {
      double2 v0 = load2<VEC>(x0, i), v1 = load2<VEC>(x1, i);
      if (mask) {
        if (mask[i] & 1) v0.x = 0.0, v1.x = 0.0;
        if (mask[i + 1] & 1) v0.y = 0.0, v1.y = 0.0;
      }
      store2<VEC>(lx0, i, v0);
      store2<VEC>(lx1, i, v1);
    } else if (i < n_true) {
      const bool m = mask && (mask[i] & 1);
      lx0[i] = m ? 0.0 : x0[i];
      lx1[i] = m ? 0.0 : x1[i];
    }
    return;
  }
  const int lane = (int)threadIdx.x % L;
  const int r = ((int)blockIdx.x - head_blocks) * (kBlock / L) + (int)threadIdx.x / L;
  double s0 = 0.0, s1 = 0.0;
  if (r < n_con) {
    const int e = row_ptr[r + 1];
    for (int k = row_ptr[r] + lane; k < e; k += L) {
      const int j = col[k];
      const bool m = mask && (mask[j] & 1);
      const double v = val[k];
      const double xj0 = m ? 0.0 : x0[j];
      const double xj1 = m ? 0.0 : x1[j];
      s0 += v * xj0;
      s1 += v * xj1;
    }
  }
  s0 = group_sum<L>(s0);
  s1 = group_sum<L>(s1);
  if (r < n_con && lane == 0) lx0[n_true + r] = s0, lx1[n_true + r] = s1;
}

template <int L, bool VEC>
__global__ __launch_bounds__(kBlock) void k_conform_restrict2(const int n_true, const int n_touched, const int head_blocks,
                                                               const int *__restrict__ t_ptr, const int32_t *__restrict__ t_dof,
                                                               const int32_t *__restrict__ t_slave, const double *__restrict__ t_val,
                                                               const uint8_t *__restrict__ touched, const double *__restrict__ ly0,
                                                               const double *__restrict__ ly1, const int flags, const double a,
                                                               const uint8_t *__restrict__ mask, const double *x_ess0,
                                                               const double *x_ess1, double *y0, double *y1) {
  if ((int)blockIdx.x < head_blocks) {
    const int i = 2 * ((int)blockIdx.x * kBlock + (int)threadIdx.x);
    if (i + 1 < n_true) {
      double2 v0 = load2<VEC>(ly0, i), v1 = load2<VEC>(ly1, i);
      const bool t0 = touched[i] != 0, t1 = touched[i + 1] != 0;
      if (!t0) {
        v0.x = restrict_value(v0.x, i, flags, a, mask, x_ess0, y0);
        v1.x = restrict_value(v1.x, i, flags, a, mask, x_ess1, y1);
      }
      if (!t1) {
        v0.y = restrict_value(v0.y, i + 1, flags, a, mask, x_ess0, y0);
        v1.y = restrict_value(v1.y, i + 1, flags, a, mask, x_ess1, y1);
      }
      if (VEC && !t0 && !t1) {
        store2<true>(y0, i, v0);
        store2<true>(y1, i, v1);
      } else {
        if (!t0) y0[i] = v0.x, y1[i] = v1.x;
        if (!t1) y0[i + 1] = v0.y, y1[i + 1] = v1.y;
      }
    } else if (i < n_true) {
      if (!touched[i]) {
        y0[i] = restrict_value(ly0[i], i, flags, a, mask, x_ess0, y0);
        y1[i] = restrict_value(ly1[i], i, flags, a, mask, x_ess1, y1);
      }
    }
    return;
  }
  const int lane = (int)threadIdx.x % L;
  const int t = ((int)blockIdx.x - head_blocks) * (kBlock / L) + (int)threadIdx.x / L;
  double s0 = 0.0, s1 = 0.0;
  if (t < n_touched) {
    const int e = t_ptr[t + 1];
    const double *tail0 = ly0 + n_true, *tail1 = ly1 + n_true;
    if (flags & Conforming::ABS) {
      for (int k = t_ptr[t] + lane; k < e; k += L) {
        const double v = fabs(t_val[k]);
        const int sl = t_slave[k];
        s0 += v * tail0[sl];
        s1 += v * tail1[sl];
      }
    } else {
      for (int k = t_ptr[t] + lane; k < e; k += L) {
        const double v = t_val[k];
        const int sl = t_slave[k];
        s0 += v * tail0[sl];
        s1 += v * tail1[sl];
      }
    }
  }
  s0 = group_sum<L>(s0);
  s1 = group_sum<L>(s1);
  if (t < n_touched && lane == 0) {
    const int i = t_dof[t];
    y0[i] = restrict_value(ly0[i] + s0, i, flags, a, mask, x_ess0, y0);
    y1[i] = restrict_value(ly1[i] + s1, i, flags, a, mask, x_ess1, y1);
  }
}

int lanes_for(int longest) {
  int l = 1;
  while (l < longest && l < 32) l *= 2;
  return l;
}

bool aligned16(const void *a, const void *b) { return (((uintptr_t)a | (uintptr_t)b) & 15) == 0; }

// true when [a, a + na) and [b, b + nb) share an element
bool overlap(const double *a, size_t na, const double *b, size_t nb) { return a && b && a < b + nb && b < a + na; }

}  // namespace

Conforming::Conforming(const Context &ctx, int n_true, int n_local, const int *row_ptr, const int32_t *col, const double *val)
    : n_true_(n_true), n_con_(n_local - n_true) {
  PA_REQUIRE(n_true >= 0 && n_local >= n_true, "conforming prolongation: bad sizes");
  PA_REQUIRE(n_local < (1 << 30), "conforming prolongation: too many dofs for the 32-bit index arithmetic of the kernels");
  PA_REQUIRE(n_con_ == 0 || (row_ptr && row_ptr[0] == 0), "conforming prolongation: the row pointer must start at 0");
  const int nnz = n_con_ ? row_ptr[n_con_] : 0;
  PA_REQUIRE(nnz == 0 || (col && val), "conforming prolongation: null arrays");
  int longest = 0;
  std::vector<int> count((size_t)n_true + 1, 0);
  for (int r = 0; r < n_con_; r++) {
    PA_REQUIRE(row_ptr[r + 1] >= row_ptr[r] && row_ptr[r + 1] <= nnz, "conforming prolongation: the row pointer must not decrease");
    longest = std::max(longest, row_ptr[r + 1] - row_ptr[r]);
    for (int k = row_ptr[r]; k < row_ptr[r + 1]; k++) {
      // one-irregular meshes: every column is a true dof (no chains of constraints)
      PA_REQUIRE(col[k] >= 0 && col[k] < n_true, "conforming prolongation: a constraint refers to a dof that is not a true dof");
      count[col[k] + 1]++;
    }
  }
  fwd_lanes_ = lanes_for(longest);
  // C^T as an inverted index over the touched true dofs; rows of C are visited in ascending order, so every list is in
  // ascending slave order
  std::vector<int32_t> t_dof;
  std::vector<int> t_ptr{0}, slot((size_t)n_true, -1);
  std::vector<uint8_t> touched((size_t)n_true, 0);
  int longest_t = 0;
  for (int i = 0; i < n_true; i++) {
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
  if (n_true_ + n_con_ == 0) return;
  const int head = ((n_true_ + 1) / 2 + kBlock - 1) / kBlock;
  const bool vec = aligned16(x, lx);
  auto launch = [&](auto kernel, int lanes) {
    const int rows_per_block = kBlock / lanes;
    const int grid = head + (n_con_ + rows_per_block - 1) / rows_per_block;
    if (grid == 0) return;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, stream, n_true_, n_con_, head, d_row_ptr_, d_col_, d_val_, x, ess_mask, lx);
  };
#define PA_CONFORM_CASE(L)                                                         \
  case L:                                                                          \
    vec ? launch(k_conform_prolongate<L, true>, L) : launch(k_conform_prolongate<L, false>, L); \
    break;
  switch (fwd_lanes_) {
    PA_CONFORM_CASE(1)
    PA_CONFORM_CASE(2)
    PA_CONFORM_CASE(4)
    PA_CONFORM_CASE(8)
    PA_CONFORM_CASE(16)
    PA_CONFORM_CASE(32)
    default: throw pa::Error("conforming prolongation: bad lane count");
  }
#undef PA_CONFORM_CASE
  PA_HIP(hipGetLastError());
}

void Conforming::Restrict(const double *ly, double *y, int flags, double a, const uint8_t *ess_mask, const double *x_ess,
                          hipStream_t stream) const {
  if (n_true_ == 0) return;
  PA_REQUIRE(!((flags & FIX_ONE) && ess_mask) || x_ess, "conforming restriction: FIX_ONE needs the vector the essential rows copy");
  PA_REQUIRE(!((flags & FIX_ONE) && (flags & FIX_ZERO)), "conforming restriction: one policy for the essential rows");
  const int head = ((n_true_ + 1) / 2 + kBlock - 1) / kBlock;
  const bool vec = aligned16(ly, y);
  auto launch = [&](auto kernel, int lanes) {
    const int rows_per_block = kBlock / lanes;
    const int grid = head + (n_touched_ + rows_per_block - 1) / rows_per_block;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, stream, n_true_, n_touched_, head, d_t_ptr_, d_t_dof_, d_t_slave_, d_t_val_,
                       d_touched_, ly, flags, a, ess_mask, x_ess, y);
  };
#define PA_CONFORM_CASE(L)                                                     \
  case L:                                                                      \
    vec ? launch(k_conform_restrict<L, true>, L) : launch(k_conform_restrict<L, false>, L); \
    break;
  switch (tr_lanes_) {
    PA_CONFORM_CASE(1)
    PA_CONFORM_CASE(2)
    PA_CONFORM_CASE(4)
    PA_CONFORM_CASE(8)
    PA_CONFORM_CASE(16)
    PA_CONFORM_CASE(32)
    default: throw pa::Error("conforming restriction: bad lane count");
  }
#undef PA_CONFORM_CASE
  PA_HIP(hipGetLastError());
}

void Conforming::Prolongate2(const double *x0, const double *x1, double *lx0, double *lx1, const uint8_t *ess_mask,
                             hipStream_t stream) const {
  if (n_true_ + n_con_ == 0) return;
  const size_t nt = (size_t)n_true_, nl = nt + n_con_;
  PA_REQUIRE(!overlap(lx0, nl, lx1, nl) && !overlap(lx0, nl, x0, nt) && !overlap(lx0, nl, x1, nt) && !overlap(lx1, nl, x0, nt) &&
                 !overlap(lx1, nl, x1, nt),
             "conforming prolongation of two vectors: the outputs must not overlap each other or the inputs");
  const int head = ((n_true_ + 1) / 2 + kBlock - 1) / kBlock;
  const bool vec = aligned16(x0, lx0) && aligned16(x1, lx1);
  auto launch = [&](auto kernel, int lanes) {
    const int rows_per_block = kBlock / lanes;
    const int grid = head + (n_con_ + rows_per_block - 1) / rows_per_block;
    if (grid == 0) return;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, stream, n_true_, n_con_, head, d_row_ptr_, d_col_, d_val_, x0, x1, ess_mask,
                       lx0, lx1);
  };
#define PA_CONFORM_CASE(L)                                                           \
  case L:                                                                            \
    vec ? launch(k_conform_prolongate2<L, true>, L) : launch(k_conform_prolongate2<L, false>, L); \
    break;
  switch (fwd_lanes_) {
    PA_CONFORM_CASE(1)
    PA_CONFORM_CASE(2)
    PA_CONFORM_CASE(4)
    PA_CONFORM_CASE(8)
    PA_CONFORM_CASE(16)
    PA_CONFORM_CASE(32)
    default: throw pa::Error("conforming prolongation: bad lane count");
  }
#undef PA_CONFORM_CASE
  PA_HIP(hipGetLastError());
}

void Conforming::Restrict2(const double *ly0, const double *ly1, double *y0, double *y1, int flags, double a, const uint8_t *ess_mask,
                           const double *x_ess0, const double *x_ess1, hipStream_t stream) const {
  if (n_true_ == 0) return;
  PA_REQUIRE(!((flags & FIX_ONE) && ess_mask) || (x_ess0 && x_ess1),
             "conforming restriction: FIX_ONE needs the vectors the essential rows copy");
  PA_REQUIRE(!((flags & FIX_ONE) && (flags & FIX_ZERO)), "conforming restriction: one policy for the essential rows");
  const size_t nt = (size_t)n_true_, nl = nt + n_con_;
  PA_REQUIRE(!overlap(y0, nt, y1, nt) && !overlap(y0, nt, ly0, nl) && !overlap(y0, nt, ly1, nl) && !overlap(y1, nt, ly0, nl) &&
                 !overlap(y1, nt, ly1, nl),
             "conforming restriction of two vectors: the outputs must not overlap each other or the inputs");
  const int head = ((n_true_ + 1) / 2 + kBlock - 1) / kBlock;
  const bool vec = aligned16(ly0, y0) && aligned16(ly1, y1);
  auto launch = [&](auto kernel, int lanes) {
    const int rows_per_block = kBlock / lanes;
    const int grid = head + (n_touched_ + rows_per_block - 1) / rows_per_block;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, stream, n_true_, n_touched_, head, d_t_ptr_, d_t_dof_, d_t_slave_, d_t_val_,
                       d_touched_, ly0, ly1, flags, a, ess_mask, x_ess0, x_ess1, y0, y1);
  };
#define PA_CONFORM_CASE(L)                                                       \
  case L:                                                                        \
    vec ? launch(k_conform_restrict2<L, true>, L) : launch(k_conform_restrict2<L, false>, L); \
    break;
  switch (tr_lanes_) {
    PA_CONFORM_CASE(1)
    PA_CONFORM_CASE(2)
    PA_CONFORM_CASE(4)
    PA_CONFORM_CASE(8)
    PA_CONFORM_CASE(16)
    PA_CONFORM_CASE(32)
    default: throw pa::Error("conforming restriction: bad lane count");
  }
#undef PA_CONFORM_CASE
  PA_HIP(hipGetLastError());
}

}  // namespace palace
