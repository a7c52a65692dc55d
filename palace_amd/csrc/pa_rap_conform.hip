// Sparse triple product with conforming prolongations, T = L B P_trial, on the device (linalg.hpp: RapConforming).
//
// The reference's coarsest level is ParOperator::ParallelAssemble (linalg/rap.cpp:84-152): on a mesh with hanging nodes a sparse
// triple product with P = [I; C].  The structure [I; C] keeps it small.  Output row i is
//
//   T[i, :] = sum over l in {i} u slaves(i) of  w_l  sum_k B[l, k] P_trial[k, :],       P_trial[k, :] = e_k  (k < n_true_trial)
//                                                                                                      C_trial[k - n_true_trial, :]
//
// with slaves(i) and w_l the (slave, value) list of i in the inverted index of the test side's Conforming (ascending slaves),
// w_i = 1; the injection form keeps l = i only.  The EXPANDED PRODUCTS of a row, in the order (l: i first, then the slaves
// ascending; position in row l of B; position in the row of C_trial), get the sequence numbers 0, 1, ...; the row of T is that
// list sorted by (column, sequence number), every run of equal columns summed from its first to its last member.  The order
// depends on the inputs alone: no floating-point atomics, bitwise the same result whatever the grid.
//
// Mapping: ONE WAVE (one 64-thread workgroup) PER OUTPUT ROW.  Its lanes expand the row 64 entries of B at a time (a wave scan
// of the entries' expansion counts gives every product its sequence number = its slot), sort the 64-bit keys
// (column << 32 | sequence number) with a bitonic network and compress the runs.  The values are not moved by the sort: they
// stay in expansion order and are read through the sequence number.  Both phases do this; the symbolic one only counts the runs
// (then a scan gives the row pointer, and one host read the total), the numeric one writes columns and values.
//   rows whose products number at most kCapSmall = 256:  keys + values in 4 KiB of LDS per workgroup: with one wave per workgroup
//       the 32 waves of a CU fit (128 of its 160 KiB), so LDS does not limit occupancy; every row of an unconstrained region of a
//       lowest-order space is here (33 entries for H(curl), 27 for H1)
//   at most kCapLarge = 2048:  32 KiB per workgroup, five workgroups per CU; masters of a few slaves at orders 1 and 2
//   longer rows:  the same code on a global workspace sized from the bounds (keys and values, padded to a power of two per row);
//       the masters of a refined face at order >= 2 have 10^4 and more products
// A first pass computes the number of products of every row (exact, not only a bound) and sorts the rows into the three lists.
#include <chrono>

#include "linalg.hpp"

namespace palace {

namespace {

constexpr int kWave = 64;
constexpr int kCapSmall = 256, kCapLarge = 2048;
constexpr unsigned long long kPadKey = ~0ull;

struct RapSide {  // one Conforming as the kernels read it; n_con == 0 and null arrays: the identity
  int n_true, n_con;
  const int *row_ptr;
  const int32_t *col;
  const double *val;
  const int *t_ptr;
  const int32_t *t_slot, *t_slave;
  const double *t_val;
};

struct RapCounters {
  int n_list[3];
  int error;                  // a row with 2^30 products or more
  unsigned long long ws_len;  // entries of the global workspace
};

// products of every row of B: an entry in a true column is one, an entry in a constrained column the length of its row of C
__global__ __launch_bounds__(256) void k_rap_local_count(const int n_rows, const int32_t *__restrict__ b_ptr, const int32_t *__restrict__ b_col,
                                                         const RapSide trial, long long *__restrict__ local_count) {
  const int l = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (l >= n_rows) return;
  long long n = 0;
  for (int a = b_ptr[l]; a < b_ptr[l + 1]; a++) {
    const int k = b_col[a];
    n += (k < trial.n_true) ? 1 : trial.row_ptr[k - trial.n_true + 1] - trial.row_ptr[k - trial.n_true];
  }
  local_count[l] = n;
}

// products of every output row; the rows by class: 0 <= kCapSmall, 1 <= kCapLarge, 2 the rest with their piece of the workspace.
// (The order of a list and the place of a piece depend on the launch; what is computed for a row does not.)
__global__ __launch_bounds__(256) void k_rap_classify(const int n_out, const RapSide test, const bool galerkin, const bool trial_identity,
                                                      const int32_t *__restrict__ b_ptr, const long long *__restrict__ local_count,
                                                      int *__restrict__ bound, int *__restrict__ lists, unsigned long long *__restrict__ ws_off,
                                                      RapCounters *__restrict__ counters) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x), lane = (int)threadIdx.x % 64;
  const bool active = i < n_out;
  auto count = [&](int l) -> long long { return trial_identity ? (long long)(b_ptr[l + 1] - b_ptr[l]) : local_count[l]; };
  long long n = 0;
  if (active) {
    n = count(i);
    if (galerkin && test.n_con && i < test.n_true) {
      const int t = test.t_slot[i];
      if (t >= 0)
        for (int k = test.t_ptr[t]; k < test.t_ptr[t + 1]; k++) n += count(test.n_true + test.t_slave[k]);
    }
    if (n >= (1ll << 30)) {
      atomicOr(&counters->error, 1);
      n = 0;
    }
    bound[i] = (int)n;
  }
  const int cls = n <= kCapSmall ? 0 : (n <= kCapLarge ? 1 : 2);
  // one counter update per wave and class (every row of a level on one address otherwise): the wave's rows of a class take
  // consecutive places in lane order
  for (int c = 0; c < 3; c++) {
    const unsigned long long mine = __ballot(active && cls == c);
    if (!mine) continue;
    const int leader = __ffsll((long long)mine) - 1;
    int first = 0;
    if (lane == leader) first = atomicAdd(&counters->n_list[c], __popcll(mine));
    first = __shfl(first, leader, 64);
    if (active && cls == c) lists[(size_t)c * n_out + first + __popcll(mine & ((1ull << lane) - 1))] = i;
  }
  if (active && cls == 2) {
    unsigned long long pad = 1;
    while (pad < (unsigned long long)n) pad <<= 1;
    ws_off[i] = atomicAdd(&counters->ws_len, pad);
  }
}

template <typename T>
__device__ __forceinline__ T wave_inclusive_scan(T v, const int lane) {
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const T u = __shfl_up(v, o, kWave);
    if (lane >= o) v += u;
  }
  return v;
}

struct RapArgs {
  RapSide test, trial;
  bool galerkin;
  const int32_t *b_ptr, *b_col;
  const double *b_val;
  const int *bound;
  const int *list;  // the rows of this launch
  int n_list;
  const unsigned long long *ws_off;
  unsigned long long *ws_keys;
  double *ws_vals;
  int *count;                // symbolic: entries of every row
  const int32_t *t_ptr_out;  // numeric: the row pointer of T
  int32_t *t_col;
  double *t_val;
};

// CAP > 0: keys (and values) of the row in LDS; CAP == 0: in the global workspace.  One workgroup = one wave = one row, so every
// barrier below is reached by the whole workgroup with the same trip counts.
template <int CAP, bool NUMERIC>
__global__ __launch_bounds__(kWave) void k_rap_row(const RapArgs A) {
  __shared__ unsigned long long s_keys[CAP > 0 ? CAP : 1];
  __shared__ double s_vals[(CAP > 0 && NUMERIC) ? CAP : 1];
  const int lane = (int)threadIdx.x;
  const int row = A.list[blockIdx.x];
  const int n = A.bound[row];
  int npad = 1;
  while (npad < n) npad <<= 1;
  unsigned long long *keys = CAP > 0 ? s_keys : A.ws_keys + A.ws_off[row];
  double *vals = CAP > 0 ? s_vals : (NUMERIC ? A.ws_vals + A.ws_off[row] : nullptr);

  // ---- expansion: the products of the row in their fixed order
  int n_left = 1, t0 = 0;
  if (A.galerkin && A.test.n_con && row < A.test.n_true) {
    const int t = A.test.t_slot[row];
    if (t >= 0) t0 = A.test.t_ptr[t], n_left = 1 + A.test.t_ptr[t + 1] - t0;
  }
  int base = 0;
  for (int li = 0; li < n_left; li++) {
    const int l = li == 0 ? row : A.test.n_true + A.test.t_slave[t0 + li - 1];
    const double w = li == 0 ? 1.0 : A.test.t_val[t0 + li - 1];
    const int end = A.b_ptr[l + 1];
    for (int a0 = A.b_ptr[l]; a0 < end; a0 += kWave) {
      const int a = a0 + lane;
      const bool active = a < end;
      int k = 0, c0 = 0, cnt = 0;
      if (active) {
        k = A.b_col[a];
        cnt = 1;
        if (k >= A.trial.n_true) c0 = A.trial.row_ptr[k - A.trial.n_true], cnt = A.trial.row_ptr[k - A.trial.n_true + 1] - c0;
      }
      const int incl = wave_inclusive_scan(cnt, lane);
      int at = base + incl - cnt;
      base += __shfl(incl, kWave - 1, kWave);
      if (active) {
        const double bv = NUMERIC ? (li == 0 ? A.b_val[a] : w * A.b_val[a]) : 0.0;
        if (k < A.trial.n_true) {
          keys[at] = ((unsigned long long)(unsigned)k << 32) | (unsigned)at;
          if (NUMERIC) vals[at] = bv;
        } else {
          for (int c = c0; c < c0 + cnt; c++, at++) {
            keys[at] = ((unsigned long long)(unsigned)A.trial.col[c] << 32) | (unsigned)at;
            if (NUMERIC) vals[at] = bv * A.trial.val[c];
          }
        }
      }
    }
  }
  for (int p = n + lane; p < npad; p += kWave) keys[p] = kPadKey;
  __syncthreads();

  // ---- bitonic sort of the keys, ascending
  for (int kk = 2; kk <= npad; kk <<= 1)
    for (int j = kk >> 1; j > 0; j >>= 1) {
      for (int t = lane; t < (npad >> 1); t += kWave) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
        const unsigned long long x = keys[lo], y = keys[hi];
        if ((x > y) == ((lo & kk) == 0)) keys[lo] = y, keys[hi] = x;
      }
      __syncthreads();
    }

  // ---- runs of equal columns
  int heads = 0;
  const int32_t out0 = NUMERIC ? A.t_ptr_out[row] : 0;
  for (int p0 = 0; p0 < n; p0 += kWave) {
    const int p = p0 + lane;
    bool head = false;
    unsigned c = 0;
    if (p < n) {
      c = (unsigned)(keys[p] >> 32);
      head = p == 0 || (unsigned)(keys[p - 1] >> 32) != c;
    }
    const int incl = wave_inclusive_scan(head ? 1 : 0, lane);
    if (NUMERIC && head) {
      double s = vals[(unsigned)keys[p]];
      for (int q = p + 1; q < n; q++) {
        const unsigned long long kq = keys[q];
        if ((unsigned)(kq >> 32) != c) break;
        s += vals[(unsigned)kq];
      }
      A.t_col[out0 + heads + incl - 1] = (int32_t)c;
      A.t_val[out0 + heads + incl - 1] = s;
    }
    heads += __shfl(incl, kWave - 1, kWave);
  }
  if (!NUMERIC && lane == 0) A.count[row] = heads;
}

// row pointer from the counts: one workgroup walks the array in tiles (set-up; the counts of a level-0 matrix)
constexpr int kScanBlock = 1024, kScanItems = 8;
__global__ __launch_bounds__(kScanBlock) void k_rap_scan(const int n, const int *__restrict__ count, int32_t *__restrict__ ptr,
                                                        long long *__restrict__ total) {
  __shared__ long long s_wave[kScanBlock / kWave];
  __shared__ long long s_carry;
  const int tid = (int)threadIdx.x, lane = tid % kWave, wave = tid / kWave;
  if (tid == 0) s_carry = 0;
  __syncthreads();
  for (long long i0 = 0; i0 < n; i0 += kScanBlock * kScanItems) {  // every thread kScanItems consecutive rows of the tile
    const long long first = i0 + (long long)tid * kScanItems;
    int c[kScanItems];
    long long v = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; k++) c[k] = first + k < n ? count[first + k] : 0, v += c[k];
    const long long incl = wave_inclusive_scan(v, lane);
    if (lane == kWave - 1) s_wave[wave] = incl;
    __syncthreads();
    long long before = s_carry;
    for (int w = 0; w < wave; w++) before += s_wave[w];
    long long run = before + incl - v;
#pragma unroll
    for (int k = 0; k < kScanItems; k++) {
      if (first + k < n) ptr[first + k] = (int32_t)run;
      run += c[k];
    }
    __syncthreads();
    if (tid == kScanBlock - 1) s_carry = before + incl;
    __syncthreads();
  }
  if (tid == 0) {
    ptr[n] = (int32_t)s_carry;
    *total = s_carry;
  }
}

RapSide side_of(const Conforming *c, int n_identity) {
  if (!c) return {n_identity, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  const Conforming::DeviceView v = c->View();
  return {v.n_true, v.n_con, v.row_ptr, v.col, v.val, v.t_ptr, v.t_slot, v.t_slave, v.t_val};
}

template <bool NUMERIC>
void launch_rows(const RapArgs &base, const int *lists, int n_out, const int n_list[3], hipStream_t s) {
  for (int cls = 0; cls < 3; cls++) {
    if (!n_list[cls]) continue;
    RapArgs a = base;
    a.list = lists + (size_t)cls * n_out, a.n_list = n_list[cls];
    if (cls == 0) hipLaunchKernelGGL((k_rap_row<kCapSmall, NUMERIC>), dim3(a.n_list), dim3(kWave), 0, s, a);
    if (cls == 1) hipLaunchKernelGGL((k_rap_row<kCapLarge, NUMERIC>), dim3(a.n_list), dim3(kWave), 0, s, a);
    if (cls == 2) hipLaunchKernelGGL((k_rap_row<0, NUMERIC>), dim3(a.n_list), dim3(kWave), 0, s, a);
  }
  PA_HIP(hipGetLastError());
}

}  // namespace

std::unique_ptr<pa_csr> RapConforming(const Context &ctx, const pa_csr &B, const Conforming *test, const Conforming *trial,
                                      RapLeft left, double *phase_ms) {
  StreamGraph::RequireNotRecording("the assembled triple product with conforming prolongations");
  PA_REQUIRE(!(test && test->IsDistributed()) && !(trial && trial->IsDistributed()),
             "triple product: a conforming prolongation that carries a halo (several ranks); the assembled P^T A P is built on one rank only");
  hipStream_t s = ctx.stream;
  const int b_rows = B.nrows, b_cols = B.ncols ? B.ncols : B.nrows;
  PA_REQUIRE(!test || test->NumLocal() == b_rows, "triple product: the test side's conforming prolongation does not match the rows of B");
  PA_REQUIRE(!trial || trial->NumLocal() == b_cols, "triple product: the trial side's conforming prolongation does not match the columns of B");
  const bool galerkin = left == RapLeft::GALERKIN;
  const int n_out = test ? test->NumTrue() : b_rows, n_cols = trial ? trial->NumTrue() : b_cols;
  const RapSide st = side_of(test, b_rows), sr = side_of(trial, b_cols);
  const bool trial_identity = !trial || sr.n_con == 0;
  const auto t_start = std::chrono::steady_clock::now();

  auto m = std::make_unique<pa_csr>();
  m->nrows = n_out, m->ncols = n_cols == n_out ? 0 : n_cols;
  m->symmetric = B.symmetric && galerkin && test == trial;
  m->d_rowptr = pa::dev_alloc<int32_t>((size_t)n_out + 1);
  if (n_out == 0) {
    PA_HIP(hipMemsetAsync(m->d_rowptr, 0, sizeof(int32_t), s));
    m->d_col = pa::dev_alloc<int32_t>(0), m->d_val = pa::dev_alloc<double>(0);
    PA_HIP(hipStreamSynchronize(s));
    if (phase_ms) phase_ms[0] = phase_ms[1] = 0.0;
    return m;
  }

  // ---- the products of every row, the three lists
  pa::DevBuf<long long> d_local;
  if (!trial_identity) {
    d_local = pa::dev_alloc<long long>((size_t)b_rows);
    hipLaunchKernelGGL(k_rap_local_count, dim3((b_rows + 255) / 256), dim3(256), 0, s, b_rows, B.d_rowptr.get(), B.d_col.get(), sr, d_local.get());
  }
  const pa::DevBuf<int> d_bound = pa::dev_alloc<int>((size_t)n_out), d_lists = pa::dev_alloc<int>(3 * (size_t)n_out),
                        d_count = pa::dev_alloc<int>((size_t)n_out);
  const pa::DevBuf<unsigned long long> d_ws_off = pa::dev_alloc<unsigned long long>((size_t)n_out);
  const pa::DevBuf<RapCounters> d_counters = pa::dev_alloc<RapCounters>(1);
  const pa::DevBuf<long long> d_total = pa::dev_alloc<long long>(1);
  PA_HIP(hipMemsetAsync(d_counters, 0, sizeof(RapCounters), s));
  hipLaunchKernelGGL(k_rap_classify, dim3((n_out + 255) / 256), dim3(256), 0, s, n_out, st, galerkin, trial_identity, B.d_rowptr.get(),
                     d_local.get(), d_bound.get(), d_lists.get(), d_ws_off.get(), d_counters.get());
  PA_HIP(hipGetLastError());
  RapCounters counters;
  PA_HIP(hipMemcpyAsync(&counters, d_counters, sizeof(RapCounters), hipMemcpyDeviceToHost, s));
  PA_HIP(hipStreamSynchronize(s));
  PA_REQUIRE(!counters.error, "triple product: a row has 2^30 expanded products or more");
  PA_REQUIRE(counters.n_list[0] + counters.n_list[1] + counters.n_list[2] == n_out, "triple product: the row lists are incomplete");
  pa::DevBuf<unsigned long long> d_ws_keys;
  pa::DevBuf<double> d_ws_vals;
  if (counters.ws_len) d_ws_keys = pa::dev_alloc<unsigned long long>((size_t)counters.ws_len);

  // ---- symbolic: entries of every row, the row pointer, the total
  RapArgs a{};
  a.test = st, a.trial = sr, a.galerkin = galerkin;
  a.b_ptr = B.d_rowptr, a.b_col = B.d_col, a.b_val = B.d_val;
  a.bound = d_bound, a.ws_off = d_ws_off, a.ws_keys = d_ws_keys, a.count = d_count;
  launch_rows<false>(a, d_lists, n_out, counters.n_list, s);
  hipLaunchKernelGGL(k_rap_scan, dim3(1), dim3(kScanBlock), 0, s, n_out, d_count.get(), m->d_rowptr.get(), d_total.get());
  PA_HIP(hipGetLastError());
  long long nnz = 0;
  PA_HIP(hipMemcpyAsync(&nnz, d_total, sizeof(long long), hipMemcpyDeviceToHost, s));
  PA_HIP(hipStreamSynchronize(s));
  PA_REQUIRE(nnz < (1ll << 31), "triple product: the result has 2^31 entries or more (int32 row pointers)");
  const auto t_symbolic = std::chrono::steady_clock::now();

  // ---- numeric
  m->nnz = nnz;
  m->d_col = pa::dev_alloc<int32_t>((size_t)nnz), m->d_val = pa::dev_alloc<double>((size_t)nnz);
  if (counters.ws_len) d_ws_vals = pa::dev_alloc<double>((size_t)counters.ws_len);
  a.ws_vals = d_ws_vals, a.t_ptr_out = m->d_rowptr, a.t_col = m->d_col, a.t_val = m->d_val;
  launch_rows<true>(a, d_lists, n_out, counters.n_list, s);
  PA_HIP(hipStreamSynchronize(s));  // (the workspaces go out of scope here)
  if (phase_ms) {
    const auto t_end = std::chrono::steady_clock::now();
    phase_ms[0] = std::chrono::duration<double, std::milli>(t_symbolic - t_start).count();
    phase_ms[1] = std::chrono::duration<double, std::milli>(t_end - t_symbolic).count();
  }
  return m;
}

}  // namespace palace
