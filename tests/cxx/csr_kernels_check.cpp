// Stand-alone check of the assembled-operator kernels (palace_amd/csrc/csr_op.hip: k_csr_spmv, k_csr_spmv_step, k_csr_spmv_split,
// k_csr_eliminate, k_flag, k_csr_diag) through the CsrOperator / ParOperator members, on matrices chosen to stress the kernels rather
// than the ones finite elements produce: every lanes-per-row instantiation (4 / 8 / 16, picked from nnz / nrows with a strict >)
// on rows that are empty, shorter than / equal to / one longer than the lane count, that end inside / at / one past the four
// software-pipelined entries per lane, on row counts around one 256-thread block, on rectangular matrices, on unsorted and on
// duplicate columns, with values of three families (uniform, magnitudes over 10^+-8, rows of cancelling pairs).
//
// Reference: the same operation in long double with plain loops (nothing of amg.hpp but the HostCsr container).  Bound (derived, not
// measured): row i with k_i stored entries may differ from the long double result by (k_i + 8) 2^-53 S_i, S_i = the exact expression
// of that output with every term replaced by its absolute value -- the forward bound of at most k_i + 8 roundings in any summation
// order (fused multiply-add only lowers it).  Selections (eliminated values, diagonals, the transpose of a symmetric matrix,
// repeated runs) are compared bit by bit.
//
// Output: one line per case -- name, rows, lanes, worst error / bound -- then the coverage of each lane count and a summary; the exit
// status is non-zero if any ratio exceeds 1, any exact comparison differs, or a guard zone around an output buffer was written.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <string>
#include <vector>

#include "amg_solver.hpp"

using namespace palace;
using amg::HostCsr;

#if !defined(__HIP_DEVICE_COMPILE__)  // (the device pass of the compiler has its own long double; nothing here runs there)
static_assert(LDBL_MANT_DIG >= 64, "the reference needs an extended-precision long double");
#endif

namespace {

constexpr long double kU = 0x1p-53L;
constexpr double kGuard = -1.2345678e123;
constexpr int kPad = 32;
const double kNaN = std::numeric_limits<double>::quiet_NaN();
const long double kInf = std::numeric_limits<long double>::infinity();

#define CK(expr)                                                                                     \
  do {                                                                                               \
    hipError_t e__ = (expr);                                                                         \
    if (e__ != hipSuccess) {                                                                         \
      std::fprintf(stderr, "%s failed: %s (line %d)\n", #expr, hipGetErrorString(e__), __LINE__);   \
      std::exit(3);                                                                                  \
    }                                                                                                \
  } while (0)

// ---- counter-based generator ----------------------------------------------------------------------------------------------------
uint64_t mix64(uint64_t z) {
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
struct Rng {
  uint64_t key, ctr = 0;
  explicit Rng(uint64_t seed) : key(mix64(seed)) {}
  uint64_t bits() { return mix64(key ^ (0xd1342543de82ef95ull * ++ctr)); }
  double uni() { return ((double)(bits() >> 12) + 0.5) * 0x1p-51 - 1.0; }  // (-1, 1), never 0
  int below(int n) { return (int)(bits() % (uint64_t)n); }
};
std::vector<double> uniform(int n, uint64_t seed) {
  Rng r(seed);
  std::vector<double> v((size_t)n);
  for (double &e : v) e = r.uni();
  return v;
}

// ---- device buffers with guard zones ----------------------------------------------------------------------------------------------
hipStream_t g_stream;
Context g_ctx;
bool g_guards_ok = true;

class Buf {
  double *d_ = nullptr;
  int n_;

public:
  explicit Buf(int n) : n_(n) { CK(hipMalloc(reinterpret_cast<void **>(&d_), sizeof(double) * (size_t)(n + 2 * kPad))); }
  Buf(const Buf &) = delete;
  Buf &operator=(const Buf &) = delete;
  ~Buf() { (void)hipFree(d_); }
  double *p() const { return d_ + kPad; }
  void set(const std::vector<double> &h) const {
    std::vector<double> all((size_t)(n_ + 2 * kPad), kGuard);
    std::copy(h.begin(), h.begin() + n_, all.begin() + kPad);
    CK(hipMemcpy(d_, all.data(), sizeof(double) * all.size(), hipMemcpyHostToDevice));
  }
  void fill(double v) const { set(std::vector<double>((size_t)n_, v)); }
  std::vector<double> get() const {
    CK(hipStreamSynchronize(g_stream));
    std::vector<double> all((size_t)(n_ + 2 * kPad));
    CK(hipMemcpy(all.data(), d_, sizeof(double) * all.size(), hipMemcpyDeviceToHost));
    for (int i = 0; i < kPad; i++)
      if (all[(size_t)i] != kGuard || all[(size_t)(kPad + n_ + i)] != kGuard) g_guards_ok = false;
    return std::vector<double>(all.begin() + kPad, all.begin() + kPad + n_);
  }
};

bool same_bits(const std::vector<double> &a, const std::vector<double> &b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), sizeof(double) * a.size()) == 0);
}

// ---- matrices ---------------------------------------------------------------------------------------------------------------------
enum Family { UNIFORM, SPREAD, CANCEL };
enum Columns { SORTED, UNSORTED, DUPLICATES };
const char *kFamily[] = {"uniform", "spread", "cancel"};

struct Mat {
  std::string name;
  HostCsr h;
  std::vector<double> val2;  // a second value array on the same pattern
  int lpr = 0;               // the instantiation this matrix is meant for
  bool all_diag = false;     // every row stores its diagonal entry
};

int expected_lanes(const HostCsr &h) {  // strict >: 12 n entries are 4 lanes, 12 n + 1 are 8
  const long long nnz = h.nnz(), n = h.nrows;
  return nnz > 24 * n ? 16 : (nnz > 12 * n ? 8 : 4);
}

Mat build(const std::string &name, int lpr, const std::vector<int> &lens, int ncols, Family fam, Columns cm, bool force_diag,
          uint64_t seed) {
  Mat M;
  M.name = name, M.lpr = lpr;
  HostCsr &h = M.h;
  h.nrows = (int)lens.size(), h.ncols = ncols;
  h.rowptr.assign(1, 0);
  Rng r(seed);
  std::vector<int> perm((size_t)ncols), cols;
  for (int c = 0; c < ncols; c++) perm[(size_t)c] = c;
  M.all_diag = force_diag;
  for (int i = 0; i < h.nrows; i++) {
    const int k = lens[(size_t)i];
    cols.clear();
    if (cm == DUPLICATES || k > ncols) {  // with replacement (a row longer than the matrix is wide cannot do without)
      for (int j = 0; j < k; j++) cols.push_back(r.below(ncols));
      if (cm == DUPLICATES && k >= 2) cols[1] = cols[0];
    } else {  // k distinct columns: the head of a running shuffle
      for (int j = 0; j < k; j++) std::swap(perm[(size_t)j], perm[(size_t)(j + r.below(ncols - j))]);
      cols.assign(perm.begin(), perm.begin() + k);
    }
    if (force_diag) {
      if (k == 0 || i >= ncols) M.all_diag = false;
      else {
        if (std::find(cols.begin(), cols.end(), i) == cols.end()) cols[0] = i;
        if (cm == DUPLICATES && k >= 2) cols[0] = cols[1] = i;  // the diagonal entry itself stored twice
      }
    }
    if (cm != UNSORTED) std::sort(cols.begin(), cols.end());
    else if (k >= 2 && std::is_sorted(cols.begin(), cols.end())) std::swap(cols[0], cols[(size_t)k - 1]);
    for (int j = 0; j < k; j++) {
      double v = r.uni();
      if (fam == SPREAD) v = (v < 0 ? -1.0 : 1.0) * std::pow(10.0, 8.0 * r.uni());
      if (fam == CANCEL && (j & 1)) v = -h.val.back();  // pairs v, -v on two columns
      h.col.push_back(cols[(size_t)j]), h.val.push_back(v);
    }
    h.rowptr.push_back((int)h.col.size());
  }
  M.val2 = uniform((int)h.nnz(), seed ^ 0x5555);
  return M;
}

// row lengths of the ragged matrices: the cycle {0, 1, L-1, L, L+1, 4L-1, 4L, 4L+1, 9L+3}; rows from the end are replaced by short (1)
// or long (5L+2) filler rows until nnz / nrows lies in the class of L lanes
std::vector<int> ragged_lengths(int L, int n) {
  const int cyc[9] = {0, 1, L - 1, L, L + 1, 4 * L - 1, 4 * L, 4 * L + 1, 9 * L + 3};
  std::vector<int> lens((size_t)n);
  for (int i = 0; i < n; i++) lens[(size_t)i] = cyc[i % 9];
  const long long lo = L == 4 ? -1 : (L == 8 ? 12 : 24), hi = L == 4 ? 12 : (L == 8 ? 24 : (1 << 20));
  for (int i = n - 1; i >= 9; i--) {
    long long nnz = 0;
    for (int k : lens) nnz += k;
    if (nnz > hi * n) lens[(size_t)i] = 1;
    else if (nnz <= lo * n) lens[(size_t)i] = 5 * L + 2;
    else break;
  }
  return lens;
}

// ---- reference --------------------------------------------------------------------------------------------------------------------
struct Ref {
  std::vector<long double> v, S;
  std::vector<int> k;
  void push(long double val, long double s, int kk) { v.push_back(val), S.push_back(s), k.push_back(kk); }
};
struct Dot {
  std::vector<long double> s, sa;  // sum_j a_ij x_j, sum_j |a_ij| |x_j|
  std::vector<int> k;
};
Dot rowdot(const HostCsr &h, const std::vector<double> &val, const std::vector<double> &x) {
  Dot d;
  for (int i = 0; i < h.nrows; i++) {
    long double s = 0.0L, sa = 0.0L;
    for (int a = h.rowptr[(size_t)i]; a < h.rowptr[(size_t)i + 1]; a++) {
      const long double t = (long double)val[(size_t)a] * (long double)x[(size_t)h.col[(size_t)a]];
      s += t, sa += fabsl(t);
    }
    d.s.push_back(s), d.sa.push_back(sa), d.k.push_back(h.rowptr[(size_t)i + 1] - h.rowptr[(size_t)i]);
  }
  return d;
}
long double worst_ratio(const std::vector<double> &out, const Ref &r) {
  if (out.size() != r.v.size()) return kInf;
  long double w = 0.0L;
  for (size_t i = 0; i < out.size(); i++) {
    if (!(out[i] == out[i])) return kInf;  // a sentinel that survived, or one that was added to
    const long double err = fabsl((long double)out[i] - r.v[i]), bound = (long double)(r.k[i] + 8) * kU * r.S[i];
    if (err == 0.0L) continue;
    if (!(bound > 0.0L)) return kInf;
    w = std::max(w, err / bound);
  }
  return w;
}

// ---- reporting --------------------------------------------------------------------------------------------------------------------
int g_cases = 0, g_failed = 0;
long double g_worst = 0.0L;
void emit(const std::string &name, const char *op, int rows, int lanes, long double ratio, bool exact_ok) {
  const bool ok = exact_ok && ratio <= 1.0L;
  g_cases++, g_failed += ok ? 0 : 1;
  if (ratio == ratio && ratio != kInf) g_worst = std::max(g_worst, ratio);
  std::printf("case %s:%s rows %d lanes %d ratio %.3Le %s\n", name.c_str(), op, rows, lanes, ratio, ok ? "OK" : "FAIL");
}
// runs `f` twice from the same state: the second result must have the bits of the first
template <typename F>
std::vector<double> twice(F &&f, bool &repro) {
  std::vector<double> a = f(), b = f();
  if (!same_bits(a, b)) repro = false;
  return a;
}
template <typename F>
bool throws(F &&f) {
  try {
    f();
  } catch (const pa::Error &) {
    return true;
  }
  return false;
}

std::vector<double> cat(const std::vector<double> &a, const std::vector<double> &b) {
  std::vector<double> c(a);
  c.insert(c.end(), b.begin(), b.end());
  return c;
}

// ---- the operations on one matrix ---------------------------------------------------------------------------------------------------
void check_matrix(const Mat &M, int cover[3][4]) {
  const HostCsr &h = M.h;
  const int nr = h.nrows, nc = h.ncols;
  const bool square = nr == nc;
  DeviceCsr D(g_ctx, h, true), Dns(g_ctx, h, false);
  const CsrOperator &A = D.Op();
  const int lanes = A.Lanes();
  const std::string &nm = M.name;
  // the instantiation: what the rule gives for this nnz / nrows, and (where the matrix was built for one) the intended one
  emit(nm, "lanes", nr, lanes, 0.0L, lanes == expected_lanes(h) && (M.lpr == 0 || lanes == M.lpr));
  if (M.lpr && lanes == M.lpr && nm.find("ragged") != std::string::npos) {
    const int li = lanes == 4 ? 0 : (lanes == 8 ? 1 : 2);
    bool empty = false, l41 = false;
    for (int i = 0; i < nr; i++) {
      const int k = h.rowptr[(size_t)i + 1] - h.rowptr[(size_t)i];
      empty = empty || k == 0, l41 = l41 || k == 4 * lanes + 1;
    }
    if (empty) cover[li][0] = 1;
    if (l41) cover[li][1] = 1;
    if (nr == 256 / lanes - 1 && empty && l41) cover[li][2] = 1;
    if (nr == 256 / lanes + 1 && empty && l41) cover[li][3] = 1;
  }

  const std::vector<double> x = uniform(nc, 11), y0 = uniform(nr, 12), r0 = uniform(nr, 13), dinv = uniform(nr, 14),
                            ep = uniform(nr, 15);
  Buf bx(nc), by(nr), bz(nr), br0(nr), bdinv(nr), bep(nr), bval2((int)h.nnz());
  bx.set(x), br0.set(r0), bdinv.set(dinv), bval2.set(M.val2);
  Vector vx(bx.p(), nc), vy(by.p(), nr), vz(bz.p(), nr), vr0(br0.p(), nr), vdinv(bdinv.p(), nr), vep(bep.p(), nr);
  const Dot d1 = rowdot(h, h.val, x), d2 = rowdot(h, M.val2, x);
  bool repro = true;

  // Mult, MultValues, AddMult
  std::vector<double> y_mult;
  for (int two = 0; two < 2; two++) {
    const Dot &d = two ? d2 : d1;
    const std::vector<double> out = twice(
        [&] {
          by.fill(kNaN);
          if (two) A.MultValues(bval2.p(), vx, vy);
          else A.Mult(vx, vy);
          return by.get();
        },
        repro);
    if (!two) y_mult = out;
    Ref r;
    for (int i = 0; i < nr; i++) r.push(d.s[(size_t)i], d.sa[(size_t)i], d.k[(size_t)i]);
    emit(nm, two ? "multvalues" : "mult", nr, lanes, worst_ratio(out, r), true);
  }
  for (const double a : {1.0, -0.7}) {
    const std::vector<double> out = twice(
        [&] {
          by.set(y0);
          A.AddMult(vx, vy, a);
          return by.get();
        },
        repro);
    Ref r;
    for (int i = 0; i < nr; i++)
      r.push((long double)y0[(size_t)i] + (long double)a * d1.s[(size_t)i], fabsl(y0[(size_t)i]) + fabsl(a) * d1.sa[(size_t)i],
             d1.k[(size_t)i]);
    emit(nm, a == 1.0 ? "addmult_1" : "addmult_m0.7", nr, lanes, worst_ratio(out, r), true);
  }
  // MultTranspose: the bits of Mult on a matrix flagged symmetric, refused on one that is not
  {
    bool ok = throws([&] { Dns.Op().MultTranspose(vx, vy); });
    if (square) {
      by.fill(kNaN);
      A.MultTranspose(vx, vy);
      ok = ok && same_bits(by.get(), y_mult);
    }
    emit(nm, "transpose", nr, lanes, 0.0L, ok);
  }
  // AssembleDiagonal: duplicates summed in storage order, 0 where no diagonal entry is stored -- exact
  {
    std::vector<double> dref((size_t)nr, 0.0);
    for (int i = 0; i < nr; i++) {
      double s = 0.0;
      for (int a = h.rowptr[(size_t)i]; a < h.rowptr[(size_t)i + 1]; a++)
        if (h.col[(size_t)a] == i) s += h.val[(size_t)a];
      dref[(size_t)i] = s;
    }
    const std::vector<double> out = twice(
        [&] {
          by.fill(kNaN);
          A.AssembleDiagonal(vy);
          return by.get();
        },
        repro);
    emit(nm, "diag", nr, lanes, 0.0L, same_bits(out, dref));
  }
  // PrepareChebyStep: square matrices, unless switched off
  {
    unsetenv("PALACE_AMD_FUSED_STEP_CSR");
    bool ok = A.PrepareChebyStep() == square;
    setenv("PALACE_AMD_FUSED_STEP_CSR", "0", 1);
    ok = ok && !A.PrepareChebyStep();
    unsetenv("PALACE_AMD_FUSED_STEP_CSR");
    emit(nm, "prepare", nr, lanes, 0.0L, ok);
  }
  if (!square) {
    emit(nm, "repro", nr, lanes, 0.0L, repro);
    return;
  }
  const int n = nr;

  // EliminatedValues: a selection, compared bit by bit (matrices that store every diagonal entry)
  if (M.all_diag && h.nnz() > 0) {
    bool ok = true;
    for (int which = 0; which < 3; which++) {
      std::vector<int32_t> ess;
      Rng r(77);
      for (int i = 0; i < n; i++)
        if (which == 2 || (which == 1 && r.below(3) == 0)) ess.push_back(i);
      std::vector<char> flag((size_t)n, 0);
      for (int32_t e : ess) flag[(size_t)e] = 1;
      int32_t *d_ess = nullptr;
      CK(hipMalloc(reinterpret_cast<void **>(&d_ess), sizeof(int32_t) * std::max<size_t>(ess.size(), 1)));
      if (!ess.empty()) CK(hipMemcpy(d_ess, ess.data(), sizeof(int32_t) * ess.size(), hipMemcpyHostToDevice));
      for (int one = 0; one < 2; one++) {
        std::vector<double> want(h.val);
        for (int i = 0; i < n; i++)
          for (int a = h.rowptr[(size_t)i]; a < h.rowptr[(size_t)i + 1]; a++) {
            const int c = h.col[(size_t)a];
            if (flag[(size_t)i] || flag[(size_t)c]) want[(size_t)a] = (flag[(size_t)i] && c == i) ? (one ? 1.0 : 0.0) : 0.0;
          }
        for (int rep = 0; rep < 2; rep++) {
          double *dv = A.EliminatedValues(d_ess, (int)ess.size(), one != 0);
          std::vector<double> got((size_t)h.nnz());
          CK(hipMemcpy(got.data(), dv, sizeof(double) * got.size(), hipMemcpyDeviceToHost));
          CK(hipFree(dv));
          ok = ok && same_bits(got, want);
        }
      }
      CK(hipFree(d_ess));
    }
    emit(nm, "eliminate", n, lanes, 0.0L, ok);
  }

  // MultResidual: res = r0 - A x and / or d0 = c0 dinv .* (r0 - A x)
  {
    const double c0 = 4.0 / 3.0;
    long double w = 0.0L;
    for (int cs = 0; cs < 4; cs++) {  // res only, d0 only, both, both with the second values
      const bool has_res = cs != 1, has_d0 = cs != 0, two = cs == 3;
      const Dot &d = two ? d2 : d1;
      const std::vector<double> out = twice(
          [&] {
            by.fill(kNaN), bz.fill(kNaN);
            if (two) A.MultResidualValues(bval2.p(), vx, vr0, has_res ? &vy : nullptr, has_d0 ? &vdinv : nullptr, c0, has_d0 ? &vz : nullptr);
            else A.MultResidual(vx, vr0, has_res ? &vy : nullptr, has_d0 ? &vdinv : nullptr, c0, has_d0 ? &vz : nullptr);
            return cat(by.get(), bz.get());
          },
          repro);
      Ref rr, rd;
      for (int i = 0; i < n; i++) {
        const long double rv = (long double)r0[(size_t)i] - d.s[(size_t)i], ra = fabsl(r0[(size_t)i]) + d.sa[(size_t)i];
        const long double cd = (long double)c0 * (long double)dinv[(size_t)i];
        rr.push(rv, ra, d.k[(size_t)i]), rd.push(cd * rv, fabsl(cd) * ra, d.k[(size_t)i]);
      }
      const std::vector<double> o_res(out.begin(), out.begin() + n), o_d0(out.begin() + n, out.end());
      if (has_res) w = std::max(w, worst_ratio(o_res, rr));
      else if (std::any_of(o_res.begin(), o_res.end(), [](double v) { return v == v; })) w = kInf;  // not asked for: untouched
      if (has_d0) w = std::max(w, worst_ratio(o_d0, rd));
      else if (std::any_of(o_d0.begin(), o_d0.end(), [](double v) { return v == v; })) w = kInf;
    }
    emit(nm, "residual", n, lanes, w, true);
  }

  // MultChebyStep: out (+)= e + sd (e - e_prev) + sr dinv .* (r0 - A e), e = x
  {
    const double sd = 3.0 / 7.0, sr = 20.0 / 7.0;
    long double w = 0.0L;
    // e_prev null | given; add; out = the buffer of e_prev; the last one with the second values
    const struct { bool prev, add, alias, two; } cases[] = {{false, false, false, false}, {false, true, false, false}, {true, false, false, false},
                                                            {true, true, false, false},   {true, false, true, false},  {true, true, false, true}};
    for (const auto &cs : cases) {
      const Dot &d = cs.two ? d2 : d1;
      const std::vector<double> out = twice(
          [&] {
            bep.set(ep);
            if (cs.add) by.set(y0);
            else by.fill(kNaN);
            Vector &vo = cs.alias ? vep : vy;
            const Operator::ChebyStepArgs args{sd, sr, &vdinv, &vr0, cs.prev ? &vep : nullptr, &vo, cs.add};
            if (cs.two) A.MultChebyStepValues(bval2.p(), vx, args);
            else A.MultChebyStep(vx, args);
            return cs.alias ? bep.get() : by.get();
          },
          repro);
      Ref r;
      for (int i = 0; i < n; i++) {
        const long double e = x[(size_t)i], p = cs.prev ? (long double)ep[(size_t)i] : 0.0L, o = cs.add ? (long double)y0[(size_t)i] : 0.0L;
        const long double cd = (long double)sr * (long double)dinv[(size_t)i];
        const long double val = o + e + (long double)sd * (e - p) + cd * ((long double)r0[(size_t)i] - d.s[(size_t)i]);
        const long double S = fabsl(o) + fabsl(e) + fabsl((long double)sd) * (fabsl(e) + fabsl(p)) +
                              fabsl(cd) * (fabsl(r0[(size_t)i]) + d.sa[(size_t)i]);
        r.push(val, S, d.k[(size_t)i]);
      }
      w = std::max(w, worst_ratio(out, r));
    }
    emit(nm, "step", n, lanes, w, true);
    // the result aliasing the vector the matrix multiplies: refused on the host, nothing launched, nothing written
    bx.set(x);
    const Operator::ChebyStepArgs bad{sd, sr, &vdinv, &vr0, nullptr, &vx, false};
    bool ok = throws([&] { A.MultChebyStep(vx, bad); }) && throws([&] { A.MultChebyStepValues(bval2.p(), vx, bad); });
    ok = ok && throws([&] { A.MultResidual(vx, vr0, &vx); });
    ok = ok && same_bits(bx.get(), x);
    emit(nm, "step_alias_refused", n, lanes, 0.0L, ok);
  }

  // MultSplit: rows / columns [0, n_true) in x / y, the rest in the ghost buffers; the plain product on the concatenated vectors
  {
    long double w = 0.0L;
    unsigned long long *d_sel = nullptr;
    CK(hipMalloc(reinterpret_cast<void **>(&d_sel), sizeof(unsigned long long)));
    std::vector<int> splits = {0, std::min(n, (n / 2) | 1), n};
    splits.erase(std::unique(splits.begin(), splits.end()), splits.end());
    for (const int nt : splits) {
      const int ng = n - nt;
      Buf sx(nt), sg(ng), sbad(ng), sy(nt), syg(ng);
      sx.set(std::vector<double>(x.begin(), x.begin() + nt)), sg.set(std::vector<double>(x.begin() + nt, x.end())), sbad.fill(kNaN);
      // sel null | 6 | 7 with a second ghost buffer (the other one poisoned), 7 without one (both parities read xg0)
      for (int v = 0; v < 4; v++) {
        const unsigned long long sel = v == 1 ? 6ull : 7ull;
        CK(hipMemcpy(d_sel, &sel, sizeof(sel), hipMemcpyHostToDevice));
        const double *g0 = v == 2 ? sbad.p() : sg.p(), *g1 = v == 3 ? nullptr : (v == 2 ? sg.p() : sbad.p());
        const bool two = v == 1 || v == 3;
        const Dot &d = two ? d2 : d1;
        const std::vector<double> out = twice(
            [&] {
              sy.fill(kNaN), syg.fill(kNaN);
              A.MultSplit(two ? bval2.p() : nullptr, sx.p(), g0, g1, v == 0 ? nullptr : d_sel, sy.p(), syg.p(), nt);
              return cat(sy.get(), syg.get());
            },
            repro);
        Ref r;
        for (int i = 0; i < n; i++) r.push(d.s[(size_t)i], d.sa[(size_t)i], d.k[(size_t)i]);
        w = std::max(w, worst_ratio(out, r));
      }
    }
    CK(hipFree(d_sel));
    emit(nm, "split", n, lanes, w, true);
  }
  emit(nm, "repro", n, lanes, 0.0L, repro);
}

// ---- ParOperator over a CsrOperator: one rank, symmetric positive definite, both diagonal policies, against dense elimination -----
void check_par_operator(int L) {
  const int n = 301, per_row = L == 4 ? 4 : (L == 8 ? 9 : 17);  // off-diagonal pairs started per row: about 2 per_row + 1 entries
  Rng r(900 + (uint64_t)L);
  std::vector<long double> dense((size_t)n * n, 0.0L);
  std::vector<double> dd((size_t)n * n, 0.0);
  for (int i = 0; i < n; i++)
    for (int t = 0; t < per_row; t++) {
      const int j = r.below(n);
      if (j == i || dd[(size_t)i * n + j] != 0.0) continue;
      dd[(size_t)i * n + j] = dd[(size_t)j * n + i] = r.uni();
    }
  for (int i = 0; i < n; i++) {
    double s = 1.0;
    for (int j = 0; j < n; j++) s += std::abs(dd[(size_t)i * n + j]);
    dd[(size_t)i * n + i] = s;  // strictly diagonally dominant with a positive diagonal: positive definite
  }
  HostCsr h;
  h.nrows = h.ncols = n;
  h.rowptr.assign(1, 0);
  for (int i = 0; i < n; i++) {
    for (int j = 0; j < n; j++)
      if (dd[(size_t)i * n + j] != 0.0) h.col.push_back(j), h.val.push_back(dd[(size_t)i * n + j]);
    h.rowptr.push_back((int)h.col.size());
  }
  DeviceCsr D(g_ctx, h, true);
  const int lanes = D.Op().Lanes();
  const std::string nm = "par/L" + std::to_string(L);
  emit(nm, "lanes", n, lanes, 0.0L, lanes == L && lanes == expected_lanes(h));
  std::vector<int32_t> ess;
  std::vector<char> flag((size_t)n, 0);
  for (int i = 0; i < n; i++)
    if (r.below(3) == 0) ess.push_back(i), flag[(size_t)i] = 1;
  const std::vector<double> x = uniform(n, 21), y0 = uniform(n, 22);
  Buf bx(n), by(n);
  Vector vx(bx.p(), n), vy(by.p(), n);
  for (int one = 0; one < 2; one++) {
    const std::string pn = nm + (one ? "/diag_one" : "/diag_zero");
    for (int i = 0; i < n; i++)
      for (int j = 0; j < n; j++)
        dense[(size_t)i * n + j] = (flag[(size_t)i] || flag[(size_t)j]) ? ((i == j && one) ? 1.0L : 0.0L) : (long double)dd[(size_t)i * n + j];
    std::vector<long double> s((size_t)n, 0.0L), sa((size_t)n, 0.0L);
    for (int i = 0; i < n; i++)
      for (int j = 0; j < n; j++) {
        const long double t = dense[(size_t)i * n + j] * (long double)x[(size_t)j];
        s[(size_t)i] += t, sa[(size_t)i] += fabsl(t);
      }
    ParOperator P(g_ctx, D.Op(), n, ess.data(), (int)ess.size(), one ? ParOperator::DiagonalPolicy::DIAG_ONE : ParOperator::DiagonalPolicy::DIAG_ZERO);
    bool repro = true;
    Ref rm, ra;
    const long double a = (long double)(-0.7);  // (the double the library receives)
    for (int i = 0; i < n; i++) {
      const int k = h.rowptr[(size_t)i + 1] - h.rowptr[(size_t)i];
      rm.push(s[(size_t)i], sa[(size_t)i], k);
      ra.push((long double)y0[(size_t)i] + a * s[(size_t)i], fabsl(y0[(size_t)i]) + fabsl(a) * sa[(size_t)i], k);
    }
    const std::vector<double> o1 = twice(
        [&] {
          bx.set(x), by.fill(kNaN);
          P.Mult(vx, vy);  // x != y: the eliminated values
          return by.get();
        },
        repro);
    emit(pn, "par_mult", n, lanes, worst_ratio(o1, rm), true);
    const std::vector<double> o2 = twice(
        [&] {
          bx.set(x);
          P.Mult(vx, vx);  // in place: the generic path
          return bx.get();
        },
        repro);
    emit(pn, "par_mult_inplace", n, lanes, worst_ratio(o2, rm), true);
    const std::vector<double> o3 = twice(
        [&] {
          bx.set(x), by.set(y0);
          P.AddMult(vx, vy, -0.7);
          return by.get();
        },
        repro);
    emit(pn, "par_addmult", n, lanes, worst_ratio(o3, ra), true);
    const std::vector<double> o4 = twice(
        [&] {
          by.fill(kNaN);
          P.AssembleDiagonal(vy);
          return by.get();
        },
        repro);
    std::vector<double> dref((size_t)n);
    for (int i = 0; i < n; i++) dref[(size_t)i] = (double)dense[(size_t)i * n + i];
    emit(pn, "par_diag", n, lanes, 0.0L, same_bits(o4, dref));
    emit(pn, "repro", n, lanes, 0.0L, repro && P.PrepareChebyStep());
  }
}

}  // namespace

int main() {
  int cover[3][4] = {};
  try {
    if (hipStreamCreate(&g_stream) != hipSuccess) {
      std::fprintf(stderr, "no HIP device\n");
      return 2;
    }
    g_ctx.stream = g_stream;
    std::vector<Mat> mats;
    uint64_t seed = 1;
    for (const int L : {4, 8, 16}) {
      const std::string t = "/L" + std::to_string(L);
      // ragged: n around one 256-thread block, one row, many blocks; the large one in the three value families
      for (const int n : {256 / L - 1, 256 / L, 256 / L + 1, 1003}) {
        const std::string nn = "/n" + std::to_string(n);
        for (const Family f : {UNIFORM, SPREAD, CANCEL})
          if (f == UNIFORM || n == 1003 || n == 256 / L + 1)
            mats.push_back(build("ragged" + t + nn + "/" + kFamily[f], L, ragged_lengths(L, n), n, f, SORTED, false, seed++));
      }
      // one row of 4L + 1 entries (its nnz / nrows puts it in the class above for L = 4, 8: the lanes line reports what ran), and one
      // row of the longest length that stays in the class
      mats.push_back(build("onerow" + t + "/len" + std::to_string(4 * L + 1), 0, {4 * L + 1}, 1, UNIFORM, SORTED, false, seed++));
      mats.push_back(build("onerow_wide" + t + "/len" + std::to_string(4 * L + 1), 0, {4 * L + 1}, 97, UNIFORM, SORTED, false, seed++));
      const int fit = L == 4 ? 12 : (L == 8 ? 24 : 9 * L + 3);
      mats.push_back(build("onerow" + t + "/len" + std::to_string(fit), L, {fit}, 1, UNIFORM, SORTED, false, seed++));
      // rectangular, both ways
      mats.push_back(build("rect" + t + "/1003x517", L, ragged_lengths(L, 1003), 517, UNIFORM, SORTED, false, seed++));
      mats.push_back(build("rect" + t + "/517x1003", L, ragged_lengths(L, 517), 1003, UNIFORM, SORTED, false, seed++));
      // columns unsorted inside the rows; duplicate (row, column) entries
      mats.push_back(build("unsorted" + t + "/n203", L, ragged_lengths(L, 203), 203, UNIFORM, UNSORTED, false, seed++));
      mats.push_back(build("duplicates" + t + "/n203", L, ragged_lengths(L, 203), 203, UNIFORM, DUPLICATES, false, seed++));
      // every diagonal entry stored (no empty rows: the cycle from its second entry on): elimination
      {
        std::vector<int> lens = ragged_lengths(L, 1003);
        for (int &k : lens) k = std::max(k, 1);
        mats.push_back(build("alldiag" + t + "/n1003", L, lens, 1003, UNIFORM, SORTED, true, seed++));
        std::vector<int> few(lens.begin(), lens.begin() + 257);
        mats.push_back(build("alldiag_dups" + t + "/n257", L, few, 257, SPREAD, DUPLICATES, true, seed++));
      }
    }
    // the thresholds (strict >): 12 n -> 4 lanes, 12 n + 1 -> 8, 24 n -> 8, 24 n + 1 -> 16
    {
      const int n = 67;
      const struct { int per, extra, lanes; } th[] = {{12, 0, 4}, {12, 1, 8}, {24, 0, 8}, {24, 1, 16}};
      for (const auto &t : th) {
        std::vector<int> lens((size_t)n, t.per);
        lens[(size_t)n / 2] += t.extra;
        mats.push_back(build("threshold/" + std::to_string(t.per) + "n+" + std::to_string(t.extra), t.lanes, lens, n, UNIFORM, SORTED, false, seed++));
      }
    }
    for (const Mat &M : mats) check_matrix(M, cover);
    for (const int L : {4, 8, 16}) check_par_operator(L);
    CK(hipStreamSynchronize(g_stream));
  } catch (const std::exception &e) {
    std::printf("exception: %s\n", e.what());
    return 4;
  }
  bool covered = true;
  for (int li = 0; li < 3; li++) {
    std::printf("coverage lanes %d empty_row %d row_4lpr_plus_1 %d n_block_minus_1 %d n_block_plus_1 %d\n", 4 << li, cover[li][0], cover[li][1],
                cover[li][2], cover[li][3]);
    for (int q = 0; q < 4; q++) covered = covered && cover[li][q];
  }
  std::printf("summary cases %d failed %d guards %s coverage %s worst %.3Le\n", g_cases, g_failed, g_guards_ok ? "intact" : "WRITTEN",
              covered ? "complete" : "INCOMPLETE", g_worst);
  return (g_failed == 0 && g_guards_ok && covered) ? 0 : 1;
}
