// TimeOperator (timeoperator.hpp): the generalized-alpha step of the transient driver and its element-wise kernels.
#include "timeoperator.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

namespace palace {

namespace {

constexpr int kBlock = 256;
constexpr int kMaxBlocks = 2048;  // memory-bound passes: a capped grid, the rest strided

inline int grid_for(long long work) {
  const long long b = (work + kBlock - 1) / kBlock;
  return (int)std::max(1LL, std::min<long long>(b, kMaxBlocks));
}

// Two consecutive doubles of an array whose base is 16-byte aligned (one 16-byte access) or only 8-byte aligned (two 8-byte
// accesses, still contiguous across the wave).  `al` is uniform over the launch, so no wave diverges on it.  The state's blocks
// start at offsets nE and 2 nE of one allocation: with nE odd the middle block cannot be read in aligned pairs together with the
// others, whatever is peeled off the front.
__device__ __forceinline__ double2 ld2(const double *p, bool al) {
  if (al) return *reinterpret_cast<const double2 *>(p);
  return make_double2(p[0], p[1]);
}
__device__ __forceinline__ void st2(double *p, bool al, double2 v) {
  if (al)
    *reinterpret_cast<double2 *>(p) = v;
  else
    p[0] = v.x, p[1] = v.y;
}
inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Every kernel below walks the pairs (2 j, 2 j + 1), j < n / 2, and -- n odd -- hands the last entry to the thread that would
// have taken pair n / 2: nothing is read or written past entry n - 1.
#define TO_PAIR_LOOP(j, n)                                                                                      \
  for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < ((n) + 1) / 2;                       \
       j += (long long)gridDim.x * blockDim.x)

// stage predictor over the whole state: y = u + c du (all three allocations share the layout and start 16-byte aligned)
__global__ __launch_bounds__(kBlock) void k_predict(const double *__restrict__ u, const double *__restrict__ du,
                                                    double *__restrict__ y, double c, long long n) {
  TO_PAIR_LOOP(j, n) {
    const long long i = 2 * j;
    if (i + 1 < n) {
      const double2 a = ld2(u + i, true), b = ld2(du + i, true);
      st2(y + i, true, make_double2(a.x + c * b.x, a.y + c * b.y));
    } else {
      y[i] = u[i] + c * du[i];
    }
  }
}

// the input of K: w = y2 + a y1
__global__ __launch_bounds__(kBlock) void k_stiffness_input(const double *__restrict__ y1, const double *__restrict__ y2,
                                                            double *__restrict__ w, double a, long long n, bool al2) {
  TO_PAIR_LOOP(j, n) {
    const long long i = 2 * j;
    if (i + 1 < n) {
      const double2 p = ld2(y1 + i, true), q = ld2(y2 + i, al2);
      st2(w + i, true, make_double2(q.x + a * p.x, q.y + a * p.y));
    } else {
      w[i] = y2[i] + a * y1[i];
    }
  }
}

// the right-hand side of the solve: r = -r + g negJ, r holding K (y2 + a y1) + C y1 (negJ == nullptr: no source)
__global__ __launch_bounds__(kBlock) void k_rhs(double *__restrict__ r, const double *__restrict__ negJ, double g, long long n,
                                                bool alJ) {
  TO_PAIR_LOOP(j, n) {
    const long long i = 2 * j;
    if (i + 1 < n) {
      const double2 p = ld2(r + i, true);
      double2 o = make_double2(-p.x, -p.y);
      if (negJ) {
        const double2 s = ld2(negJ + i, alJ);
        o.x += g * s.x, o.y += g * s.y;
      }
      st2(r + i, true, o);
    } else {
      r[i] = -r[i] + (negJ ? g * negJ[i] : 0.0);
    }
  }
}

// k2 = y1 + a k1 and, in the same pass, the input of Curl: w = y2 + a k2
__global__ __launch_bounds__(kBlock) void k_stage_e(const double *__restrict__ y1, const double *__restrict__ y2,
                                                    const double *__restrict__ k1, double *__restrict__ k2, double *__restrict__ w,
                                                    double a, long long n, bool al2) {
  TO_PAIR_LOOP(j, n) {
    const long long i = 2 * j;
    if (i + 1 < n) {
      const double2 p = ld2(y1 + i, true), q = ld2(y2 + i, al2), s = ld2(k1 + i, true);
      const double2 t = make_double2(p.x + a * s.x, p.y + a * s.y);
      st2(k2 + i, al2, t);
      st2(w + i, true, make_double2(q.x + a * t.x, q.y + a * t.y));
    } else {
      const double t = y1[i] + a * k1[i];
      k2[i] = t;
      w[i] = y2[i] + a * t;
    }
  }
}

// The closing update over the whole state: u += a1 du + a2 k, du = c1 du + c2 k, reading three arrays and writing two.  The
// third block of k holds Curl (y2 + a k2), that is -k3: from entry `flip` (= 2 nE, even, so no pair straddles it) on, a2 and
// c2 enter with the opposite sign.
__global__ __launch_bounds__(kBlock) void k_close(double *__restrict__ u, double *__restrict__ du, const double *__restrict__ k,
                                                  double a1, double a2, double c1, double c2, long long flip, long long n) {
  TO_PAIR_LOOP(j, n) {
    const long long i = 2 * j;
    const double s = i >= flip ? -1.0 : 1.0;
    const double b2 = s * a2, d2 = s * c2;
    if (i + 1 < n) {
      const double2 x = ld2(u + i, true), v = ld2(du + i, true), q = ld2(k + i, true);
      st2(u + i, true, make_double2(x.x + a1 * v.x + b2 * q.x, x.y + a1 * v.y + b2 * q.y));
      st2(du + i, true, make_double2(c1 * v.x + d2 * q.x, c1 * v.y + d2 * q.y));
    } else {
      const double x = u[i], v = du[i], q = k[i];
      u[i] = x + a1 * v + b2 * q;
      du[i] = c1 * v + d2 * q;
    }
  }
}

// the last two blocks of du = Mult(u): du2 = u1, du3 = -Curl u2 (the curl waits in the third block of k); i runs over [nE, n).
// Once per integration: plain 8-byte accesses.
__global__ __launch_bounds__(kBlock) void k_first_tail(const double *__restrict__ u, const double *__restrict__ k,
                                                       double *__restrict__ du, long long nE, long long n) {
  for (long long i = nE + (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    du[i] = i < 2 * nE ? u[i - nE] : -k[i];
}

__global__ __launch_bounds__(kBlock) void k_fill(double *__restrict__ x, double s, long long n) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) x[i] = s;
}

void fill(const Context &c, double *x, double s, long long n) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_fill, dim3(grid_for(n)), dim3(kBlock), 0, c.stream, x, s, n);
  PA_HIP(hipGetLastError());
}

constexpr double kGuardValue = -7.0e77;  // what the guard doubles hold

}  // namespace

int TimeOperator::LinearSolve::Mult(const Vector &b, Vector &x, bool guess) const {
  if (ksp_) {
    const int before = ksp_->NumTotalMultIterations();
    ksp_->Mult(b, x);
    return ksp_->NumTotalMultIterations() - before;
  }
  PA_REQUIRE(solver_, "no linear solver has been set");
  solver_->SetInitialGuess(guess);
  solver_->Mult(b, x);
  const auto *it = dynamic_cast<const IterativeSolver *>(solver_);
  return it ? it->GetNumIterations() : 0;
}

double TimeOperator::StageFactor(double rho_inf, double dt) {
  const double alpha_m = 0.5 * (3.0 - rho_inf) / (1.0 + rho_inf), alpha_f = 1.0 / (1.0 + rho_inf);
  const double gamma = 0.5 + alpha_m - alpha_f;
  return alpha_f * gamma / alpha_m * dt;
}

TimeOperator::TimeOperator(const Context &ctx, const Operator *K, const Operator *C, const Operator *M, const Operator &Curl,
                           const Vector &NegJ, std::function<double(double)> dJ_coef, double rho_inf, LinearSolve kspM,
                           std::function<void(double)> configure)
    : ctx_(&ctx), K_(K), C_(C), M_(M), Curl_(&Curl), NegJ_(&NegJ), dJ_(std::move(dJ_coef)), configure_(std::move(configure)),
      kspM_(kspM) {
  PA_REQUIRE(K, "the stiffness operator is required");
  PA_REQUIRE(rho_inf >= 0.0 && rho_inf <= 1.0, "rho_inf must lie in [0, 1]");
  nE_ = K->Height(), nB_ = Curl.Height();
  PA_REQUIRE(nE_ > 0 && nB_ > 0, "empty state");
  PA_REQUIRE(K->Width() == nE_ && (!M || (M->Height() == nE_ && M->Width() == nE_)) && Curl.Width() == nE_ &&
                 (!C || (C->Height() == nE_ && C->Width() == nE_)),
             "operator sizes do not match");
  PA_REQUIRE(NegJ.Size() == 0 || NegJ.Size() == nE_, "the excitation vector has the wrong size");
  PA_REQUIRE(NegJ.Size() == 0 || dJ_, "an excitation vector needs its time dependence");
  PA_REQUIRE(kspM_, "a solver for the mass matrix is required");
  alpha_m_ = 0.5 * (3.0 - rho_inf) / (1.0 + rho_inf);
  alpha_f_ = 1.0 / (1.0 + rho_inf);
  gamma_ = 0.5 + alpha_m_ - alpha_f_;
  rho_inf_ = rho_inf;
  n_ = 2LL * nE_ + nB_;
  // every buffer carries kGuard doubles in front of and behind its data; the stage values are needed only when the predictor
  // has a non-zero coefficient (rho_inf != 1), which is known here: a step allocates nothing
  auto guarded = [&](pa::DevBuf<double> &buf, long long n) {
    buf = pa::dev_alloc<double>((size_t)n + 2 * kGuard);
    fill(ctx, buf, kGuardValue, kGuard);
    fill(ctx, buf + kGuard, 0.0, n);
    fill(ctx, buf + kGuard + n, kGuardValue, kGuard);
  };
  guarded(u_, n_), guarded(du_, n_), guarded(k_, n_), guarded(w_, nE_), guarded(r_, nE_);
  if (alpha_f_ * (1.0 - gamma_ / alpha_m_) != 0.0) guarded(y_, n_);
  double *u = u_ + kGuard;
  Edot_.MakeRef(u, nE_), E_.MakeRef(u + nE_, nE_), B_.MakeRef(u + 2LL * nE_, nB_);
}

const KspSolver &TimeOperator::GetLinearSolver() const {
  PA_REQUIRE(kspA_.Ksp(), "No linear solver for time-dependent operator has been constructed!");
  return *kspA_.Ksp();
}

void TimeOperator::Init() {
  fill(*ctx_, u_ + kGuard, 0.0, n_);
  fill(*ctx_, du_ + kGuard, 0.0, n_);
  started_ = false;
}

void TimeOperator::SetState(const Vector &Edot, const Vector &E, const Vector &B) {
  PA_REQUIRE(Edot.Size() == nE_ && E.Size() == nE_ && B.Size() == nB_, "state blocks of the wrong size");
  linalg::Copy(*ctx_, Edot, Edot_), linalg::Copy(*ctx_, E, E_), linalg::Copy(*ctx_, B, B_);
  fill(*ctx_, du_ + kGuard, 0.0, n_);
  started_ = false;
}

void TimeOperator::FirstDerivative(double t) {
  // du = Mult(u): M du1 = -(K u2 + C u1) + g'(t) NegJ, du2 = u1, du3 = -Curl u2.  The copy of u2 (the stage kernel with a = 0)
  // gives K and Curl an input at a 16-byte boundary.
  const hipStream_t s = ctx_->stream;
  double *u = u_ + kGuard, *du = du_ + kGuard;
  double *kb = k_ + kGuard, *wb = w_ + kGuard, *rb = r_ + kGuard;
  const double *u1 = u, *u2 = u + nE_;
  const int grid = grid_for((nE_ + 1LL) / 2);
  hipLaunchKernelGGL(k_stiffness_input, dim3(grid), dim3(kBlock), 0, s, u1, u2, wb, 0.0, (long long)nE_, aligned16(u2));
  PA_HIP(hipGetLastError());
  Vector w(wb, nE_), r(rb, nE_), v1(u, nE_), d1(du, nE_), c3(kb + 2LL * nE_, nB_);
  K_->Mult(w, r), stats_.k_applies++;
  if (C_) C_->AddMult(v1, r, 1.0), stats_.c_applies++;
  const double *negJ = NegJ_->Size() ? NegJ_->Data() : nullptr;
  hipLaunchKernelGGL(k_rhs, dim3(grid), dim3(kBlock), 0, s, rb, negJ, negJ ? dJ_(t) : 0.0, (long long)nE_, aligned16(negJ));
  PA_HIP(hipGetLastError());
  stats_.m_iterations += kspM_.Mult(r, d1, false), stats_.m_solves++;  // (du was zeroed: timeoperator.cpp:154-158)
  Curl_->Mult(w, c3), stats_.curl_applies++;
  hipLaunchKernelGGL(k_first_tail, dim3(grid_for(n_ - nE_)), dim3(kBlock), 0, s, u, kb, du, (long long)nE_, n_);
  PA_HIP(hipGetLastError());
  stats_.ew_launches += 3;
}

void TimeOperator::ImplicitSolve(double a, double t, const double *y) {
  if (!have_a_ || a != a_) {
    PA_REQUIRE(configure_, "the stage factor changed and there is no callback to rebuild the system");
    configure_(a), stats_.configures++;
    PA_REQUIRE(kspA_, "the callback did not hand over a linear solver (SetLinearSolver)");
    a_ = a, have_a_ = true;
    fill(*ctx_, k_ + kGuard, 0.0, n_);  // (timeoperator.cpp:192: the starting iterate of the first solve)
  }
  const hipStream_t s = ctx_->stream;
  const double *y1 = y, *y2 = y + nE_;
  double *kb = k_ + kGuard, *wb = w_ + kGuard, *rb = r_ + kGuard;
  double *k1 = kb, *k2 = kb + nE_;
  const bool al2 = aligned16(y2);  // (y and k share the layout and the alignment of their bases)
  const int grid = grid_for((nE_ + 1LL) / 2);
  Vector w(wb, nE_), r(rb, nE_), v1(const_cast<double *>(y1), nE_), x1(k1, nE_), c3(kb + 2LL * nE_, nB_);

  // A k1 = -K (y2 + a y1) - C y1 + g' NegJ
  hipLaunchKernelGGL(k_stiffness_input, dim3(grid), dim3(kBlock), 0, s, y1, y2, wb, a, (long long)nE_, al2);
  PA_HIP(hipGetLastError());
  K_->Mult(w, r), stats_.k_applies++;
  if (C_) C_->AddMult(v1, r, 1.0), stats_.c_applies++;
  const double *negJ = NegJ_->Size() ? NegJ_->Data() : nullptr;
  hipLaunchKernelGGL(k_rhs, dim3(grid), dim3(kBlock), 0, s, rb, negJ, negJ ? dJ_(t) : 0.0, (long long)nE_, aligned16(negJ));
  PA_HIP(hipGetLastError());
  stats_.a_iterations += kspA_.Mult(r, x1, true), stats_.a_solves++;

  // k2 = y1 + a k1;  Curl (y2 + a k2) = -k3
  hipLaunchKernelGGL(k_stage_e, dim3(grid), dim3(kBlock), 0, s, y1, y2, k1, k2, wb, a, (long long)nE_, al2);
  PA_HIP(hipGetLastError());
  Curl_->Mult(w, c3), stats_.curl_applies++;
  stats_.ew_launches += 3;
}

void TimeOperator::Step(double &t, double &dt) {
  PhaseRange range("Time Stepping");  // utils/timer.hpp: Timer::TS
  if (!started_) {
    FirstDerivative(t);
    started_ = true;
  }
  const hipStream_t s = ctx_->stream;
  double *u = u_ + kGuard, *du = du_ + kGuard;
  const double gm = gamma_ / alpha_m_;
  // y = u + alpha_f (1 - gamma / alpha_m) dt du: with rho_inf = 1 the coefficient is zero and y is u itself
  const double cp = alpha_f_ * (1.0 - gm) * dt;
  const double *y = u;
  if (cp != 0.0) {
    PA_REQUIRE(y_, "no stage vector");  // (allocated by the constructor whenever the coefficient can be non-zero)
    hipLaunchKernelGGL(k_predict, dim3(grid_for((n_ + 1) / 2)), dim3(kBlock), 0, s, u, du, y_ + kGuard, cp, n_);
    PA_HIP(hipGetLastError());
    stats_.ew_launches++, stats_.predictor_launches++;
    y = y_ + kGuard;
  }
  // (the one expression a caller of StageFactor evaluates: a callback may compare the two for equality)
  ImplicitSolve(StageFactor(rho_inf_, dt), t + alpha_f_ * dt, y);
  hipLaunchKernelGGL(k_close, dim3(grid_for((n_ + 1) / 2)), dim3(kBlock), 0, s, u, du, k_ + kGuard, (1.0 - gm) * dt, gm * dt,
                     1.0 - 1.0 / alpha_m_, 1.0 / alpha_m_, 2LL * nE_, n_);
  PA_HIP(hipGetLastError());
  stats_.ew_launches++, stats_.steps++;
  t += dt;
}

bool TimeOperator::GuardsIntact() const {
  StreamGraph::RequireNotRecording("TimeOperator::GuardsIntact");
  std::vector<double> h(2 * kGuard);
  const std::pair<const double *, long long> bufs[] = {{u_, n_}, {du_, n_}, {k_, n_}, {w_, nE_}, {r_, nE_}, {y_, n_}};
  PA_HIP(hipStreamSynchronize(ctx_->stream));
  for (const auto &[p, n] : bufs) {
    if (!p) continue;
    PA_HIP(hipMemcpy(h.data(), p, sizeof(double) * kGuard, hipMemcpyDeviceToHost));
    PA_HIP(hipMemcpy(h.data() + kGuard, p + kGuard + n, sizeof(double) * kGuard, hipMemcpyDeviceToHost));
    for (double v : h)
      if (std::memcmp(&v, &kGuardValue, sizeof(double)) != 0) return false;
  }
  return true;
}

void TimeOperator::PrintStats() const {
  const Stats &s = stats_;
  std::printf("Time stepping: %lld steps, %lld K / %lld C / %lld Curl applies, %lld solves with A (%lld iterations), "
              "%lld with M (%lld iterations), %lld element-wise launches\n",
              s.steps, s.k_applies, s.c_applies, s.curl_applies, s.a_solves, s.a_iterations, s.m_solves, s.m_iterations,
              s.ew_launches);
}

double PulseValue(int kind, double omega, double tau, double t0, double t) {
  const double ts = t - t0;
  switch (kind) {
    case 0: return std::sin(omega * ts);
    case 1: return std::exp(-0.5 * ts * ts / (tau * tau));
    case 2: return -ts / (tau * tau) * std::exp(-0.5 * ts * ts / (tau * tau));
    case 3: return std::sin(omega * ts) * std::exp(-0.5 * ts * ts / (tau * tau));
    case 4: return ts <= 0.0 ? 0.0 : (ts >= tau ? 1.0 : ts / tau);
    case 5: {
      const double x = ts <= 0.0 ? 0.0 : (ts >= tau ? 1.0 : ts / tau);
      return x * x * x * (6.0 * x * x - 15.0 * x + 10.0);
    }
  }
  throw pa::Error("unknown pulse kind");
}

double PulseDerivative(int kind, double omega, double tau, double t0, double t) {
  const double ts = t - t0, oot2 = tau != 0.0 ? 1.0 / (tau * tau) : 0.0;
  switch (kind) {
    case 0: return omega * std::cos(omega * ts);
    case 1: return -ts * oot2 * std::exp(-0.5 * ts * ts * oot2);
    case 2: return -oot2 * (1.0 - ts * ts * oot2) * std::exp(-0.5 * ts * ts * oot2);
    case 3: return (-ts * oot2 * std::sin(omega * ts) + omega * std::cos(omega * ts)) * std::exp(-0.5 * ts * ts * oot2);
    case 4: return (ts <= 0.0 || ts >= tau) ? 0.0 : 1.0 / tau;
    case 5: {
      const double x = ts <= 0.0 ? 0.0 : (ts >= tau ? 1.0 : ts / tau);
      return 30.0 * x * x * (x - 1.0) * (x - 1.0) / tau;
    }
  }
  throw pa::Error("unknown pulse kind");
}

}  // namespace palace
