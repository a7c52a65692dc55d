// Time integration of the first-order system the reference's transient driver advances (models/timeoperator.{hpp,cpp},
// drivers/transientsolver.cpp:25-116): the state u = (u1, u2, u3) = (dE/dt, E, B) of sizes (nE, nE, nB) in ONE device
// allocation (blocks at offsets 0, nE and 2 nE), with
//     M u1' = -(K u2 + C u1) + g'(t) NegJ         K, C: DIAG_ZERO on the essential rows, M: DIAG_ONE
//       u2' = u1
//       u3' = -Curl u2
// (TimeDependentFirstOrderOperator, timeoperator.cpp:22-282) and the generalized-alpha stepper for first-order systems
// (Jansen, Whiting, Hulbert 2000; mfem::GeneralizedAlphaSolver, which TimeOperator selects with rho_inf = 1, :317-322):
//     alpha_m = (3 - rho) / (2 (1 + rho)),  alpha_f = 1 / (1 + rho),  gamma = 1/2 + alpha_m - alpha_f
//     first step only:  du = Mult(u) at t                               (M^-1 of the right-hand side)
//     y  = u + alpha_f (1 - gamma / alpha_m) dt du
//     k  = ImplicitSolve(a, y) at t + alpha_f dt,  a = alpha_f gamma / alpha_m dt
//     u  = u + (1 - gamma / alpha_m) dt du + gamma / alpha_m dt k
//     du = (1 - 1 / alpha_m) du + k / alpha_m
// ImplicitSolve is the reference's block elimination (:182-223) with its separate applies merged:
//     A k1 = -K (y2 + a y1) - C y1 + g' NegJ,  A = M + a C + a^2 K       (rhs1(y) - a K y1 in the reference: two K applies)
//     k2   = y1 + a k1
//     k3   = -Curl (y2 + a k2)                                            (-Curl y2 - a Curl k2 in the reference: two applies)
// so one step is one K apply, one C apply (none without C), one Curl apply, one solve with A and four element-wise launches
// (five when the stage predictor has a non-zero coefficient, rho_inf != 1).  The element-wise kernels are in timeoperator.hip.
// The step is a plain launch sequence on the context's stream: it is not recorded as a graph of its own (g' changes every step;
// the solvers keep their own recordings).
#pragma once

#include <functional>

#include "ksp.hpp"
#include "linalg.hpp"

namespace palace {

class TimeOperator {
public:
  // what a driver reads in place of a profile: how often each piece ran since construction
  struct Stats {
    long long steps = 0;
    long long k_applies = 0, c_applies = 0, curl_applies = 0;
    long long a_solves = 0, m_solves = 0;
    long long a_iterations = 0, m_iterations = 0;  // Krylov iterations of the two solvers
    long long ew_launches = 0;                     // element-wise launches over state-sized data (timeoperator.hip)
    long long predictor_launches = 0;              // ... of which stage predictors (none when rho_inf = 1)
    long long configures = 0;                      // calls of the (re)build callback
  };
  // The solver of one linear system: the drivers' KspSolver (its own initial-guess setting holds), or a bare Solver of the C
  // ABI (an IterativeSolver reports its iterations; `guess` says whether the solution vector is a starting iterate).
  class LinearSolve {
    const KspSolver *ksp_ = nullptr;
    Solver *solver_ = nullptr;

  public:
    LinearSolve() = default;
    LinearSolve(const KspSolver &ksp) : ksp_(&ksp) {}
    LinearSolve(Solver &solver) : solver_(&solver) {}
    explicit operator bool() const { return ksp_ || solver_; }
    const KspSolver *Ksp() const { return ksp_; }
    // returns the iterations of this solve.  Side effect on a bare Solver: its initial-guess flag is SET to `guess` and stays
    // so (the flag has no getter to restore it from; pa_solver_mult sets it on every call as well), so a caller that shares
    // the solver sets the flag itself before its own solves
    int Mult(const Vector &b, Vector &x, bool guess) const;
  };

  // K, C (may be null), M (may be null: only its solver is applied): true-dof operators of size nE (ParOperators with the
  // policies above); Curl: nB x nE; NegJ: the excitation vector (nE; may be empty: no source); dJ_coef: g'(t).  kspM solves
  // with M (Jacobi-PCG in the reference, :79-88).
  // configure(a) (re)builds A(a) = M + a C + a^2 K and its solver, and hands the solver over with SetLinearSolver; it is called
  // when the stage factor a first appears or changes, as ConfigureLinearSolver is (:186-193).  None of the arguments is owned.
  TimeOperator(const Context &ctx, const Operator *K, const Operator *C, const Operator *M, const Operator &Curl,
               const Vector &NegJ, std::function<double(double)> dJ_coef, double rho_inf, LinearSolve kspM,
               std::function<void(double)> configure);
  TimeOperator(const TimeOperator &) = delete;
  TimeOperator &operator=(const TimeOperator &) = delete;

  void SetLinearSolver(LinearSolve kspA) { kspA_ = kspA; }
  const KspSolver &GetLinearSolver() const;  // timeoperator.cpp:390-396 (the KspSolver form only)

  // a = alpha_f gamma / alpha_m dt: the factor of A(a) a step of size dt solves with
  static double StageFactor(double rho_inf, double dt);

  void Init();  // zero initial conditions (timeoperator.cpp:398-406); the next Step starts a new integration
  // any other initial state (not in the reference, which always starts from zero); device vectors, copied
  void SetState(const Vector &Edot, const Vector &E, const Vector &B);
  void Step(double &t, double &dt);  // t -> t + dt; dt comes back unchanged (:408-414)

  const Operator *GetMassOperator() const { return M_; }
  int SizeE() const { return nE_; }
  int SizeB() const { return nB_; }
  const Vector &GetE() const { return E_; }
  const Vector &GetEdot() const { return Edot_; }
  const Vector &GetB() const { return B_; }
  // The whole state (u) and its time derivative (du), 2 nE + nB doubles each.  Every allocation of the object (these two, k, the
  // stage values, the two work vectors) carries kGuard doubles in front of and behind the data, filled once at construction and
  // never written again; GuardsIntact() reads them all back and compares the bits (it waits for the stream: tests).
  static constexpr int kGuard = 64;
  bool GuardsIntact() const;
  const double *State() const { return u_ + kGuard; }
  const double *StateDot() const { return du_ + kGuard; }
  const Stats &GetStats() const { return stats_; }
  void PrintStats() const;

private:
  const Context *ctx_;
  const Operator *K_, *C_, *M_, *Curl_;
  const Vector *NegJ_;
  std::function<double(double)> dJ_;
  std::function<void(double)> configure_;
  LinearSolve kspM_, kspA_;
  double rho_inf_, alpha_m_, alpha_f_, gamma_;
  int nE_, nB_;
  long long n_;  // 2 nE + nB
  // u, du, the stage values y (allocated by the constructor when rho_inf != 1) and k = (k1, k2, Curl(...)) in the state's
  // layout; w: the input of K, then of Curl (nE entries both); r: K's output, then the right-hand side.  Every vector an
  // operator or a solver sees starts at a 16-byte boundary (k1, Curl's output at 2 nE, w, r); the blocks at offset nE, which
  // are 8-byte aligned when nE is odd, are touched by this file's kernels alone.
  pa::DevBuf<double> u_, du_, y_, k_, w_, r_;
  Vector Edot_, E_, B_;
  double a_ = 0.0;
  bool have_a_ = false, started_ = false;
  Stats stats_;

  void FirstDerivative(double t);  // du = Mult(u) (:148-180)
  void ImplicitSolve(double a, double t, const double *y);
};

// The excitation pulses of utils/excitations.hpp with the delay of drivers/transientsolver.cpp:135-138 applied by the caller:
// value g(t) and derivative g'(t).  kind: 0 sinusoidal, 1 Gaussian, 2 differentiated Gaussian, 3 modulated Gaussian, 4 ramp,
// 5 smoother step.
double PulseValue(int kind, double omega, double tau, double t0, double t);
double PulseDerivative(int kind, double omega, double tau, double t0, double t);

}  // namespace palace
