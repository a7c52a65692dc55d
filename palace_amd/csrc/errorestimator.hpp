// The flux error estimators of linalg/errorestimator.{hpp,cpp} in 3-D: smooth flux recovery by a mass-matrix projection
// (FluxProjector, :111-187), element-wise error between the discontinuous and the smooth flux (ComputeErrorEstimates,
// :189-268), and the two estimators built on them (GradFluxErrorEstimator :271-360, CurlFluxErrorEstimator :390-510,
// TimeDependentFluxErrorEstimator :512-541), plus the running indicator they feed (fem/errorindicator.{hpp,cpp}).
// Spaces are two dense-table spaces on one dense Mesh (fem.hpp; the operators are pa_op_add_sub_dense[_mixed] and
// pa_error_op_create, pa_mixed.hip) or, for the 3-D vector estimators on hexahedra, two tensor spaces of one order on one tensor
// Mesh (pa_op_add_sub, pa_op_add_sub_mixed and pa_error_op_create_tensor: sum-factorised, pa_rt_hex.hip / pa_nd_hex.hip /
// pa_mixed_hex.hip).  FluxProjector and the two estimators come for real vectors and, as Complex*, for a ComplexVector (the
// reference's second instantiation, errorestimator.cpp:183-268, :272-480).  There the flux operator (ceed::Operator::Mult2) and the
// error integrator (pa_error_op_apply_add2) take both parts together, and so does the mass apply inside the PCG where it can:
// on one rank, where the mass operator has a two-vector kernel and no streaming form (ComplexMassOperator below); with a halo, or
// without such a kernel, the mass solve runs two applies per iteration.  On tensor hexahedra "together" is one pass over the
// element data where a two-part kernel is compiled in (pa_op_two_rhs, pa_error_op_two_parts), two passes in the reference's
// order everywhere else.
#pragma once

#include <array>
#include <memory>
#include <vector>

#include "amg_solver.hpp"
#include "complex.hpp"
#include "fem.hpp"
#include "ksp.hpp"

namespace palace {

namespace linalg {
// f(M) for a symmetric 3x3 matrix (column-major) through its eigen-decomposition: MatrixSqrt / MatrixPow of
// linalg/densematrix.cpp:222-252 as the estimators use them on the material tensors
std::array<double, 9> MatrixSqrt(const double *M);
std::array<double, 9> MatrixPow(const double *M, double p);
}  // namespace linalg

// fem/errorindicator.{hpp,cpp}: running root-mean-square of the element indicators over the solves of a simulation
class ErrorIndicator {
  const Context *ctx_;
  Vector local_;
  int n_ = 0;

public:
  explicit ErrorIndicator(const Context &ctx) : ctx_(&ctx) {}
  void AddIndicator(const Vector &indicator);  // errorindicator.cpp:11-47
  const Vector &Local() const { return local_; }
  double Norml2() const;
  int NumSamples() const { return n_; }
};

// what MaterialOperator hands to the estimators: attribute -> material index and one symmetric dim x dim tensor per material
// (mat_op.GetAttributeToMaterial() with GetPermittivityReal(), GetInvPermeability() or, for the scalar curl of a plane
// problem, the 1 x 1 GetCurlCurlInvPermeability(); column-major).  dim = 3 unless stated.
struct MaterialTensors {
  std::vector<int> attr_mat;
  std::vector<double> mat;  // [num_mat][dim * dim]
  int dim = 3;
  // f acts on symmetric 3 x 3 matrices: smaller tensors are bordered with an identity block, which f maps to itself
  // up to f(1) and which is dropped again
  template <typename F>
  MaterialTensors Map(F &&f) const {
    MaterialTensors out{attr_mat, mat, dim};
    const size_t dd = (size_t)dim * dim;
    for (size_t k = 0; k + dd <= mat.size(); k += dd) {
      double M[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
      for (int j = 0; j < dim; j++)
        for (int i = 0; i < dim; i++) M[i + 3 * j] = mat[k + i + (size_t)dim * j];
      const auto m = f(M);
      for (int j = 0; j < dim; j++)
        for (int i = 0; i < dim; i++) out.mat[k + i + (size_t)dim * j] = m[i + 3 * j];
    }
    return out;
  }
  MaterialPropertyCoefficient Coefficient() const { return MaterialPropertyCoefficient(attr_mat, dim, mat); }
};

// errorestimator.hpp:34-58, .cpp:111-187: y = M^-1 Flux x with M the mass matrix of the smooth space and Flux the
// coefficient-weighted mixed mass from the space of x into the smooth space; PCG + Jacobi (use_mg = false), or PCG preconditioned
// by a p-multigrid cycle over a hierarchy of the smooth space (use_mg = true, ConfigureLinearSolver :67-104): the system operator
// is the MultigridOperator of the levels' masses, the cycle one pre and one post step of 4th-kind Chebyshev of order 2 and one
// native AMG cycle (strength threshold 0.8) on the fully assembled coarsest level; a one-level hierarchy gets the AMG alone.
// One rank.
// On a mesh with hanging nodes either space may carry a Conforming prolongation P (fem.hpp: SetConformingProlongation): the
// right-hand side is then P_smooth^T Flux P_rhs x, M the ParOperator P^T M P, Jacobi its |P|^T diag (rap.cpp:163-175), and the
// estimators prolongate F and G through P before the element integrator.  use_mg with a constrained smooth space is refused.

// BoomerAmgSolver(1, 1, true, 0) with SetStrengthThresh(0.8) as the projectors' coarse solve (:81-82): one cycle of the native
// AMG on the assembled matrix of the level it is given (a ParOperator or FespaceParOperator without a halo)
class FluxAmgSolver : public Solver {
  const Context *ctx_;
  std::unique_ptr<AmgSolver> amg_;

public:
  explicit FluxAmgSolver(const Context &ctx) : ctx_(&ctx) {}
  void SetOperator(const Operator &op) override;
  void Mult(const Vector &b, Vector &x) const override;
  const AmgSolver *Amg() const { return amg_.get(); }
};

class FluxProjector {
  const Context *ctx_;
  std::unique_ptr<ceed::Operator> flux_, mass_;
  std::unique_ptr<ParOperator> M_;
  std::unique_ptr<MultigridOperator> M_mg_;  // use_mg: the masses of all levels
  std::unique_ptr<Solver> pc_;
  std::unique_ptr<CgSolver> pcg_;
  const FiniteElementSpace *smooth_, *rhs_space_;
  mutable Vector rhs_, lx_, ly_;
  void Init(const MaterialPropertyCoefficient &coeff, const FiniteElementSpaceHierarchy *smooth_fespaces, double tol, int max_it,
            int print);

public:
  FluxProjector(const MaterialPropertyCoefficient &coeff, const FiniteElementSpace &smooth_fespace,
                const FiniteElementSpace &rhs_fespace, double tol, int max_it, int print);
  FluxProjector(const MaterialPropertyCoefficient &coeff, const FiniteElementSpaceHierarchy &smooth_fespaces,
                const FiniteElementSpace &rhs_fespace, double tol, int max_it, int print, bool use_mg);
  bool UsesMultigrid() const { return M_mg_ != nullptr; }
  bool Converged() const { return pcg_->GetConverged(); }
  void Mult(const Vector &x, Vector &y) const;
  int NumIterations() const { return pcg_->GetNumIterations(); }
};

// Common part of the two estimators: F in `fespace`, its smooth recovery G in `smooth_fespace`, estimates += error^2
class FluxErrorEstimatorBase {
protected:
  const Context *ctx_;
  const FiniteElementSpace &fespace_, &smooth_fespace_;
  FluxProjector projector_;
  pa_error_op *integ_op_ = nullptr;
  mutable Vector G_;

  FluxErrorEstimatorBase(const FiniteElementSpace &fespace, const FiniteElementSpace &smooth_fespace,
                         const MaterialPropertyCoefficient &flux_coeff, int error_qf, const MaterialTensors &first,
                         const MaterialTensors &second, double tol, int max_it, int print);
  FluxErrorEstimatorBase(const FiniteElementSpace &fespace, const FiniteElementSpaceHierarchy &smooth_fespaces,
                         const MaterialPropertyCoefficient &flux_coeff, int error_qf, const MaterialTensors &first,
                         const MaterialTensors &second, double tol, int max_it, int print, bool use_mg);

public:
  virtual ~FluxErrorEstimatorBase();
  FluxErrorEstimatorBase(const FluxErrorEstimatorBase &) = delete;
  // ComputeErrorEstimates (:189-268): squared element errors added to `estimates` [num_elem]
  void AddErrorEstimates(const Vector &F, Vector &estimates) const;
  // AddErrorIndicator (:352-360, :502-510): sqrt(estimates) scaled by the total field energy
  void AddErrorIndicator(const Vector &F, double Et, ErrorIndicator &indicator) const;
  int NumElements() const { return fespace_.GetMesh().GetNE(); }
  const FluxProjector &GetProjector() const { return projector_; }
  const Vector &GetSmoothFlux() const { return G_; }
};

// eta_e^2 = || eps^-1/2 D - eps^1/2 E ||^2_e with D the RT recovery of eps E (E in ND)
class GradFluxErrorEstimator : public FluxErrorEstimatorBase {
public:
  GradFluxErrorEstimator(const MaterialTensors &epsilon, const FiniteElementSpace &nd_fespace,
                         const FiniteElementSpace &rt_fespace, double tol, int max_it, int print);
  // errorestimator.cpp:272-280: the smooth space as a hierarchy (`rt_fespaces`), the projector's use_mg passed through
  GradFluxErrorEstimator(const MaterialTensors &epsilon, const FiniteElementSpace &nd_fespace,
                         const FiniteElementSpaceHierarchy &rt_fespaces, double tol, int max_it, int print, bool use_mg);
};

// eta_e^2 = || mu^1/2 H - mu^-1/2 B ||^2_e with H the ND recovery of mu^-1 B (B in RT).  Plane problems: B = curl E is a scalar
// in a discontinuous space, H its H1 recovery, muinv the 1 x 1 curl-curl tensor (errorestimator.cpp:446-472, f_apply_l2h1_error)
class CurlFluxErrorEstimator : public FluxErrorEstimatorBase {
public:
  CurlFluxErrorEstimator(const MaterialTensors &muinv, const FiniteElementSpace &rt_fespace,
                         const FiniteElementSpace &nd_fespace, double tol, int max_it, int print);
  // errorestimator.cpp:394-398 (`nd_fespaces`)
  CurlFluxErrorEstimator(const MaterialTensors &muinv, const FiniteElementSpace &rt_fespace,
                         const FiniteElementSpaceHierarchy &nd_fespaces, double tol, int max_it, int print, bool use_mg);
};

// FluxProjector<ComplexVector> (errorestimator.cpp:111-187): the same two forms; M is a ComplexParOperator with a real part only
// (BuildLevelParOperator<ComplexOperator>, :50-65), the solver ComplexCgSolver + ComplexJacobiSmoother (ConfigureLinearSolver
// with use_mg = false), the flux operator is applied to both parts at once (ceed::Operator::Mult2)
// The projector's system matrix as the PCG applies it: y = M x on both parts of x.  ComplexParOperator::Mult applies a real
// part without essential dofs as two one-part applies; here, on one rank and where the mass operator has a two-vector kernel and
// no streaming form (pa_op_two_rhs, pa_op_streams), both parts go through one ceed::Operator::Mult2.  Everything else, and the
// diagonal, is the ComplexParOperator's.
// On a smooth space with hanging-node constraints (conf) the one-pass route is P2, Mult2, P^T2 (Conforming::Prolongate2 /
// Restrict2): three launches where the two real ParOperators of the ComplexParOperator take six.
class ComplexMassOperator : public ComplexOperator {
  const Context *ctx_;
  const ceed::Operator *mass_;
  const ComplexParOperator *par_;
  bool has_halo_;
  const Conforming *conf_;
  mutable ComplexVector lx_, ly_;
  mutable long one_pass_applies_ = 0;

public:
  ComplexMassOperator(const Context &ctx, const ceed::Operator &mass, const ComplexParOperator &par, bool has_halo,
                      const Conforming *conf = nullptr);
  const Operator *Real() const override { return par_->Real(); }
  void AssembleDiagonal(ComplexVector &diag) const override { par_->AssembleDiagonal(diag); }
  void Mult(const ComplexVector &x, ComplexVector &y) const override;
  bool OnePass() const;                                       // the route Mult takes (PALACE_AMD_TWO_PART is read at every call)
  long OnePassApplies() const { return one_pass_applies_; }   // how often it took the one-pass route
};

// use_mg: the levels' masses as ComplexParOperators with a real part only, a ComplexGeometricMultigridSolver with complex Chebyshev
// smoothers and the real FluxAmgSolver wrapped for both parts (MfemWrapperSolver<ComplexOperator>) as coarse solve; the PCG still
// applies the finest mass through ComplexMassOperator (one pass where there is one)
class ComplexFluxProjector {
  const Context *ctx_;
  std::unique_ptr<ceed::Operator> flux_, mass_;
  std::vector<std::unique_ptr<Operator>> level_mass_;          // use_mg: the local masses of all levels, finest last
  std::vector<std::unique_ptr<ComplexParOperator>> level_M_;   // ... and their complex ParOperators
  std::unique_ptr<ComplexParOperator> M_;
  std::unique_ptr<ComplexMassOperator> Mboth_;
  std::unique_ptr<FluxAmgSolver> amg_;
  std::unique_ptr<ComplexSolver> pc_;
  std::unique_ptr<ComplexCgSolver> pcg_;
  const FiniteElementSpace *smooth_, *rhs_space_;
  mutable ComplexVector rhs_, lx_, ly_;
  void Init(const MaterialPropertyCoefficient &coeff, const FiniteElementSpaceHierarchy *smooth_fespaces, double tol, int max_it,
            int print);

public:
  ComplexFluxProjector(const MaterialPropertyCoefficient &coeff, const FiniteElementSpace &smooth_fespace,
                       const FiniteElementSpace &rhs_fespace, double tol, int max_it, int print);
  ComplexFluxProjector(const MaterialPropertyCoefficient &coeff, const FiniteElementSpaceHierarchy &smooth_fespaces,
                       const FiniteElementSpace &rhs_fespace, double tol, int max_it, int print, bool use_mg);
  void Mult(const ComplexVector &x, ComplexVector &y) const;
  int NumIterations() const { return pcg_->GetNumIterations(); }
  bool UsesMultigrid() const { return !level_M_.empty(); }
  bool Converged() const { return pcg_->GetConverged(); }
  bool FluxTwoRhs() const;  // the flux operator takes both parts in one pass over the element data (pa_op_two_rhs)
  bool MassTwoRhs() const { return Mboth_->OnePass(); }  // ... and so does the mass apply inside the PCG (the route taken)
  long MassOnePassApplies() const { return Mboth_->OnePassApplies(); }  // mass applies that went through Mult2 so far
};

// The estimators for a complex field: F and its smooth recovery G as ComplexVectors, estimates += error^2 of the real parts +
// error^2 of the imaginary parts (ComputeErrorEstimates, :249-261) through one pa_error_op_apply_add2
class ComplexFluxErrorEstimatorBase {
protected:
  const Context *ctx_;
  const FiniteElementSpace &fespace_, &smooth_fespace_;
  ComplexFluxProjector projector_;
  pa_error_op *integ_op_ = nullptr;
  mutable ComplexVector G_;

  ComplexFluxErrorEstimatorBase(const FiniteElementSpace &fespace, const FiniteElementSpace &smooth_fespace,
                                const MaterialPropertyCoefficient &flux_coeff, int error_qf, const MaterialTensors &first,
                                const MaterialTensors &second, double tol, int max_it, int print);
  ComplexFluxErrorEstimatorBase(const FiniteElementSpace &fespace, const FiniteElementSpaceHierarchy &smooth_fespaces,
                                const MaterialPropertyCoefficient &flux_coeff, int error_qf, const MaterialTensors &first,
                                const MaterialTensors &second, double tol, int max_it, int print, bool use_mg);

public:
  virtual ~ComplexFluxErrorEstimatorBase();
  ComplexFluxErrorEstimatorBase(const ComplexFluxErrorEstimatorBase &) = delete;
  void AddErrorEstimates(const ComplexVector &F, Vector &estimates) const;
  void AddErrorIndicator(const ComplexVector &F, double Et, ErrorIndicator &indicator) const;
  int NumElements() const { return fespace_.GetMesh().GetNE(); }
  const ComplexFluxProjector &GetProjector() const { return projector_; }
  const ComplexVector &GetSmoothFlux() const { return G_; }
  bool TwoParts() const { return pa_error_op_two_parts(integ_op_) != 0; }  // the error integrator runs one launch for both parts
};

class ComplexGradFluxErrorEstimator : public ComplexFluxErrorEstimatorBase {
public:
  ComplexGradFluxErrorEstimator(const MaterialTensors &epsilon, const FiniteElementSpace &nd_fespace,
                                const FiniteElementSpace &rt_fespace, double tol, int max_it, int print);
  ComplexGradFluxErrorEstimator(const MaterialTensors &epsilon, const FiniteElementSpace &nd_fespace,
                                const FiniteElementSpaceHierarchy &rt_fespaces, double tol, int max_it, int print, bool use_mg);
};

class ComplexCurlFluxErrorEstimator : public ComplexFluxErrorEstimatorBase {
public:
  ComplexCurlFluxErrorEstimator(const MaterialTensors &muinv, const FiniteElementSpace &rt_fespace,
                                const FiniteElementSpace &nd_fespace, double tol, int max_it, int print);
  ComplexCurlFluxErrorEstimator(const MaterialTensors &muinv, const FiniteElementSpace &rt_fespace,
                                const FiniteElementSpaceHierarchy &nd_fespaces, double tol, int max_it, int print, bool use_mg);
};

// :512-541: both of the above added before the square root (real in the reference)
class TimeDependentFluxErrorEstimator {
  const Context *ctx_;
  GradFluxErrorEstimator grad_;
  CurlFluxErrorEstimator curl_;

public:
  TimeDependentFluxErrorEstimator(const MaterialTensors &epsilon, const MaterialTensors &muinv,
                                  const FiniteElementSpace &nd_fespace, const FiniteElementSpace &rt_fespace, double tol,
                                  int max_it, int print);
  // :512-520: both hierarchies, the finest spaces carry the fields
  TimeDependentFluxErrorEstimator(const MaterialTensors &epsilon, const MaterialTensors &muinv,
                                  const FiniteElementSpaceHierarchy &nd_fespaces, const FiniteElementSpaceHierarchy &rt_fespaces,
                                  double tol, int max_it, int print, bool use_mg);
  void AddErrorIndicator(const Vector &E, const Vector &B, double Et, ErrorIndicator &indicator) const;
};

}  // namespace palace
