// Flux error estimators (see errorestimator.hpp).  Host orchestration + two small element-wise kernels.
#include "errorestimator.hpp"

#include <hip/hip_runtime.h>

#include <cmath>
#include <limits>

namespace palace {

namespace {

void check(int rc) {
  if (rc) throw pa::Error(pa_last_error());
}

// errorindicator.cpp:41-43
__global__ void k_indicator_update(double *__restrict__ local, const double *__restrict__ ind, const int dn, const int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) local[i] = sqrt((local[i] * local[i] * dn + ind[i] * ind[i]) / (dn + 1));
}

// Symmetric 3x3 eigen-decomposition by cyclic Jacobi rotations (the reference goes through MFEM's dense eigensolver,
// densematrix.cpp:150-220; any orthogonal diagonalisation gives the same f(M))
template <typename F>
std::array<double, 9> matrix_function(const double *M, F &&f) {
  double A[3][3], V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) A[i][j] = 0.5 * (M[i + 3 * j] + M[j + 3 * i]);
  for (int sweep = 0; sweep < 64; sweep++) {
    const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
    const double diag = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2];
    if (off <= 1e-32 * diag || off == 0.0) break;
    for (int p = 0; p < 2; p++)
      for (int q = p + 1; q < 3; q++) {
        if (A[p][q] == 0.0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 3; k++) {  // A <- A J
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq, A[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < 3; k++) {  // A <- J^T A
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk, A[q][k] = s * apk + c * aqk;
        }
        for (int k = 0; k < 3; k++) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq, V[k][q] = s * vkp + c * vkq;
        }
      }
  }
  std::array<double, 9> out{};
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      double v = 0.0;
      for (int k = 0; k < 3; k++) v += V[i][k] * f(A[k][k]) * V[j][k];
      out[i + 3 * j] = v;
    }
  return out;
}

}  // namespace

namespace linalg {

std::array<double, 9> MatrixSqrt(const double *M) {
  return matrix_function(M, [](double s) { return std::sqrt(s); });
}
std::array<double, 9> MatrixPow(const double *M, double p) {
  return matrix_function(M, [p](double s) { return std::pow(s, p); });
}

}  // namespace linalg

// ---- ErrorIndicator --------------------------------------------------------------------------------------------------
void ErrorIndicator::AddIndicator(const Vector &indicator) {
  if (n_ == 0) {
    local_.SetSize(indicator.Size());
    linalg::Copy(*ctx_, indicator, local_);
    n_ = 1;
    return;
  }
  PA_REQUIRE(local_.Size() == indicator.Size(), "Unexpected size mismatch for ErrorIndicator::AddIndicator!");
  const int n = local_.Size();
  if (n)
    hipLaunchKernelGGL(k_indicator_update, dim3((n + 255) / 256), dim3(256), 0, ctx_->stream, local_.Data(), indicator.Data(),
                       n_, n);
  n_ += 1;
}

double ErrorIndicator::Norml2() const { return n_ ? std::sqrt(linalg::Dot(*ctx_, local_, local_)) : 0.0; }

// ---- FluxProjector ---------------------------------------------------------------------------------------------------
namespace {

// the mass form of the smooth space (:117-131): MassIntegrator for a scalar space, VectorFEMassIntegrator else, no coefficient
void add_mass_integrator(BilinearForm &m, bool scalar_flux) {
  if (scalar_flux)
    m.AddDomainIntegrator<MassIntegrator>((const MaterialPropertyCoefficient *)nullptr);
  else
    m.AddDomainIntegrator<VectorFEMassIntegrator>((const MaterialPropertyCoefficient *)nullptr);
}

void require_one_rank(const FiniteElementSpaceHierarchy &fespaces) {
  for (std::size_t l = 0; l < fespaces.GetNumLevels(); l++)
    PA_REQUIRE(!fespaces.GetFESpaceAtLevel(l).GetHalo(),
               "the multigrid (use_mg) flux projector runs on one rank: a level of the smooth space has a halo (use_mg = false "
               "takes spaces with halos)");
  // (the RT / ND p-prolongation between spaces that both carry hanging-node constraints is not built)
  for (std::size_t l = 0; l < fespaces.GetNumLevels(); l++)
    PA_REQUIRE(!fespaces.GetFESpaceAtLevel(l).GetConforming(),
               "the multigrid (use_mg) flux projector does not take a smooth space with hanging-node constraints: pass use_mg = false "
               "(PCG + Jacobi on P^T M P)");
}

// true-dof vector -> L-vector through the hanging-node constraints: lv = P x
void conform_to_lvector(const Context &ctx, const Conforming &c, const Vector &x, Vector &lv) {
  c.Prolongate(x.Data(), lv.Data(), nullptr, ctx.stream);
}

}  // namespace

void FluxAmgSolver::SetOperator(const Operator &op) {
  StreamGraph::Invalidate();
  height = op.Height(), width = op.Width();
  const auto *fop = dynamic_cast<const FespaceParOperator *>(&op);
  const ParOperator *par = fop ? &fop->Par() : dynamic_cast<const ParOperator *>(&op);
  PA_REQUIRE(par && !par->GetHalo(), "the flux projector's AMG needs the ParOperator of a level without a halo");
  AmgOptions opt;
  opt.theta = 0.8;  // errorestimator.cpp:82 ("more coarsening to save memory")
  if (const auto *csr = dynamic_cast<const CsrOperator *>(&par->LocalOperator())) {
    amg_ = std::make_unique<AmgSolver>(*ctx_, DownloadCsr(csr->Matrix()), opt);
    return;
  }
  const auto *pa = dynamic_cast<const ceed::Operator *>(&par->LocalOperator());
  PA_REQUIRE(pa, "the coarse operator is neither assembled nor a partially assembled operator");
  const auto m = BilinearForm::FullAssemble(*pa, /*skip_zeros=*/false);
  amg_ = std::make_unique<AmgSolver>(*ctx_, DownloadCsr(m->Matrix()), opt);
}

void FluxAmgSolver::Mult(const Vector &b, Vector &x) const {
  PA_REQUIRE(amg_, "FluxAmgSolver: SetOperator first");
  amg_->Mult(b, x);  // one cycle from a zero guess
}

FluxProjector::FluxProjector(const MaterialPropertyCoefficient &coeff, const FiniteElementSpace &smooth_fespace,
                             const FiniteElementSpace &rhs_fespace, double tol, int max_it, int print)
    : ctx_(&smooth_fespace.GetContext()), smooth_(&smooth_fespace), rhs_space_(&rhs_fespace) {
  Init(coeff, nullptr, tol, max_it, print);
}

FluxProjector::FluxProjector(const MaterialPropertyCoefficient &coeff, const FiniteElementSpaceHierarchy &smooth_fespaces,
                             const FiniteElementSpace &rhs_fespace, double tol, int max_it, int print, bool use_mg)
    : ctx_(&smooth_fespaces.GetFinestFESpace().GetContext()), smooth_(&smooth_fespaces.GetFinestFESpace()), rhs_space_(&rhs_fespace) {
  Init(coeff, use_mg ? &smooth_fespaces : nullptr, tol, max_it, print);
}

// smooth_fespaces: the hierarchy of the multigrid form, nullptr for use_mg = false
void FluxProjector::Init(const MaterialPropertyCoefficient &coeff, const FiniteElementSpaceHierarchy *smooth_fespaces, double tol,
                         int max_it, int print) {
  const FiniteElementSpace &smooth_fespace = *smooth_, &rhs_fespace = *rhs_space_;
  PhaseRange range("Estimation / Construction");  // errorestimator.cpp:114
  // :117-120: a scalar smooth space (the H1 recovery of the scalar curl of a plane field) takes MassIntegrator
  const bool scalar_flux = smooth_fespace.GetFEType() == PA_FE_H1;
  if (!smooth_fespaces) {  // errorestimator.cpp:125-153 (use_mg = false): the mass matrix of the smooth space, no coefficient
    BilinearForm m(smooth_fespace);
    add_mass_integrator(m, scalar_flux);
    mass_ = m.PartialAssemble();
    M_ = std::make_unique<ParOperator>(*ctx_, *mass_, smooth_fespace.GetTrueVSize(), nullptr, 0,
                                       ParOperator::DiagonalPolicy::DIAG_ONE, smooth_fespace.GetHalo(), smooth_fespace.GetConforming());
  } else {  // :136-147: one mass per level
    require_one_rank(*smooth_fespaces);
    BilinearForm m(smooth_fespace);
    add_mass_integrator(m, scalar_flux);
    auto m_vec = m.Assemble(*smooth_fespaces, /*skip_zeros=*/false);
    M_mg_ = std::make_unique<MultigridOperator>(smooth_fespaces->GetNumLevels());
    for (std::size_t l = 0; l < smooth_fespaces->GetNumLevels(); l++)
      M_mg_->AddOperator(std::make_unique<FespaceParOperator>(std::move(m_vec[l]), smooth_fespaces->GetFESpaceAtLevel(l)));
  }
  {  // :154-176: the flux operator is always partially assembled
    BilinearForm flux(rhs_fespace, smooth_fespace);
    if (scalar_flux)
      flux.AddDomainIntegrator<MassIntegrator>(coeff);
    else
      flux.AddDomainIntegrator<VectorFEMassIntegrator>(coeff);
    flux_ = flux.PartialAssemble();
  }
  // ConfigureLinearSolver (:66-107): the system matrix is real, SPD and diagonally dominant
  pcg_ = std::make_unique<CgSolver>(*ctx_, print);
  pcg_->SetInitialGuess(false);
  pcg_->SetTol(tol);
  pcg_->SetAbsTol(std::numeric_limits<double>::epsilon());
  pcg_->SetMaxIter(max_it);
  if (!smooth_fespaces) {
    pc_ = std::make_unique<JacobiSmoother>(*ctx_);
    pcg_->SetOperator(*M_);
    pc_->SetOperator(*M_);
  } else {
    const ParOperator &finest = M_mg_->GetFinestOperator().Par();  // (what MultigridOperator::Mult applies)
    pcg_->SetOperator(finest);
    auto amg = std::make_unique<FluxAmgSolver>(*ctx_);
    if (smooth_fespaces->GetNumLevels() > 1) {  // :83-91
      const int mg_smooth_order = 2;  // smooth order independent of the order of the space
      auto mg = std::make_unique<GeometricMultigridSolver>(*ctx_, std::move(amg), smooth_fespaces->GetProlongationOperators(), 1, 1,
                                                           mg_smooth_order, 1.0, 0.0, true, nullptr);
      std::vector<const ParOperator *> ops;
      for (std::size_t l = 0; l < M_mg_->GetNumLevels(); l++) ops.push_back(&M_mg_->GetOperatorAtLevel(l).Par());
      mg->SetOperators(ops);
      pc_ = std::move(mg);
    } else {
      amg->SetOperator(finest);
      pc_ = std::move(amg);
    }
  }
  pcg_->SetPreconditioner(*pc_);
  rhs_.SetSize(smooth_fespace.GetTrueVSize());
  if (rhs_fespace.GetHalo() || rhs_fespace.GetConforming()) lx_.SetSize(rhs_fespace.GetVSize());
  if (smooth_fespace.GetHalo() || smooth_fespace.GetConforming()) ly_.SetSize(smooth_fespace.GetVSize());
}

void FluxProjector::Mult(const Vector &x, Vector &y) const {
  PhaseRange range("Estimation / Solve");  // errorestimator.cpp:172
  PA_REQUIRE(x.Size() == rhs_space_->GetTrueVSize() && y.Size() == rhs_.Size(), "Invalid vector dimensions for FluxProjector::Mult!");
  // Flux as a ParOperator between two spaces (rap.cpp:207-220 without essential dofs): P_test^T A P_trial
  // (on a mesh with hanging nodes P is the conforming prolongation of either space: the right-hand side is P_smooth^T Flux P_rhs x,
  // the system matrix P^T M P with the Jacobi diagonal |P|^T diag, rap.cpp:163-175)
  const Halo *hx = rhs_space_->GetHalo(), *hy = smooth_->GetHalo();
  const Conforming *cx = rhs_space_->GetConforming(), *cy = smooth_->GetConforming();
  const Vector *in = &x;
  if (hx) {
    Vector t(lx_.Data(), x.Size());
    linalg::Copy(*ctx_, x, t);
    hx->Prolongate(lx_.Data(), ctx_->stream);
    in = &lx_;
  } else if (cx) {
    conform_to_lvector(*ctx_, *cx, x, lx_);
    in = &lx_;
  }
  if (cy) {
    flux_->Mult(*in, ly_);
    cy->Restrict(ly_.Data(), rhs_.Data(), 0, 1.0, nullptr, nullptr, ctx_->stream);
  } else if (hy) {
    flux_->Mult(*in, ly_);
    hy->RestrictAdd(ly_.Data(), ctx_->stream);
    Vector t(ly_.Data(), rhs_.Size());
    linalg::Copy(*ctx_, t, rhs_);
  } else {
    flux_->Mult(*in, rhs_);
  }
  pcg_->Mult(rhs_, y);
}

// ---- estimators ------------------------------------------------------------------------------------------------------
namespace {

// the error integrator of two dense-table spaces or two tensor spaces on one mesh (both estimator bases)
pa_error_op *make_error_op(const FiniteElementSpace &fespace, const FiniteElementSpace &smooth_fespace, int error_qf,
                           const MaterialTensors &first, const MaterialTensors &second) {
  PA_REQUIRE(fespace.IsDense() == smooth_fespace.IsDense() && &fespace.GetMesh() == &smooth_fespace.GetMesh(),
             "the estimators take two dense-table spaces or two tensor spaces on one mesh");
  PA_REQUIRE(first.dim == second.dim, "the two coefficients of an error integrator have one dimension");
  const auto c1 = first.Coefficient(), c2 = second.Coefficient();
  const auto ctx = ceed::PopulateCoefficientContext(first.dim, &c1, second.dim, &c2);
  const auto r1 = fespace.GetCeedElemRestriction(), r2 = smooth_fespace.GetCeedElemRestriction();
  pa_error_op *op = nullptr;
  if (!fespace.IsDense()) {
    const auto b1 = fespace.GetCeedBasis(), b2 = smooth_fespace.GetCeedBasis();
    check(pa_error_op_create_tensor(fespace.GetMesh().GetCeedGeomFactorData(), &r1, &b1, &r2, &b2, error_qf, ctx.data(),
                                    ctx.size() * sizeof(double), &op));
  } else {
    const auto b1 = fespace.GetCeedDenseBasis(), b2 = smooth_fespace.GetCeedDenseBasis();
    check(pa_error_op_create(fespace.GetMesh().GetCeedGeomFactorData(), &r1, &b1, &r2, &b2, error_qf, ctx.data(),
                             ctx.size() * sizeof(double), &op));
  }
  return op;
}

}  // namespace

FluxErrorEstimatorBase::FluxErrorEstimatorBase(const FiniteElementSpace &fespace, const FiniteElementSpace &smooth_fespace,
                                               const MaterialPropertyCoefficient &flux_coeff, int error_qf,
                                               const MaterialTensors &first, const MaterialTensors &second, double tol,
                                               int max_it, int print)
    : ctx_(&fespace.GetContext()), fespace_(fespace), smooth_fespace_(smooth_fespace),
      projector_(flux_coeff, smooth_fespace, fespace, tol, max_it, print), G_(smooth_fespace.GetTrueVSize()) {
  PA_REQUIRE(fespace.IsDense() == smooth_fespace.IsDense() && &fespace.GetMesh() == &smooth_fespace.GetMesh(),
             "the estimators take two dense-table spaces or two tensor spaces on one mesh");
  const auto c1 = first.Coefficient(), c2 = second.Coefficient();
  PA_REQUIRE(first.dim == second.dim, "the two coefficients of an error integrator have one dimension");
  const auto ctx = ceed::PopulateCoefficientContext(first.dim, &c1, second.dim, &c2);  // errorestimator.cpp:326-329, :459-460
  const auto r1 = fespace.GetCeedElemRestriction(), r2 = smooth_fespace.GetCeedElemRestriction();
  if (!fespace.IsDense()) {  // tensor-product hexahedra: the sum-factorised error integrator (pa_mixed_hex.hip)
    const auto b1 = fespace.GetCeedBasis(), b2 = smooth_fespace.GetCeedBasis();
    check(pa_error_op_create_tensor(fespace.GetMesh().GetCeedGeomFactorData(), &r1, &b1, &r2, &b2, error_qf, ctx.data(),
                                    ctx.size() * sizeof(double), &integ_op_));
    return;
  }
  const auto b1 = fespace.GetCeedDenseBasis(), b2 = smooth_fespace.GetCeedDenseBasis();
  check(pa_error_op_create(fespace.GetMesh().GetCeedGeomFactorData(), &r1, &b1, &r2, &b2, error_qf, ctx.data(),
                           ctx.size() * sizeof(double), &integ_op_));
}

FluxErrorEstimatorBase::FluxErrorEstimatorBase(const FiniteElementSpace &fespace, const FiniteElementSpaceHierarchy &smooth_fespaces,
                                               const MaterialPropertyCoefficient &flux_coeff, int error_qf,
                                               const MaterialTensors &first, const MaterialTensors &second, double tol,
                                               int max_it, int print, bool use_mg)
    : ctx_(&fespace.GetContext()), fespace_(fespace), smooth_fespace_(smooth_fespaces.GetFinestFESpace()),
      projector_(flux_coeff, smooth_fespaces, fespace, tol, max_it, print, use_mg), G_(smooth_fespace_.GetTrueVSize()) {
  integ_op_ = make_error_op(fespace, smooth_fespace_, error_qf, first, second);
}

FluxErrorEstimatorBase::~FluxErrorEstimatorBase() { pa_error_op_destroy(integ_op_); }

void FluxErrorEstimatorBase::AddErrorEstimates(const Vector &F, Vector &estimates) const {
  PA_REQUIRE(F.Size() == fespace_.GetTrueVSize() && estimates.Size() == fespace_.GetMesh().GetNE(),
             "Invalid vector dimensions for the error estimate!");
  projector_.Mult(F, G_);
  // grid functions = L-vectors (GetProlongationMatrix()->Mult, :202-214): ghosts filled through the halos
  // ... or, on a mesh with hanging nodes, the constrained dofs through the conforming prolongation
  const Halo *hf = fespace_.GetHalo(), *hg = smooth_fespace_.GetHalo();
  const Conforming *cf = fespace_.GetConforming(), *cg = smooth_fespace_.GetConforming();
  Vector F_gf, G_gf;
  const double *pf = F.Data(), *pg = G_.Data();
  if (hf) {
    F_gf.SetSize(fespace_.GetVSize());
    Vector t(F_gf.Data(), F.Size());
    linalg::Copy(*ctx_, F, t);
    hf->Prolongate(F_gf.Data(), ctx_->stream);
    pf = F_gf.Data();
  } else if (cf) {
    F_gf.SetSize(fespace_.GetVSize());
    conform_to_lvector(*ctx_, *cf, F, F_gf);
    pf = F_gf.Data();
  }
  if (hg) {
    G_gf.SetSize(smooth_fespace_.GetVSize());
    Vector t(G_gf.Data(), G_.Size());
    linalg::Copy(*ctx_, G_, t);
    hg->Prolongate(G_gf.Data(), ctx_->stream);
    pg = G_gf.Data();
  } else if (cg) {
    G_gf.SetSize(smooth_fespace_.GetVSize());
    conform_to_lvector(*ctx_, *cg, G_, G_gf);
    pg = G_gf.Data();
  }
  check(pa_error_op_apply_add(integ_op_, pf, pg, estimates.Data(), ctx_->stream));
  if (hf || hg || cf || cg) PA_HIP(hipStreamSynchronize(ctx_->stream));  // the temporaries go out of scope
}

void FluxErrorEstimatorBase::AddErrorIndicator(const Vector &F, double Et, ErrorIndicator &indicator) const {
  PhaseRange range("Estimation");  // errorestimator.cpp:192
  Vector estimates(fespace_.GetMesh().GetNE());
  linalg::Fill(*ctx_, estimates, 0.0);
  AddErrorEstimates(F, estimates);
  linalg::Sqrt(*ctx_, estimates, (Et > 0.0) ? 0.5 / Et : 1.0);  // Correct factor of 1/2 in energy
  indicator.AddIndicator(estimates);
}

GradFluxErrorEstimator::GradFluxErrorEstimator(const MaterialTensors &epsilon, const FiniteElementSpace &nd_fespace,
                                               const FiniteElementSpace &rt_fespace, double tol, int max_it, int print)
    : FluxErrorEstimatorBase(nd_fespace, rt_fespace, epsilon.Coefficient(),
                             nd_fespace.GetMesh().Dimension() == 2 ? PA_QF_HCURLHDIV_ERROR_22 : PA_QF_HCURLHDIV_ERROR_33,  // :343-356
                             epsilon.Map([](const double *m) { return linalg::MatrixSqrt(m); }),
                             epsilon.Map([](const double *m) { return linalg::MatrixPow(m, -0.5); }), tol, max_it, print) {}

CurlFluxErrorEstimator::CurlFluxErrorEstimator(const MaterialTensors &muinv, const FiniteElementSpace &rt_fespace,
                                               const FiniteElementSpace &nd_fespace, double tol, int max_it, int print)
    : FluxErrorEstimatorBase(rt_fespace, nd_fespace, muinv.Coefficient(),
                             rt_fespace.GetMesh().Dimension() == 2 ? PA_QF_L2H1_ERROR : PA_QF_HDIVHCURL_ERROR_33,  // :464-480
                             muinv.Map([](const double *m) { return linalg::MatrixSqrt(m); }),
                             muinv.Map([](const double *m) { return linalg::MatrixPow(m, -0.5); }), tol, max_it, print) {}

GradFluxErrorEstimator::GradFluxErrorEstimator(const MaterialTensors &epsilon, const FiniteElementSpace &nd_fespace,
                                               const FiniteElementSpaceHierarchy &rt_fespaces, double tol, int max_it, int print,
                                               bool use_mg)
    : FluxErrorEstimatorBase(nd_fespace, rt_fespaces, epsilon.Coefficient(),
                             nd_fespace.GetMesh().Dimension() == 2 ? PA_QF_HCURLHDIV_ERROR_22 : PA_QF_HCURLHDIV_ERROR_33,
                             epsilon.Map([](const double *m) { return linalg::MatrixSqrt(m); }),
                             epsilon.Map([](const double *m) { return linalg::MatrixPow(m, -0.5); }), tol, max_it, print, use_mg) {}

CurlFluxErrorEstimator::CurlFluxErrorEstimator(const MaterialTensors &muinv, const FiniteElementSpace &rt_fespace,
                                               const FiniteElementSpaceHierarchy &nd_fespaces, double tol, int max_it, int print,
                                               bool use_mg)
    : FluxErrorEstimatorBase(rt_fespace, nd_fespaces, muinv.Coefficient(),
                             rt_fespace.GetMesh().Dimension() == 2 ? PA_QF_L2H1_ERROR : PA_QF_HDIVHCURL_ERROR_33,
                             muinv.Map([](const double *m) { return linalg::MatrixSqrt(m); }),
                             muinv.Map([](const double *m) { return linalg::MatrixPow(m, -0.5); }), tol, max_it, print, use_mg) {}

// ---- the same for a ComplexVector -------------------------------------------------------------------------------------
namespace {

// true-dof vector -> L-vector through the halo: lv[0, n) = x, ghosts filled
void to_lvector(const Context &ctx, const Halo &h, const Vector &x, Vector &lv) {
  Vector t(lv.Data(), x.Size());
  linalg::Copy(ctx, x, t);
  h.Prolongate(lv.Data(), ctx.stream);
}

}  // namespace

ComplexFluxProjector::ComplexFluxProjector(const MaterialPropertyCoefficient &coeff, const FiniteElementSpace &smooth_fespace,
                                           const FiniteElementSpace &rhs_fespace, double tol, int max_it, int print)
    : ctx_(&smooth_fespace.GetContext()), smooth_(&smooth_fespace), rhs_space_(&rhs_fespace) {
  Init(coeff, nullptr, tol, max_it, print);
}

ComplexFluxProjector::ComplexFluxProjector(const MaterialPropertyCoefficient &coeff, const FiniteElementSpaceHierarchy &smooth_fespaces,
                                           const FiniteElementSpace &rhs_fespace, double tol, int max_it, int print, bool use_mg)
    : ctx_(&smooth_fespaces.GetFinestFESpace().GetContext()), smooth_(&smooth_fespaces.GetFinestFESpace()), rhs_space_(&rhs_fespace) {
  Init(coeff, use_mg ? &smooth_fespaces : nullptr, tol, max_it, print);
}

void ComplexFluxProjector::Init(const MaterialPropertyCoefficient &coeff, const FiniteElementSpaceHierarchy *smooth_fespaces, double tol,
                                int max_it, int print) {
  const FiniteElementSpace &smooth_fespace = *smooth_, &rhs_fespace = *rhs_space_;
  PhaseRange range("Estimation / Construction");
  const bool scalar_flux = smooth_fespace.GetFEType() == PA_FE_H1;
  const ceed::Operator *finest_mass = nullptr;
  const ComplexParOperator *finest_M = nullptr;
  if (!smooth_fespaces) {
    BilinearForm m(smooth_fespace);
    add_mass_integrator(m, scalar_flux);
    mass_ = m.PartialAssemble();
    // BuildLevelParOperator<ComplexOperator> (:50-65): the real mass matrix as the real part, no imaginary part
    M_ = std::make_unique<ComplexParOperator>(*ctx_, mass_.get(), nullptr, smooth_fespace.GetTrueVSize(), smooth_fespace.GetHalo(),
                                              smooth_fespace.GetConforming());
    finest_mass = mass_.get(), finest_M = M_.get();
  } else {  // :136-147
    require_one_rank(*smooth_fespaces);
    BilinearForm m(smooth_fespace);
    add_mass_integrator(m, scalar_flux);
    level_mass_ = m.Assemble(*smooth_fespaces, /*skip_zeros=*/false);
    for (std::size_t l = 0; l < smooth_fespaces->GetNumLevels(); l++)
      level_M_.push_back(std::make_unique<ComplexParOperator>(*ctx_, level_mass_[l].get(), nullptr,
                                                              smooth_fespaces->GetFESpaceAtLevel(l).GetTrueVSize(), nullptr));
    finest_mass = dynamic_cast<const ceed::Operator *>(level_mass_.back().get());
    PA_REQUIRE(finest_mass, "the finest level of the flux projector's hierarchy is partially assembled");
    finest_M = level_M_.back().get();
  }
  {
    BilinearForm flux(rhs_fespace, smooth_fespace);
    if (scalar_flux)
      flux.AddDomainIntegrator<MassIntegrator>(coeff);
    else
      flux.AddDomainIntegrator<VectorFEMassIntegrator>(coeff);
    flux_ = flux.PartialAssemble();
  }
  pcg_ = std::make_unique<ComplexCgSolver>(*ctx_, print);
  pcg_->SetTol(tol);
  pcg_->SetAbsTol(std::numeric_limits<double>::epsilon());
  pcg_->SetMaxIter(max_it);
  Mboth_ = std::make_unique<ComplexMassOperator>(*ctx_, *finest_mass, *finest_M, smooth_fespace.GetHalo() != nullptr,
                                                 smooth_fespaces ? nullptr : smooth_fespace.GetConforming());
  pcg_->SetOperator(*Mboth_);
  if (!smooth_fespaces) {
    pc_ = std::make_unique<ComplexJacobiSmoother>(*ctx_);
    pc_->SetOperator(*M_);
  } else {
    amg_ = std::make_unique<FluxAmgSolver>(*ctx_);
    auto coarse = std::make_unique<ComplexWrapperSolver>(*amg_);
    if (smooth_fespaces->GetNumLevels() > 1) {
      auto mg = std::make_unique<ComplexGeometricMultigridSolver>(*ctx_, std::move(coarse), smooth_fespaces->GetProlongationOperators(),
                                                                  1, 1, /*mg_smooth_order=*/2, 1.0, 0.0, true, nullptr);
      std::vector<const ComplexParOperator *> ops;
      for (const auto &M : level_M_) ops.push_back(M.get());
      mg->SetOperators(ops);
      pc_ = std::move(mg);
    } else {
      coarse->SetOperator(*finest_M);
      pc_ = std::move(coarse);
    }
  }
  pcg_->SetPreconditioner(*pc_);
  rhs_.SetSize(smooth_fespace.GetTrueVSize());
  if (rhs_fespace.GetHalo() || rhs_fespace.GetConforming()) lx_.SetSize(rhs_fespace.GetVSize());
  if (smooth_fespace.GetHalo() || smooth_fespace.GetConforming()) ly_.SetSize(smooth_fespace.GetVSize());
}

bool ComplexFluxProjector::FluxTwoRhs() const { return pa_op_two_rhs(flux_->Handle()) != 0; }

ComplexMassOperator::ComplexMassOperator(const Context &ctx, const ceed::Operator &mass, const ComplexParOperator &par, bool has_halo,
                                         const Conforming *conf)
    : ComplexOperator(par.Height(), par.Width()), ctx_(&ctx), mass_(&mass), par_(&par), has_halo_(has_halo), conf_(conf) {
  PA_REQUIRE(!conf || (conf->NumTrue() == par.Height() && conf->NumLocal() == mass.Height()),
             "the conforming prolongation does not match the mass operator");
  if (conf) lx_.SetSize(conf->NumLocal()), ly_.SetSize(conf->NumLocal());
}

// (with a streaming form two separate applies are the faster choice, as in ParOperator::Mult2)
bool ComplexMassOperator::OnePass() const { return !has_halo_ && pa_op_two_rhs(mass_->Handle()) != 0 && !mass_->Streams(); }

void ComplexMassOperator::Mult(const ComplexVector &x, ComplexVector &y) const {
  if (!OnePass()) return par_->Mult(x, y);
  if (conf_) {  // P^T M P on both parts: three launches where the two real ParOperators take six
    conf_->Prolongate2(x.Real().Data(), x.Imag().Data(), lx_.Real().Data(), lx_.Imag().Data(), nullptr, ctx_->stream);
    mass_->Mult2(lx_.Real(), lx_.Imag(), ly_.Real(), ly_.Imag());
    conf_->Restrict2(ly_.Real().Data(), ly_.Imag().Data(), y.Real().Data(), y.Imag().Data(), 0, 1.0, nullptr, nullptr, nullptr,
                     ctx_->stream);
  } else {
    mass_->Mult2(x.Real(), x.Imag(), y.Real(), y.Imag());  // no essential dofs, no imaginary part: yr = M xr, yi = M xi
  }
  one_pass_applies_++;
}

void ComplexFluxProjector::Mult(const ComplexVector &x, ComplexVector &y) const {
  PhaseRange range("Estimation / Solve");
  PA_REQUIRE(x.Size() == rhs_space_->GetTrueVSize() && y.Size() == rhs_.Size(),
             "Invalid vector dimensions for ComplexFluxProjector::Mult!");
  const Halo *hx = rhs_space_->GetHalo(), *hy = smooth_->GetHalo();
  const Conforming *cx = rhs_space_->GetConforming(), *cy = smooth_->GetConforming();
  const Vector *in_r = &x.Real(), *in_i = &x.Imag();
  if (hx) {
    to_lvector(*ctx_, *hx, x.Real(), lx_.Real());
    to_lvector(*ctx_, *hx, x.Imag(), lx_.Imag());
    in_r = &lx_.Real(), in_i = &lx_.Imag();
  } else if (cx) {  // both parts through P in one launch
    cx->Prolongate2(x.Real().Data(), x.Imag().Data(), lx_.Real().Data(), lx_.Imag().Data(), nullptr, ctx_->stream);
    in_r = &lx_.Real(), in_i = &lx_.Imag();
  }
  if (cy) {  // P_smooth^T Flux P_rhs x
    flux_->Mult2(*in_r, *in_i, ly_.Real(), ly_.Imag());
    cy->Restrict2(ly_.Real().Data(), ly_.Imag().Data(), rhs_.Real().Data(), rhs_.Imag().Data(), 0, 1.0, nullptr, nullptr, nullptr,
                  ctx_->stream);
  } else if (hy) {
    flux_->Mult2(*in_r, *in_i, ly_.Real(), ly_.Imag());
    for (Vector *part : {&ly_.Real(), &ly_.Imag()}) hy->RestrictAdd(part->Data(), ctx_->stream);
    Vector tr(ly_.Real().Data(), rhs_.Size()), ti(ly_.Imag().Data(), rhs_.Size());
    linalg::Copy(*ctx_, tr, rhs_.Real());
    linalg::Copy(*ctx_, ti, rhs_.Imag());
  } else {
    flux_->Mult2(*in_r, *in_i, rhs_.Real(), rhs_.Imag());
  }
  pcg_->Mult(rhs_, y, false);
}

ComplexFluxErrorEstimatorBase::ComplexFluxErrorEstimatorBase(const FiniteElementSpace &fespace,
                                                             const FiniteElementSpace &smooth_fespace,
                                                             const MaterialPropertyCoefficient &flux_coeff, int error_qf,
                                                             const MaterialTensors &first, const MaterialTensors &second,
                                                             double tol, int max_it, int print)
    : ctx_(&fespace.GetContext()), fespace_(fespace), smooth_fespace_(smooth_fespace),
      projector_(flux_coeff, smooth_fespace, fespace, tol, max_it, print) {
  G_.SetSize(smooth_fespace.GetTrueVSize());
  integ_op_ = make_error_op(fespace, smooth_fespace, error_qf, first, second);
}

ComplexFluxErrorEstimatorBase::ComplexFluxErrorEstimatorBase(const FiniteElementSpace &fespace,
                                                             const FiniteElementSpaceHierarchy &smooth_fespaces,
                                                             const MaterialPropertyCoefficient &flux_coeff, int error_qf,
                                                             const MaterialTensors &first, const MaterialTensors &second,
                                                             double tol, int max_it, int print, bool use_mg)
    : ctx_(&fespace.GetContext()), fespace_(fespace), smooth_fespace_(smooth_fespaces.GetFinestFESpace()),
      projector_(flux_coeff, smooth_fespaces, fespace, tol, max_it, print, use_mg) {
  G_.SetSize(smooth_fespace_.GetTrueVSize());
  integ_op_ = make_error_op(fespace, smooth_fespace_, error_qf, first, second);
}

ComplexFluxErrorEstimatorBase::~ComplexFluxErrorEstimatorBase() { pa_error_op_destroy(integ_op_); }

void ComplexFluxErrorEstimatorBase::AddErrorEstimates(const ComplexVector &F, Vector &estimates) const {
  PA_REQUIRE(F.Size() == fespace_.GetTrueVSize() && estimates.Size() == fespace_.GetMesh().GetNE(),
             "Invalid vector dimensions for the error estimate!");
  projector_.Mult(F, G_);
  // both parts of F and G as L-vectors (:202-214), then one error integrator call for the two parts (:249-261)
  const Halo *hf = fespace_.GetHalo(), *hg = smooth_fespace_.GetHalo();
  const Conforming *cf = fespace_.GetConforming(), *cg = smooth_fespace_.GetConforming();
  ComplexVector F_gf, G_gf;
  const double *pf[2] = {F.Real().Data(), F.Imag().Data()}, *pg[2] = {G_.Real().Data(), G_.Imag().Data()};
  if (hf) {
    F_gf.SetSize(fespace_.GetVSize());
    to_lvector(*ctx_, *hf, F.Real(), F_gf.Real());
    to_lvector(*ctx_, *hf, F.Imag(), F_gf.Imag());
    pf[0] = F_gf.Real().Data(), pf[1] = F_gf.Imag().Data();
  } else if (cf) {
    F_gf.SetSize(fespace_.GetVSize());
    cf->Prolongate2(pf[0], pf[1], F_gf.Real().Data(), F_gf.Imag().Data(), nullptr, ctx_->stream);
    pf[0] = F_gf.Real().Data(), pf[1] = F_gf.Imag().Data();
  }
  if (hg) {
    G_gf.SetSize(smooth_fespace_.GetVSize());
    to_lvector(*ctx_, *hg, G_.Real(), G_gf.Real());
    to_lvector(*ctx_, *hg, G_.Imag(), G_gf.Imag());
    pg[0] = G_gf.Real().Data(), pg[1] = G_gf.Imag().Data();
  } else if (cg) {
    G_gf.SetSize(smooth_fespace_.GetVSize());
    cg->Prolongate2(pg[0], pg[1], G_gf.Real().Data(), G_gf.Imag().Data(), nullptr, ctx_->stream);
    pg[0] = G_gf.Real().Data(), pg[1] = G_gf.Imag().Data();
  }
  check(pa_error_op_apply_add2(integ_op_, pf[0], pg[0], pf[1], pg[1], estimates.Data(), ctx_->stream));
  if (hf || hg || cf || cg) PA_HIP(hipStreamSynchronize(ctx_->stream));  // the temporaries go out of scope
}

void ComplexFluxErrorEstimatorBase::AddErrorIndicator(const ComplexVector &F, double Et, ErrorIndicator &indicator) const {
  PhaseRange range("Estimation");
  Vector estimates(fespace_.GetMesh().GetNE());
  linalg::Fill(*ctx_, estimates, 0.0);
  AddErrorEstimates(F, estimates);
  linalg::Sqrt(*ctx_, estimates, (Et > 0.0) ? 0.5 / Et : 1.0);  // Correct factor of 1/2 in energy
  indicator.AddIndicator(estimates);
}

ComplexGradFluxErrorEstimator::ComplexGradFluxErrorEstimator(const MaterialTensors &epsilon, const FiniteElementSpace &nd_fespace,
                                                             const FiniteElementSpace &rt_fespace, double tol, int max_it,
                                                             int print)
    : ComplexFluxErrorEstimatorBase(nd_fespace, rt_fespace, epsilon.Coefficient(),
                                    nd_fespace.GetMesh().Dimension() == 2 ? PA_QF_HCURLHDIV_ERROR_22 : PA_QF_HCURLHDIV_ERROR_33,
                                    epsilon.Map([](const double *m) { return linalg::MatrixSqrt(m); }),
                                    epsilon.Map([](const double *m) { return linalg::MatrixPow(m, -0.5); }), tol, max_it, print) {}

ComplexCurlFluxErrorEstimator::ComplexCurlFluxErrorEstimator(const MaterialTensors &muinv, const FiniteElementSpace &rt_fespace,
                                                             const FiniteElementSpace &nd_fespace, double tol, int max_it,
                                                             int print)
    : ComplexFluxErrorEstimatorBase(rt_fespace, nd_fespace, muinv.Coefficient(),
                                    rt_fespace.GetMesh().Dimension() == 2 ? PA_QF_L2H1_ERROR : PA_QF_HDIVHCURL_ERROR_33,
                                    muinv.Map([](const double *m) { return linalg::MatrixSqrt(m); }),
                                    muinv.Map([](const double *m) { return linalg::MatrixPow(m, -0.5); }), tol, max_it, print) {}

ComplexGradFluxErrorEstimator::ComplexGradFluxErrorEstimator(const MaterialTensors &epsilon, const FiniteElementSpace &nd_fespace,
                                                             const FiniteElementSpaceHierarchy &rt_fespaces, double tol, int max_it,
                                                             int print, bool use_mg)
    : ComplexFluxErrorEstimatorBase(nd_fespace, rt_fespaces, epsilon.Coefficient(),
                                    nd_fespace.GetMesh().Dimension() == 2 ? PA_QF_HCURLHDIV_ERROR_22 : PA_QF_HCURLHDIV_ERROR_33,
                                    epsilon.Map([](const double *m) { return linalg::MatrixSqrt(m); }),
                                    epsilon.Map([](const double *m) { return linalg::MatrixPow(m, -0.5); }), tol, max_it, print,
                                    use_mg) {}

ComplexCurlFluxErrorEstimator::ComplexCurlFluxErrorEstimator(const MaterialTensors &muinv, const FiniteElementSpace &rt_fespace,
                                                             const FiniteElementSpaceHierarchy &nd_fespaces, double tol, int max_it,
                                                             int print, bool use_mg)
    : ComplexFluxErrorEstimatorBase(rt_fespace, nd_fespaces, muinv.Coefficient(),
                                    rt_fespace.GetMesh().Dimension() == 2 ? PA_QF_L2H1_ERROR : PA_QF_HDIVHCURL_ERROR_33,
                                    muinv.Map([](const double *m) { return linalg::MatrixSqrt(m); }),
                                    muinv.Map([](const double *m) { return linalg::MatrixPow(m, -0.5); }), tol, max_it, print,
                                    use_mg) {}

TimeDependentFluxErrorEstimator::TimeDependentFluxErrorEstimator(const MaterialTensors &epsilon, const MaterialTensors &muinv,
                                                                 const FiniteElementSpaceHierarchy &nd_fespaces,
                                                                 const FiniteElementSpaceHierarchy &rt_fespaces, double tol,
                                                                 int max_it, int print, bool use_mg)
    : ctx_(&nd_fespaces.GetFinestFESpace().GetContext()),
      grad_(epsilon, nd_fespaces.GetFinestFESpace(), rt_fespaces, tol, max_it, print, use_mg),
      curl_(muinv, rt_fespaces.GetFinestFESpace(), nd_fespaces, tol, max_it, print, use_mg) {}

TimeDependentFluxErrorEstimator::TimeDependentFluxErrorEstimator(const MaterialTensors &epsilon, const MaterialTensors &muinv,
                                                                 const FiniteElementSpace &nd_fespace,
                                                                 const FiniteElementSpace &rt_fespace, double tol,
                                                                 int max_it, int print)
    : ctx_(&nd_fespace.GetContext()), grad_(epsilon, nd_fespace, rt_fespace, tol, max_it, print),
      curl_(muinv, rt_fespace, nd_fespace, tol, max_it, print) {}

void TimeDependentFluxErrorEstimator::AddErrorIndicator(const Vector &E, const Vector &B, double Et,
                                                        ErrorIndicator &indicator) const {
  Vector estimates(grad_.NumElements());
  linalg::Fill(*ctx_, estimates, 0.0);
  grad_.AddErrorEstimates(E, estimates);
  curl_.AddErrorEstimates(B, estimates);  // grad_estimates += curl_estimates (:536)
  linalg::Sqrt(*ctx_, estimates, (Et > 0.0) ? 0.5 / Et : 1.0);  // Correct factor of 1/2 in energy
  indicator.AddIndicator(estimates);
}

}  // namespace palace
