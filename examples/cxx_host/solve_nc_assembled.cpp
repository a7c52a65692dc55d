// C++ host example on a mesh with hanging nodes with an ASSEMBLED coarsest level: the problem of solve_nc.cpp with
// BilinearForm::pa_order_threshold = 2, so that level 0 (order 1) is a matrix -- the reference's PartialAssemblyOrder route --
// and the algebraic coarse solvers get P^T A P through the device triple product (pa_rap_conform.hip):
//   amg   H1 diffusion + mass,  PCG + p-multigrid, LinearSolver::BOOMER_AMG at level 0
//   ams   ND curl-curl + mass,  PCG + p-multigrid, LinearSolver::AMS at level 0 (the true-dof gradient R_nd G_local P_h1 of the
//         constrained lowest-order pair, the true-vertex coordinates)
// It reads the blob of dump_nc_problem.py (mesh, Nedelec spaces) and that of dump_nc_h1_problem.py (H1 spaces) and prints the line
// of solve_nc.cpp.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -I<repo>/palace_amd/csrc -I<repo>/include solve_nc_assembled.cpp -L<repo>/palace_amd/lib
//         -lpalace_amd -Wl,-rpath,<repo>/palace_amd/lib -o solve_nc_assembled
//   ./solve_nc_assembled problem.bin h1.bin amg|ams
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "ksp.hpp"

using namespace palace;

static std::vector<std::vector<char>> read_blobs(const char *path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", path);
    std::exit(2);
  }
  int64_t n = 0;
  f.read(reinterpret_cast<char *>(&n), 8);
  std::vector<std::vector<char>> out((size_t)n);
  for (auto &b : out) {
    int64_t bytes = 0;
    f.read(reinterpret_cast<char *>(&bytes), 8);
    b.resize((size_t)bytes);
    f.read(b.data(), bytes);
  }
  return out;
}

int main(int argc, char **argv) {
  if (argc < 4) return 2;
  const std::string coarse = argv[3];
  if (coarse != "amg" && coarse != "ams") return 2;
  try {
    auto blobs = read_blobs(argv[1]), hblobs = read_blobs(argv[2]);
    auto i32 = [&](size_t i) { return reinterpret_cast<const int32_t *>(blobs[i].data()); };
    auto f64 = [&](size_t i) { return reinterpret_cast<const double *>(blobs[i].data()); };
    auto h32 = [&](size_t i) { return reinterpret_cast<const int32_t *>(hblobs[i].data()); };
    const int ne = i32(0)[0], nn = i32(0)[1], order = i32(0)[2], nlev = i32(0)[3];
    if (h32(0)[0] != order || h32(0)[1] != nlev) throw pa::Error("the two files describe different hierarchies");

    hipStream_t stream;
    if (hipStreamCreate(&stream) != hipSuccess) throw pa::Error("no HIP device");
    Context ctx;
    ctx.stream = stream;

    fem::DefaultIntegrationOrder::p_trial = order;
    Mesh mesh(ctx, ne, 2, nn, i32(1), f64(2), i32(3), fem::DefaultIntegrationOrder::GetQ1d(2 * 3 - 1));

    FiniteElementSpaceHierarchy nd_fespaces, h1_fespaces;
    for (int l = 0; l < nlev; l++) {
      const size_t b = 4 + 8 * (size_t)l, h = 1 + 6 * (size_t)l;
      const int p = i32(0)[4 + l];
      auto nd = std::make_unique<FiniteElementSpace>(ctx, mesh, PA_FE_HCURL, p, i32(b)[0], i32(b + 1),
                                                     reinterpret_cast<const uint8_t *>(blobs[b + 2].data()), i32(b + 3));
      nd->SetConformingProlongation(i32(b)[1], reinterpret_cast<const int *>(blobs[b + 5].data()), i32(b + 6), f64(b + 7));
      nd->SetEssentialTrueDofs(i32(b + 4), (int)(blobs[b + 4].size() / 4));
      nd_fespaces.AddLevel(std::move(nd));
      auto h1 = std::make_unique<FiniteElementSpace>(ctx, mesh, PA_FE_H1, p, h32(h)[0], h32(h + 1), nullptr, nullptr);
      h1->SetConformingProlongation(h32(h)[1], reinterpret_cast<const int *>(hblobs[h + 3].data()), h32(h + 4),
                                    reinterpret_cast<const double *>(hblobs[h + 5].data()));
      h1->SetEssentialTrueDofs(h32(h + 2), (int)(hblobs[h + 2].size() / 4));
      h1_fespaces.AddLevel(std::move(h1));
    }
    const bool amg = coarse == "amg";
    const FiniteElementSpaceHierarchy &fespaces = amg ? h1_fespaces : nd_fespaces;

    MaterialPropertyCoefficient muinv(1), eps(1);
    muinv.AddMaterialProperty(1, 1.0);
    eps.AddMaterialProperty(1, 2.08);

    BilinearForm::pa_order_threshold = 2;  // the order-1 level becomes a matrix: the algebraic solvers get its P^T A P
    BilinearForm a(fespaces.GetFinestFESpace());
    if (amg)
      a.AddDomainIntegrator<DiffusionMassIntegrator>(muinv, eps);
    else
      a.AddDomainIntegrator<CurlCurlMassIntegrator>(muinv, eps);
    auto a_ops = a.Assemble(fespaces, /*skip_zeros=*/false);
    auto A = std::make_unique<MultigridOperator>(fespaces.GetNumLevels());
    for (std::size_t l = 0; l < fespaces.GetNumLevels(); l++) {
      const auto &fes = fespaces.GetFESpaceAtLevel(l);
      auto op = std::make_unique<FespaceParOperator>(std::move(a_ops[l]), fes);
      op->SetEssentialTrueDofs(fes.GetEssentialTrueDofs(), ParOperator::DiagonalPolicy::DIAG_ONE);
      A->AddOperator(std::move(op));
    }

    config::LinearSolverData linear;
    linear.krylov_solver = KrylovSolver::CG;
    linear.type = amg ? LinearSolver::BOOMER_AMG : LinearSolver::AMS;
    linear.tol = 1e-10, linear.max_it = 400;
    linear.mg_smooth_aux = 0;
    linear.initial_guess = 0;
    linear.SetDefaults(order, /*spd_problem=*/true);
    KspSolver ksp(linear, /*verbose=*/0, fespaces, amg ? nullptr : &h1_fespaces);
    ksp.SetOperators(*A, *A);

    const int n = A->Height();
    const int constrained = fespaces.GetFinestFESpace().GetVSize() - fespaces.GetFinestFESpace().GetTrueVSize();
    Vector ones(n), rhs(n), x(n), res(n);
    linalg::Fill(ctx, ones, 1.0);
    A->Mult(ones, rhs);
    const auto &ess = A->GetFinestOperator().Par();
    linalg::SetSubVector(ctx, rhs, ess.GetEssentialTrueDofs(), ess.NumEssentialTrueDofs(), 0.0);
    ksp.Mult(rhs, x);
    A->Mult(x, res);
    linalg::AXPBY(ctx, 1.0, rhs, -1.0, res);
    std::printf("cxx_host_nc: order %d  levels %d  ndofs %d  constrained %d  coarse %s  iterations %d  converged %d  "
                "|b - A x| / |b| %.3e  sum(x) %.12e\n",
                order, nlev, n, constrained, coarse.c_str(), ksp.GetKrylovSolver().GetNumIterations(),
                (int)ksp.GetKrylovSolver().GetConverged(), linalg::Norml2(ctx, res) / linalg::Norml2(ctx, rhs),
                linalg::Dot(ctx, x, ones));
  } catch (const std::exception &e) {
    std::fprintf(stderr, "palace_amd: %s\n", e.what());  // MFEM_ABORT in Palace
    return 1;
  }
  return 0;
}
