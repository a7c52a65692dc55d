// C++ host example on a mesh with hanging nodes: the driver of solve.cpp after one nonconformal refinement step (the
// reference refines tensor elements only this way, utils/geodata.cpp:174-186).  From the arrays MFEM would provide (leaf
// elements, element -> dof tables per level in the true-dofs-first layout, the constraint matrix of the conforming
// prolongation; see dump_nc_problem.py) it builds
//   Mesh, FiniteElementSpaceHierarchy (p = 1 .. order), every space carrying its constraint (SetConformingProlongation),
//   BilinearForm + CurlCurlMassIntegrator -> Assemble(hierarchy): every level's ParOperator is P^T A P,
//   MultigridOperator, KspSolver (PCG + p-multigrid, Chebyshev smoothers; the transfers are R_f I P_c),
// solves (K + eps_r M) x = b and prints what solve.cpp prints.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -I<repo>/palace_amd/csrc -I<repo>/include solve_nc.cpp -L<repo>/palace_amd/lib
//         -lpalace_amd -Wl,-rpath,<repo>/palace_amd/lib -o solve_nc
//   ./solve_nc problem.bin [coarse=pcg|cheb|jacobi|amg]
// coarse = amg (LinearSolver::BOOMER_AMG) is refused on a constrained level 0: it needs the assembled P^T A P, which is not built.
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
  if (argc < 2) return 2;
  const std::string coarse = argc > 2 ? argv[2] : "pcg";
  try {
    auto blobs = read_blobs(argv[1]);
    auto i32 = [&](size_t i) { return reinterpret_cast<const int32_t *>(blobs[i].data()); };
    auto f64 = [&](size_t i) { return reinterpret_cast<const double *>(blobs[i].data()); };
    const int ne = i32(0)[0], nn = i32(0)[1], order = i32(0)[2], nlev = i32(0)[3];

    hipStream_t stream;
    if (hipStreamCreate(&stream) != hipSuccess) throw pa::Error("no HIP device");
    Context ctx;
    ctx.stream = stream;

    fem::DefaultIntegrationOrder::p_trial = order;
    Mesh mesh(ctx, ne, 2, nn, i32(1), f64(2), i32(3), fem::DefaultIntegrationOrder::GetQ1d(2 * 3 - 1));

    FiniteElementSpaceHierarchy nd_fespaces;
    int constrained = 0;
    for (int l = 0; l < nlev; l++) {
      const size_t b = 4 + 8 * (size_t)l;
      const int p = i32(0)[4 + l], n_local = i32(b)[0], n_true = i32(b)[1];
      auto nd = std::make_unique<FiniteElementSpace>(ctx, mesh, PA_FE_HCURL, p, n_local, i32(b + 1),
                                                     reinterpret_cast<const uint8_t *>(blobs[b + 2].data()), i32(b + 3));
      // (int and int32_t are the same type here: the row pointer is stored as int32)
      nd->SetConformingProlongation(n_true, reinterpret_cast<const int *>(blobs[b + 5].data()), i32(b + 6), f64(b + 7));
      nd->SetEssentialTrueDofs(i32(b + 4), (int)(blobs[b + 4].size() / 4));
      constrained = n_local - n_true;
      nd_fespaces.AddLevel(std::move(nd));
    }

    MaterialPropertyCoefficient muinv(1), eps(1);
    muinv.AddMaterialProperty(1, 1.0);
    eps.AddMaterialProperty(1, 2.08);

    BilinearForm a(nd_fespaces.GetFinestFESpace());
    a.AddDomainIntegrator<CurlCurlMassIntegrator>(muinv, eps);
    auto a_ops = a.Assemble(nd_fespaces, /*skip_zeros=*/false);
    auto A = std::make_unique<MultigridOperator>(nd_fespaces.GetNumLevels());
    for (std::size_t l = 0; l < nd_fespaces.GetNumLevels(); l++) {
      const auto &fes = nd_fespaces.GetFESpaceAtLevel(l);
      auto op = std::make_unique<FespaceParOperator>(std::move(a_ops[l]), fes);
      op->SetEssentialTrueDofs(fes.GetEssentialTrueDofs(), ParOperator::DiagonalPolicy::DIAG_ONE);
      A->AddOperator(std::move(op));
    }

    config::LinearSolverData linear;
    linear.krylov_solver = KrylovSolver::CG;
    linear.type = coarse == "pcg"      ? LinearSolver::JACOBI_PCG
                  : coarse == "jacobi" ? LinearSolver::JACOBI
                  : coarse == "amg"    ? LinearSolver::BOOMER_AMG
                                       : LinearSolver::CHEBYSHEV_JACOBI;
    linear.tol = 1e-10, linear.max_it = 400;
    linear.mg_smooth_aux = 0;
    linear.initial_guess = 0;
    linear.SetDefaults(order, /*spd_problem=*/true);
    KspSolver ksp(linear, /*verbose=*/0, nd_fespaces, nullptr);
    ksp.SetOperators(*A, *A);

    const int n = A->Height();
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
