// C++ host example: the operators of the flux and smooth-flux spaces of a hexahedral mesh.  On a Raviart-Thomas space given
// by its tensor description (see dump_rt_hex_problem.py) it assembles, with the classes of fem.hpp / ksp.hpp used the way
// the error estimators of linalg/errorestimator.cpp use theirs,
//   m.AddDomainIntegrator<VectorFEMassIntegrator>(eps)           (f_apply_hdiv_33)
//   k.AddDomainIntegrator<DivDivMassIntegrator>(lambda, eps)      (f_apply_l2mass_33)
// both on the sum-factorised hex kernel, applies each to a vector, assembles their diagonals and writes the four vectors;
// then it solves M d = b, b = M d0, with PCG + Jacobi through KspSolver and prints the iteration count, and shows that a
// hierarchy of such spaces refuses to build a prolongation.
//   ./rt_mass_hex problem.bin out.bin
#include <cstdio>
#include <cstdlib>
#include <fstream>
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
  if (argc < 3) return 2;
  try {
    auto blobs = read_blobs(argv[1]);
    auto i32 = [&](size_t i) { return reinterpret_cast<const int32_t *>(blobs[i].data()); };
    auto f64 = [&](size_t i) { return reinterpret_cast<const double *>(blobs[i].data()); };
    auto u8 = [&](size_t i) { return reinterpret_cast<const uint8_t *>(blobs[i].data()); };
    const int ne = i32(0)[0], nn = i32(0)[1], p = i32(0)[2], q1d = i32(0)[3], n = i32(0)[4];
    hipStream_t stream;
    if (hipStreamCreate(&stream) != hipSuccess) throw pa::Error("no HIP device");
    Context ctx;
    ctx.stream = stream;

    Mesh mesh(ctx, ne, 2, nn, i32(1), f64(2), i32(3), q1d);
    FiniteElementSpaceHierarchy rt_fespaces;
    rt_fespaces.AddLevel(std::make_unique<FiniteElementSpace>(ctx, mesh, PA_FE_HDIV, p, n, i32(4), u8(5), nullptr));
    const FiniteElementSpace &rt = rt_fespaces.GetFinestFESpace();

    const std::vector<int> attr_mat{0, 1};
    MaterialPropertyCoefficient eps(attr_mat, 3, std::vector<double>(f64(6), f64(6) + 18)),
        lambda(attr_mat, 1, std::vector<double>(f64(7), f64(7) + 2));

    BilinearForm m(rt), k(rt);
    m.AddDomainIntegrator<VectorFEMassIntegrator>(eps);
    k.AddDomainIntegrator<DivDivMassIntegrator>(lambda, eps);
    auto M = m.PartialAssemble(), K = k.PartialAssemble();

    Vector x(n), y(n), d(n);
    std::vector<double> out((size_t)4 * n);
    hipMemcpy(x.Data(), f64(8), sizeof(double) * n, hipMemcpyHostToDevice);
    int row = 0;
    for (const auto *A : {M.get(), K.get()}) {
      A->Mult(x, y);
      A->AssembleDiagonal(d);
      hipStreamSynchronize(stream);
      hipMemcpy(out.data() + (size_t)(row++) * n, y.Data(), sizeof(double) * n, hipMemcpyDeviceToHost);
      hipMemcpy(out.data() + (size_t)(row++) * n, d.Data(), sizeof(double) * n, hipMemcpyDeviceToHost);
    }
    std::ofstream(argv[2], std::ios::binary).write(reinterpret_cast<const char *>(out.data()), sizeof(double) * out.size());
    const int symmetric = (int)(M->IsSymmetric() && K->IsSymmetric());

    // the smooth-flux projection solve: M d = b with PCG + Jacobi, no essential dofs
    FespaceParOperator Mp(std::move(M), rt);
    config::LinearSolverData linear;
    linear.krylov_solver = KrylovSolver::CG;
    linear.type = LinearSolver::JACOBI;
    linear.tol = 1e-12, linear.max_it = 1000, linear.initial_guess = 0;
    linear.SetDefaults(p, /*spd_problem=*/true);
    KspSolver ksp(linear, /*verbose=*/0, rt_fespaces);
    ksp.SetOperators(Mp, Mp);
    Vector d0(n), b(n), sol(n);
    hipMemcpy(d0.Data(), f64(9), sizeof(double) * n, hipMemcpyHostToDevice);
    Mp.Mult(d0, b);
    ksp.Mult(b, sol);
    linalg::AXPBY(ctx, 1.0, d0, -1.0, sol);
    // a Raviart-Thomas space has no multigrid hierarchy: asking a two-level hierarchy for its prolongation is refused
    FiniteElementSpaceHierarchy two;
    two.AddLevel(std::make_unique<FiniteElementSpace>(ctx, mesh, PA_FE_HDIV, p, n, i32(4), u8(5), nullptr));
    two.AddLevel(std::make_unique<FiniteElementSpace>(ctx, mesh, PA_FE_HDIV, p, n, i32(4), u8(5), nullptr));
    try {
      two.GetProlongationOperators();
      std::printf("prolongation built\n");
    } catch (const std::exception &e) {
      std::printf("prolongation refused: %s\n", e.what());
    }
    std::printf("hexes %d order %d dofs %d symmetric %d iterations %d converged %d |d - d0| / |d0| %.3e\nOK\n", ne, p, n, symmetric,
                ksp.GetKrylovSolver().GetNumIterations(), (int)ksp.GetKrylovSolver().GetConverged(),
                linalg::Norml2(ctx, sol) / linalg::Norml2(ctx, d0));
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
