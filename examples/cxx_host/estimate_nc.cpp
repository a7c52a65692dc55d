// C++ host example: the flux error estimators on a hexahedral mesh with hanging nodes -- the second estimator pass of the
// reference's adapt loop (BaseSolver::SolveEstimateMarkRefine) on a nonconformally refined mesh.  A tensor Mesh with a Nedelec and
// a Raviart-Thomas space of one order, both carrying their hanging-node constraints (SetConformingProlongation; see
// dump_estimator_nc_problem.py), fields on the true dofs.  GradFluxErrorEstimator / CurlFluxErrorEstimator on the real and on the
// imaginary part, then ComplexGradFluxErrorEstimator / ComplexCurlFluxErrorEstimator on both together: the right-hand side of the
// projection is P_smooth^T Flux P_rhs x, the mass P^T M P with Jacobi on |P|^T diag, the complex mass apply P2, Mult2, P^T2 where
// the mass operator has a two-vector kernel.  Also shows that the multigrid projector (use_mg = true) refuses a constrained
// smooth space.  Writes the element estimates and the real smooth fluxes.
//   ./estimate_nc problem.bin out.bin
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <vector>

#include "errorestimator.hpp"

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

static void upload(Vector &v, const double *h) { hipMemcpy(v.Data(), h, sizeof(double) * v.Size(), hipMemcpyHostToDevice); }

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  try {
    auto blobs = read_blobs(argv[1]);
    auto i32 = [&](size_t i) { return reinterpret_cast<const int32_t *>(blobs[i].data()); };
    auto f64 = [&](size_t i) { return reinterpret_cast<const double *>(blobs[i].data()); };
    auto u8 = [&](size_t i) { return reinterpret_cast<const uint8_t *>(blobs[i].data()); };
    const int ne = i32(0)[0], nn = i32(0)[1], p = i32(0)[2], q1d = i32(0)[3], nd_local = i32(0)[4], rt_local = i32(0)[5],
              nd_true = i32(0)[6], rt_true = i32(0)[7];
    hipStream_t stream;
    if (hipStreamCreate(&stream) != hipSuccess) throw pa::Error("no HIP device");
    Context ctx;
    ctx.stream = stream;

    Mesh mesh(ctx, ne, 2, nn, i32(1), f64(2), i32(3), q1d);
    auto make_space = [&](int fe_type, int n_local, int n_true, size_t dofs, size_t csr) {
      auto s = std::make_unique<FiniteElementSpace>(ctx, mesh, fe_type, p, n_local, i32(dofs), u8(dofs + 1), nullptr);
      // (int and int32_t are the same type here: the row pointer is stored as int32)
      s->SetConformingProlongation(n_true, reinterpret_cast<const int *>(blobs[csr].data()), i32(csr + 1), f64(csr + 2));
      return s;
    };
    auto nd_p = make_space(PA_FE_HCURL, nd_local, nd_true, 4, 10), rt_p = make_space(PA_FE_HDIV, rt_local, rt_true, 6, 13);
    const FiniteElementSpace &nd = *nd_p, &rt = *rt_p;
    MaterialTensors eps{{0, 1}, std::vector<double>(f64(8), f64(8) + 18)};
    MaterialTensors muinv{{0, 1}, std::vector<double>(f64(9), f64(9) + 18)};

    ComplexVector E(nd_true), B(rt_true);
    upload(E.Real(), f64(16)), upload(E.Imag(), f64(17));
    upload(B.Real(), f64(18)), upload(B.Imag(), f64(19));

    const double tol = 1e-13;
    // ---- real estimators, on either part
    GradFluxErrorEstimator grad(eps, nd, rt, tol, 1000, 0);
    CurlFluxErrorEstimator curl(muinv, rt, nd, tol, 1000, 0);
    Vector eg(ne), ec(ne), eg_im(ne), ec_im(ne), eg2(ne), ec2(ne);
    for (Vector *v : {&eg, &ec, &eg_im, &ec_im, &eg2, &ec2}) linalg::Fill(ctx, *v, 0.0);
    grad.AddErrorEstimates(E.Imag(), eg_im);
    curl.AddErrorEstimates(B.Imag(), ec_im);
    grad.AddErrorEstimates(E.Real(), eg);
    const int its_grad = grad.GetProjector().NumIterations();
    curl.AddErrorEstimates(B.Real(), ec);
    const int its_curl = curl.GetProjector().NumIterations();
    hipStreamSynchronize(stream);
    std::vector<double> out((size_t)6 * ne + (size_t)rt_true + (size_t)nd_true);
    double *o = out.data() + (size_t)6 * ne;
    for (const Vector *v : {&grad.GetSmoothFlux(), &curl.GetSmoothFlux()}) {  // the smooth fluxes of the real parts
      hipMemcpy(o, v->Data(), sizeof(double) * v->Size(), hipMemcpyDeviceToHost);
      o += v->Size();
    }
    // ---- complex estimators: both parts through every step together
    ComplexGradFluxErrorEstimator cgrad(eps, nd, rt, tol, 1000, 0);
    ComplexCurlFluxErrorEstimator ccurl(muinv, rt, nd, tol, 1000, 0);
    cgrad.AddErrorEstimates(E, eg2);
    ccurl.AddErrorEstimates(B, ec2);
    hipStreamSynchronize(stream);
    o = out.data();
    for (const Vector *v : {&eg, &ec, &eg_im, &ec_im, &eg2, &ec2}) {
      hipMemcpy(o, v->Data(), sizeof(double) * ne, hipMemcpyDeviceToHost);
      o += ne;
    }
    std::ofstream(argv[2], std::ios::binary).write(reinterpret_cast<const char *>(out.data()), sizeof(double) * out.size());
    std::printf("hexes %d order %d nd %d / %d rt %d / %d\n", ne, p, nd_true, nd_local, rt_true, rt_local);
    std::printf("grad: pcg_its %d\ncurl: pcg_its %d\n", its_grad, its_curl);
    std::printf("complex grad: pcg_its %d one_pass flux %d mass %d mass_one_pass_applies %ld\n", cgrad.GetProjector().NumIterations(),
                (int)cgrad.GetProjector().FluxTwoRhs(), (int)cgrad.GetProjector().MassTwoRhs(), cgrad.GetProjector().MassOnePassApplies());
    std::printf("complex curl: pcg_its %d one_pass flux %d mass %d mass_one_pass_applies %ld\n", ccurl.GetProjector().NumIterations(),
                (int)ccurl.GetProjector().FluxTwoRhs(), (int)ccurl.GetProjector().MassTwoRhs(), ccurl.GetProjector().MassOnePassApplies());
    // ---- the multigrid projector on a constrained smooth space is refused, real and complex
    FiniteElementSpaceHierarchy rt_fespaces(std::move(rt_p));
    for (int complex_field = 0; complex_field < 2; complex_field++) {
      try {
        if (complex_field)
          ComplexGradFluxErrorEstimator refused(eps, nd, rt_fespaces, tol, 1000, 0, /*use_mg=*/true);
        else
          GradFluxErrorEstimator refused(eps, nd, rt_fespaces, tol, 1000, 0, /*use_mg=*/true);
        std::printf("use_mg %d: accepted\n", complex_field);
      } catch (const std::exception &e) {
        std::printf("use_mg %d: refused: %s\n", complex_field, e.what());
      }
    }
    {  // ... and use_mg = false on the same hierarchy is the Jacobi form above
      GradFluxErrorEstimator plain(eps, nd, rt_fespaces, tol, 1000, 0, /*use_mg=*/false);
      Vector e3(ne);
      linalg::Fill(ctx, e3, 0.0);
      plain.AddErrorEstimates(E.Real(), e3);
      hipStreamSynchronize(stream);
      std::vector<double> h((size_t)ne);
      hipMemcpy(h.data(), e3.Data(), sizeof(double) * ne, hipMemcpyDeviceToHost);
      std::printf("hierarchy use_mg 0: same %d\n", (int)(std::memcmp(h.data(), out.data(), sizeof(double) * ne) == 0));
    }
    std::printf("OK\n");
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
