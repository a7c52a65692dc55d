// C++ host example: the multigrid (use_mg) option of the flux error estimators on a hexahedral mesh (FluxProjector with a
// FiniteElementSpaceHierarchy of the smooth space, linalg/errorestimator.cpp:67-104, :132-147).  A tensor Mesh with the Nedelec
// and the Raviart-Thomas spaces of orders 1 .. p (see dump_estimator_hex_mg_problem.py).  The gradient estimator (E in H(curl),
// smooth flux in the RT hierarchy) and the curl estimator (B in H(div), smooth flux in the ND hierarchy), each for a real and for
// a complex field, run three times: PCG + Jacobi (use_mg = false), PCG + the p-multigrid cycle over levels 1 .. p, and PCG + the
// AMG alone on a one-level hierarchy.  Prints the iteration counts and writes the three sets of element estimates.
//   ./estimate_hex_mg problem.bin out.bin [tol]
#include <cmath>
#include <cstdio>
#include <cstdlib>
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

static void upload(Vector &v, const double *x) { hipMemcpy(v.Data(), x, sizeof(double) * v.Size(), hipMemcpyHostToDevice); }

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  try {
    auto blobs = read_blobs(argv[1]);
    auto i32 = [&](size_t i) { return reinterpret_cast<const int32_t *>(blobs[i].data()); };
    auto f64 = [&](size_t i) { return reinterpret_cast<const double *>(blobs[i].data()); };
    auto u8 = [&](size_t i) { return reinterpret_cast<const uint8_t *>(blobs[i].data()); };
    const int ne = i32(0)[0], nn = i32(0)[1], p = i32(0)[2], q1d = i32(0)[3];
    const int32_t *nd_sizes = i32(0) + 4, *rt_sizes = i32(0) + 4 + p;
    const double tol = argc > 3 ? std::atof(argv[3]) : 1e-12;
    hipStream_t stream;
    if (hipStreamCreate(&stream) != hipSuccess) throw pa::Error("no HIP device");
    Context ctx;
    ctx.stream = stream;

    Mesh mesh(ctx, ne, 2, nn, i32(1), f64(2), i32(3), q1d);
    // hierarchies 1 .. p, and the one-level hierarchies of the finest spaces
    FiniteElementSpaceHierarchy nd_fespaces, rt_fespaces, nd_one, rt_one;
    for (int l = 0; l < p; l++) {
      const size_t bn = 10 + 2 * (size_t)l, br = 10 + 2 * (size_t)(p + l);
      nd_fespaces.AddLevel(std::make_unique<FiniteElementSpace>(ctx, mesh, PA_FE_HCURL, l + 1, nd_sizes[l], i32(bn), u8(bn + 1), nullptr));
      rt_fespaces.AddLevel(std::make_unique<FiniteElementSpace>(ctx, mesh, PA_FE_HDIV, l + 1, rt_sizes[l], i32(br), u8(br + 1), nullptr));
    }
    const size_t bn = 10 + 2 * (size_t)(p - 1), br = 10 + 2 * (size_t)(2 * p - 1);
    const int nd_size = nd_sizes[p - 1], rt_size = rt_sizes[p - 1];
    nd_one.AddLevel(std::make_unique<FiniteElementSpace>(ctx, mesh, PA_FE_HCURL, p, nd_size, i32(bn), u8(bn + 1), nullptr));
    rt_one.AddLevel(std::make_unique<FiniteElementSpace>(ctx, mesh, PA_FE_HDIV, p, rt_size, i32(br), u8(br + 1), nullptr));
    const FiniteElementSpace &nd = nd_fespaces.GetFinestFESpace(), &rt = rt_fespaces.GetFinestFESpace();
    MaterialTensors eps{{0, 1}, std::vector<double>(f64(4), f64(4) + 18)};
    MaterialTensors muinv{{0, 1}, std::vector<double>(f64(5), f64(5) + 18)};

    ComplexVector E(nd_size), B(rt_size);
    upload(E.Real(), f64(6)), upload(E.Imag(), f64(7)), upload(B.Real(), f64(8)), upload(B.Imag(), f64(9));

    // rows of one set: grad real, curl real, grad complex, curl complex
    std::vector<double> out((size_t)3 * 4 * ne);
    const char *names[3] = {"jacobi", "mg", "amg"};
    int all_converged = 1;
    for (int mode = 0; mode < 3; mode++) {
      const FiniteElementSpaceHierarchy &rts = mode == 1 ? rt_fespaces : rt_one, &nds = mode == 1 ? nd_fespaces : nd_one;
      const FiniteElementSpace &rt_m = rts.GetFinestFESpace(), &nd_m = nds.GetFinestFESpace();
      const bool use_mg = mode > 0;
      GradFluxErrorEstimator grad(eps, nd_m, rts, tol, 1000, 0, use_mg);
      CurlFluxErrorEstimator curl(muinv, rt_m, nds, tol, 1000, 0, use_mg);
      ComplexGradFluxErrorEstimator cgrad(eps, nd_m, rts, tol, 1000, 0, use_mg);
      ComplexCurlFluxErrorEstimator ccurl(muinv, rt_m, nds, tol, 1000, 0, use_mg);
      Vector est[4];
      for (Vector &v : est) {
        v.SetSize(ne);
        linalg::Fill(ctx, v, 0.0);
      }
      grad.AddErrorEstimates(E.Real(), est[0]);
      curl.AddErrorEstimates(B.Real(), est[1]);
      cgrad.AddErrorEstimates(E, est[2]);
      ccurl.AddErrorEstimates(B, est[3]);
      hipStreamSynchronize(stream);
      const int its[4] = {grad.GetProjector().NumIterations(), curl.GetProjector().NumIterations(),
                          cgrad.GetProjector().NumIterations(), ccurl.GetProjector().NumIterations()};
      const int conv[4] = {(int)grad.GetProjector().Converged(), (int)curl.GetProjector().Converged(),
                           (int)cgrad.GetProjector().Converged(), (int)ccurl.GetProjector().Converged()};
      const int mg[4] = {(int)grad.GetProjector().UsesMultigrid(), (int)curl.GetProjector().UsesMultigrid(),
                         (int)cgrad.GetProjector().UsesMultigrid(), (int)ccurl.GetProjector().UsesMultigrid()};
      for (int k = 0; k < 4; k++) {
        hipMemcpy(out.data() + ((size_t)mode * 4 + k) * ne, est[k].Data(), sizeof(double) * ne, hipMemcpyDeviceToHost);
        all_converged = all_converged && conv[k];
      }
      std::printf("%s: levels %d its grad %d curl %d cgrad %d ccurl %d converged %d %d %d %d use_mg %d %d %d %d mass_one_pass %d %d\n",
                  names[mode], (int)rts.GetNumLevels(), its[0], its[1], its[2], its[3], conv[0], conv[1], conv[2], conv[3], mg[0], mg[1],
                  mg[2], mg[3], (int)cgrad.GetProjector().MassTwoRhs(), (int)ccurl.GetProjector().MassTwoRhs());
    }
    std::ofstream(argv[2], std::ios::binary).write(reinterpret_cast<const char *>(out.data()), sizeof(double) * out.size());

    // two Raviart-Thomas levels of equal order are no hierarchy: the multigrid projector over them is refused
    FiniteElementSpaceHierarchy equal;
    equal.AddLevel(std::make_unique<FiniteElementSpace>(ctx, mesh, PA_FE_HDIV, p, rt_size, i32(br), u8(br + 1), nullptr));
    equal.AddLevel(std::make_unique<FiniteElementSpace>(ctx, mesh, PA_FE_HDIV, p, rt_size, i32(br), u8(br + 1), nullptr));
    try {
      GradFluxErrorEstimator refused(eps, nd, equal, tol, 1000, 0, true);
      std::printf("equal-order hierarchy accepted\n");
    } catch (const std::exception &e) {
      std::printf("equal-order hierarchy refused: %s\n", e.what());
    }
    std::printf("hexes %d order %d nd %d rt %d tol %.1e all_converged %d\nOK\n", ne, p, nd_size, rt_size, tol, all_converged);
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
