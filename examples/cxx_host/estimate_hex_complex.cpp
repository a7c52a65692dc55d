// C++ host example: the flux error estimators for a COMPLEX field on a hexahedral mesh (the ComplexVector instantiation of
// linalg/errorestimator.cpp:183-268, :272-480 that the eigenmode and driven drivers call).  A tensor Mesh with a Nedelec and a
// Raviart-Thomas space of one order (see dump_estimator_hex_complex_problem.py); ComplexGradFluxErrorEstimator (E in H(curl))
// and ComplexCurlFluxErrorEstimator (B in H(div)) take both parts of the field through every step together: the flux operator
// (pa_op_mult2), the mass solve (ComplexCgSolver + ComplexJacobiSmoother on a ComplexParOperator with a real part only; its
// apply is one pa_op_mult2 per iteration where the mass operator has a two-vector kernel, else two applies: the output says
// which and counts them) and the element error integrator (pa_error_op_apply_add2).  Writes the element estimates of both and the two smooth fluxes.
//   ./estimate_hex_complex problem.bin out.bin
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

static void upload(ComplexVector &v, const double *re, const double *im) {
  hipMemcpy(v.Real().Data(), re, sizeof(double) * v.Size(), hipMemcpyHostToDevice);
  hipMemcpy(v.Imag().Data(), im, sizeof(double) * v.Size(), hipMemcpyHostToDevice);
}

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  try {
    auto blobs = read_blobs(argv[1]);
    auto i32 = [&](size_t i) { return reinterpret_cast<const int32_t *>(blobs[i].data()); };
    auto f64 = [&](size_t i) { return reinterpret_cast<const double *>(blobs[i].data()); };
    auto u8 = [&](size_t i) { return reinterpret_cast<const uint8_t *>(blobs[i].data()); };
    const int ne = i32(0)[0], nn = i32(0)[1], p = i32(0)[2], q1d = i32(0)[3], nd_size = i32(0)[4], rt_size = i32(0)[5];
    hipStream_t stream;
    if (hipStreamCreate(&stream) != hipSuccess) throw pa::Error("no HIP device");
    Context ctx;
    ctx.stream = stream;

    Mesh mesh(ctx, ne, 2, nn, i32(1), f64(2), i32(3), q1d);
    FiniteElementSpace nd(ctx, mesh, PA_FE_HCURL, p, nd_size, i32(4), u8(5), nullptr);
    FiniteElementSpace rt(ctx, mesh, PA_FE_HDIV, p, rt_size, i32(6), u8(7), nullptr);
    MaterialTensors eps{{0, 1}, std::vector<double>(f64(8), f64(8) + 18)};
    MaterialTensors muinv{{0, 1}, std::vector<double>(f64(9), f64(9) + 18)};

    ComplexVector E(nd_size), B(rt_size);
    upload(E, f64(10), f64(11));
    upload(B, f64(12), f64(13));

    const double tol = 1e-13;
    ComplexGradFluxErrorEstimator grad(eps, nd, rt, tol, 1000, 0);
    ComplexCurlFluxErrorEstimator curl(muinv, rt, nd, tol, 1000, 0);
    Vector eg(ne), ec(ne);
    linalg::Fill(ctx, eg, 0.0);
    linalg::Fill(ctx, ec, 0.0);
    grad.AddErrorEstimates(E, eg);
    const int its_grad = grad.GetProjector().NumIterations();
    const long mass2_grad = grad.GetProjector().MassOnePassApplies();  // mass applies of this solve that took both parts in one pass
    curl.AddErrorEstimates(B, ec);
    const int its_curl = curl.GetProjector().NumIterations();
    const long mass2_curl = curl.GetProjector().MassOnePassApplies();
    ErrorIndicator ind(ctx);
    grad.AddErrorIndicator(E, 0.0, ind);
    curl.AddErrorIndicator(B, 0.0, ind);
    hipStreamSynchronize(stream);
    const ComplexVector &D = grad.GetSmoothFlux(), &H = curl.GetSmoothFlux();
    std::vector<double> out((size_t)2 * ne + 2 * (size_t)rt_size + 2 * (size_t)nd_size);
    double *o = out.data();
    for (const Vector *v : {(const Vector *)&eg, (const Vector *)&ec, &D.Real(), &D.Imag(), &H.Real(), &H.Imag()}) {
      hipMemcpy(o, v->Data(), sizeof(double) * v->Size(), hipMemcpyDeviceToHost);
      o += v->Size();
    }
    std::ofstream(argv[2], std::ios::binary).write(reinterpret_cast<const char *>(out.data()), sizeof(double) * out.size());
    double sum_g = 0.0, sum_c = 0.0;
    for (int e = 0; e < ne; e++) sum_g += out[e], sum_c += out[(size_t)ne + e];
    std::printf("hexes %d order %d nd %d rt %d\n", ne, p, nd_size, rt_size);
    std::printf("grad: pcg_its %d checksum %.15e one_pass flux %d mass %d error %d mass_one_pass_applies %ld\n", its_grad, sum_g,
                (int)grad.GetProjector().FluxTwoRhs(), (int)grad.GetProjector().MassTwoRhs(), (int)grad.TwoParts(), mass2_grad);
    std::printf("curl: pcg_its %d checksum %.15e one_pass flux %d mass %d error %d mass_one_pass_applies %ld\n", its_curl, sum_c,
                (int)curl.GetProjector().FluxTwoRhs(), (int)curl.GetProjector().MassTwoRhs(), (int)curl.TwoParts(), mass2_curl);
    std::printf("indicator: norm %.15e\nOK\n", ind.Norml2());
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
