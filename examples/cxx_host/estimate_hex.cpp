// C++ host example: the flux error estimators of linalg/errorestimator.cpp on a hexahedral mesh, on the same tensor Mesh and
// FiniteElementSpace objects a solver uses.  A Nedelec and a Raviart-Thomas space of one order are given by their tensor
// descriptions (see dump_estimator_hex_problem.py); GradFluxErrorEstimator (E in H(curl), smooth flux in H(div)) and
// CurlFluxErrorEstimator (B in H(div), smooth flux in H(curl)) then run sum-factorised throughout: the flux operator
// (pa_op_add_sub_mixed), the mass of the smooth space under PCG + Jacobi (pa_op_add_sub) and the element error integrator
// (pa_error_op_create_tensor).  Writes the element estimates of both and the two smooth fluxes.
//   ./estimate_hex problem.bin out.bin
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

    Vector E(nd_size), B(rt_size);
    hipMemcpy(E.Data(), f64(10), sizeof(double) * nd_size, hipMemcpyHostToDevice);
    hipMemcpy(B.Data(), f64(11), sizeof(double) * rt_size, hipMemcpyHostToDevice);

    const double tol = 1e-13;
    GradFluxErrorEstimator grad(eps, nd, rt, tol, 1000, 0);
    CurlFluxErrorEstimator curl(muinv, rt, nd, tol, 1000, 0);
    Vector eg(ne), ec(ne), D(rt_size), H(nd_size);
    linalg::Fill(ctx, eg, 0.0);
    linalg::Fill(ctx, ec, 0.0);
    grad.AddErrorEstimates(E, eg);
    const int its_grad = grad.GetProjector().NumIterations();
    curl.AddErrorEstimates(B, ec);
    const int its_curl = curl.GetProjector().NumIterations();
    grad.GetProjector().Mult(E, D);  // the smooth fluxes themselves
    curl.GetProjector().Mult(B, H);
    // the time-dependent estimator is the two together (errorestimator.cpp:512-541)
    TimeDependentFluxErrorEstimator both(eps, muinv, nd, rt, tol, 1000, 0);
    ErrorIndicator it(ctx);
    both.AddErrorIndicator(E, B, 0.0, it);
    hipStreamSynchronize(stream);
    std::vector<double> out((size_t)3 * ne + rt_size + nd_size);
    hipMemcpy(out.data(), eg.Data(), sizeof(double) * ne, hipMemcpyDeviceToHost);
    hipMemcpy(out.data() + ne, ec.Data(), sizeof(double) * ne, hipMemcpyDeviceToHost);
    hipMemcpy(out.data() + 2 * (size_t)ne, it.Local().Data(), sizeof(double) * ne, hipMemcpyDeviceToHost);
    hipMemcpy(out.data() + 3 * (size_t)ne, D.Data(), sizeof(double) * rt_size, hipMemcpyDeviceToHost);
    hipMemcpy(out.data() + 3 * (size_t)ne + rt_size, H.Data(), sizeof(double) * nd_size, hipMemcpyDeviceToHost);
    std::ofstream(argv[2], std::ios::binary).write(reinterpret_cast<const char *>(out.data()), sizeof(double) * out.size());
    std::printf("hexes %d order %d nd %d rt %d\n", ne, p, nd_size, rt_size);
    std::printf("grad: pcg_its %d\ncurl: pcg_its %d\n", its_grad, its_curl);
    std::printf("both: norm %.15e\nOK\n", it.Norml2());
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
