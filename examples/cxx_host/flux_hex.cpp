// C++ host example: the flux B = curl A on a hexahedral mesh and the estimator that consumes it, on the same tensor Mesh and
// FiniteElementSpace objects a solver uses.  Reads the file dump_estimator_hex_problem.py writes (its field E serves as the
// potential A, its field B as an input of the transposed curl).  The discrete curl is the one Palace asks the Raviart-Thomas
// space for (fem/fespace.cpp:199-206: rt.GetDiscreteInterpolator(nd)), here sum-factorised (pa_curl_hex.hip);
// CurlFluxErrorEstimator then runs on the COMPUTED flux.  Writes B = C A, C^T B_file, the element estimates and the smooth flux.
//   ./flux_hex problem.bin out.bin
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
    MaterialTensors muinv{{0, 1}, std::vector<double>(f64(9), f64(9) + 18)};

    Vector A(nd_size), Bfile(rt_size), B(rt_size), CtB(nd_size);
    hipMemcpy(A.Data(), f64(10), sizeof(double) * nd_size, hipMemcpyHostToDevice);
    hipMemcpy(Bfile.Data(), f64(11), sizeof(double) * rt_size, hipMemcpyHostToDevice);

    const Operator &Curl = rt.GetDiscreteInterpolator(nd);
    if (&Curl != &rt.GetDiscreteInterpolator(nd)) throw pa::Error("the discrete curl is not cached");
    bool refused = false;  // (the pair the other way round is no discrete interpolator)
    try {
      nd.GetDiscreteInterpolator(rt);
    } catch (const std::exception &e) {
      refused = true;
      std::printf("refused: %s\n", e.what());
    }
    if (!refused) throw pa::Error("ND.GetDiscreteInterpolator(RT) was accepted");
    Curl.Mult(A, B);
    Curl.MultTranspose(Bfile, CtB);

    CurlFluxErrorEstimator est(muinv, rt, nd, 1e-13, 1000, 0);
    Vector ec(ne), H(nd_size);
    linalg::Fill(ctx, ec, 0.0);
    est.AddErrorEstimates(B, ec);
    const int its = est.GetProjector().NumIterations();
    est.GetProjector().Mult(B, H);  // the smooth flux itself
    hipStreamSynchronize(stream);
    std::vector<double> out((size_t)rt_size + nd_size + ne + nd_size);
    double *o = out.data();
    hipMemcpy(o, B.Data(), sizeof(double) * rt_size, hipMemcpyDeviceToHost);
    hipMemcpy(o + rt_size, CtB.Data(), sizeof(double) * nd_size, hipMemcpyDeviceToHost);
    hipMemcpy(o + rt_size + nd_size, ec.Data(), sizeof(double) * ne, hipMemcpyDeviceToHost);
    hipMemcpy(o + rt_size + nd_size + ne, H.Data(), sizeof(double) * nd_size, hipMemcpyDeviceToHost);
    std::ofstream(argv[2], std::ios::binary).write(reinterpret_cast<const char *>(out.data()), sizeof(double) * out.size());
    std::printf("hexes %d order %d nd %d rt %d\n", ne, p, nd_size, rt_size);
    std::printf("curl: pcg_its %d\nOK\n", its);
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
