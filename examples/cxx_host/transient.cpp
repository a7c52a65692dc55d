// C++ host example: the reference's transient driver (drivers/transientsolver.cpp:25-116) on its coaxial example
// (examples/coaxial/coaxial_matched.json: order 3, two coaxial lumped ports, 200 generalized-alpha steps), from the arrays of
// dump_transient_problem.py.  SpaceOperator's part is written out with palace::fem: K (curl-curl, mu^-1), M (mass, eps),
// C (mass with sigma + the 1 / R_s surface masses on the port faces: BilinearForm with a domain and a boundary integrator), the
// discrete curl; TimeOperator gets them with a Jacobi-PCG KspSolver for M and the callback that (re)builds
// A(a) = M + a C + a^2 K on every level of the p-hierarchy -- one CurlCurlMassIntegrator(a^2 mu^-1, eps + a sigma) with the
// a / R_s surface mass beside it -- and its KspSolver (PCG, p-multigrid, Jacobi-PCG on the coarsest level), as
// ConfigureLinearSolver does (models/timeoperator.cpp:93-108).  Prints t, V[1], V[2], E_elec, E_mag per step and the statistics.
//   ./transient problem.bin
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>

#include "timeoperator.hpp"

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
  try {
    auto blobs = read_blobs(argv[1]);
    auto i32 = [&](size_t i) { return reinterpret_cast<const int32_t *>(blobs[i].data()); };
    auto f64 = [&](size_t i) { return reinterpret_cast<const double *>(blobs[i].data()); };
    auto u8 = [&](size_t i) { return reinterpret_cast<const uint8_t *>(blobs[i].data()); };
    const int32_t *h = i32(0);
    const int ne = h[0], nn = h[1], order = h[2], q1d = h[3], nlev = h[4], rt_size = h[5], nsteps = h[6], max_it = h[7];
    const double *sc = f64(4);
    double dt = sc[0];
    const double omega = sc[1], tau = sc[2], t0 = sc[3], sigma_v = sc[4], eps_v = sc[5], muinv_v = sc[6], volts = sc[9],
                 joules = sc[10], rho_inf = sc[11], tol = sc[12];
    hipStream_t stream;
    if (hipStreamCreate(&stream) != hipSuccess) throw pa::Error("no HIP device");
    Context ctx;
    ctx.stream = stream;
    fem::DefaultIntegrationOrder::p_trial = order;

    Mesh mesh(ctx, ne, 2, nn, i32(1), f64(2), i32(3), q1d);
    // the spaces of the p-hierarchy and their views on the port faces
    const size_t per_level = 8, b_shared = 5 + per_level * nlev;
    const int bne = i32(5)[1], bnq = i32(5)[3];
    pa_mesh_dense_desc bd{bne, 9, bnq, nn, i32(b_shared), f64(2), i32(b_shared + 1), f64(b_shared + 2), f64(b_shared + 3), 2, 3};
    Mesh bdr_mesh(ctx, bd);
    FiniteElementSpaceHierarchy nd_fespaces;
    std::vector<std::unique_ptr<FiniteElementSpace>> nd_bdr;
    for (int l = 0; l < nlev; l++) {
      const size_t b = 5 + per_level * l;
      const int p = h[8 + l], nd_size = i32(b)[0], b_P = i32(b)[2];
      auto nd = std::make_unique<FiniteElementSpace>(ctx, mesh, PA_FE_HCURL, p, nd_size, i32(b + 1), u8(b + 2), nullptr);
      nd->SetEssentialTrueDofs(i32(b + 3), (int)(blobs[b + 3].size() / 4));
      nd_fespaces.AddLevel(std::move(nd));
      nd_bdr.push_back(std::make_unique<FiniteElementSpace>(ctx, bdr_mesh, PA_FE_HCURL, p, b_P, nd_size, i32(b + 4), u8(b + 5),
                                                            nullptr, f64(b + 6), nullptr));
    }
    const FiniteElementSpace &nd = nd_fespaces.GetFinestFESpace();
    const int nE = nd.GetTrueVSize();
    FiniteElementSpace rt(ctx, mesh, PA_FE_HDIV, order, rt_size, i32(b_shared + 4), u8(b_shared + 5), nullptr);

    auto surface = [&](double a) {  // a / R_s on the faces of port 1 (attribute 1) and port 2 (attribute 2)
      std::vector<double> m(18, 0.0);
      for (int k = 0; k < 2; k++)
        for (int d = 0; d < 3; d++) m[9 * k + 4 * d] = a * sc[7 + k];
      return MaterialPropertyCoefficient(std::vector<int>{0, 1}, 3, m);
    };
    auto volume = [&](double v) {
      MaterialPropertyCoefficient c(1);
      c.AddMaterialProperty(1, v);
      return c;
    };
    auto wrap = [&](std::unique_ptr<Operator> &&op, const FiniteElementSpace &fes, ParOperator::DiagonalPolicy policy) {
      auto par = std::make_unique<FespaceParOperator>(std::move(op), fes);
      par->SetEssentialTrueDofs(fes.GetEssentialTrueDofs(), policy);
      return par;
    };
    const MaterialPropertyCoefficient muinv = volume(muinv_v), eps = volume(eps_v), sigma = volume(sigma_v), inv_rs = surface(1.0);
    BilinearForm k(nd), m(nd), c(nd), mrt(rt);
    k.AddDomainIntegrator<CurlCurlIntegrator>(muinv);
    m.AddDomainIntegrator<VectorFEMassIntegrator>(eps);
    c.AddDomainIntegrator<VectorFEMassIntegrator>(sigma);
    c.AddBoundaryIntegrator<VectorFEMassIntegrator>(*nd_bdr.back(), inv_rs);
    mrt.AddDomainIntegrator<VectorFEMassIntegrator>(muinv);
    auto K = wrap(k.PartialAssemble(), nd, ParOperator::DiagonalPolicy::DIAG_ZERO);
    auto C = wrap(c.PartialAssemble(), nd, ParOperator::DiagonalPolicy::DIAG_ZERO);
    auto M = wrap(m.PartialAssemble(), nd, ParOperator::DiagonalPolicy::DIAG_ONE);
    auto M_eps = m.PartialAssemble();  // the unconstrained masses the energies are measured with
    auto M_mu = mrt.PartialAssemble();
    const Operator &Curl = rt.GetDiscreteInterpolator(nd);

    // M^-1: Jacobi-preconditioned CG (models/timeoperator.cpp:79-88)
    auto pcg = std::make_unique<CgSolver>(ctx, 0);
    pcg->SetTol(tol), pcg->SetAbsTol(2.220446049250313e-16), pcg->SetMaxIter(max_it);
    KspSolver kspM(std::move(pcg), std::make_unique<JacobiSmoother>(ctx));
    kspM.SetOperators(*M, *M);

    config::LinearSolverData linear;
    linear.krylov_solver = KrylovSolver::CG;
    linear.type = LinearSolver::JACOBI_PCG;
    linear.tol = tol, linear.max_it = max_it;
    linear.SetDefaults(order, /*spd_problem=*/true);
    std::unique_ptr<MultigridOperator> A;
    std::unique_ptr<KspSolver> kspA;
    TimeOperator *top = nullptr;
    int rebuilds = 0;
    auto configure = [&](double a) {
      // A(a) on every level; the coefficients live until the forms are assembled
      const MaterialPropertyCoefficient a2_muinv = volume(a * a * muinv_v), mass = volume(eps_v + a * sigma_v), a_rs = surface(a);
      auto ops = std::make_unique<MultigridOperator>(nd_fespaces.GetNumLevels());
      for (std::size_t l = 0; l < nd_fespaces.GetNumLevels(); l++) {
        const auto &fes = nd_fespaces.GetFESpaceAtLevel(l);
        BilinearForm f(fes);
        f.AddDomainIntegrator<CurlCurlMassIntegrator>(a2_muinv, mass);
        f.AddBoundaryIntegrator<VectorFEMassIntegrator>(*nd_bdr[l], a_rs);
        ops->AddOperator(wrap(f.PartialAssemble(), fes, ParOperator::DiagonalPolicy::DIAG_ONE));
      }
      if (!kspA) kspA = std::make_unique<KspSolver>(linear, /*verbose=*/0, nd_fespaces);
      kspA->SetOperators(*ops, *ops);
      A = std::move(ops);
      top->SetLinearSolver(*kspA);
      rebuilds++;
    };
    Vector negJ(nE), v1(nE), v2(nE), tE(nE), tB(rt_size);
    hipMemcpy(negJ.Data(), f64(b_shared + 6), sizeof(double) * nE, hipMemcpyHostToDevice);
    hipMemcpy(v1.Data(), f64(b_shared + 7), sizeof(double) * nE, hipMemcpyHostToDevice);
    hipMemcpy(v2.Data(), f64(b_shared + 8), sizeof(double) * nE, hipMemcpyHostToDevice);
    auto dJ = [=](double t) { return PulseDerivative(/*modulated Gaussian*/ 3, omega, tau, t0, t); };
    TimeOperator time_op(ctx, K.get(), C.get(), M.get(), Curl, negJ, dJ, rho_inf, kspM, configure);
    top = &time_op;

    auto measure = [&](int step, double t) {
      const Vector &E = time_op.GetE(), &B = time_op.GetB();
      M_eps->Mult(E, tE);
      M_mu->Mult(B, tB);
      std::printf("step %d t %.15e V1 %.15e V2 %.15e E_elec %.15e E_mag %.15e\n", step, t, volts * linalg::Dot(ctx, v1, E),
                  volts * linalg::Dot(ctx, v2, E), 0.5 * joules * linalg::Dot(ctx, E, tE), 0.5 * joules * linalg::Dot(ctx, B, tB));
    };
    double t = 0.0;
    time_op.Init();
    measure(0, t);
    for (int step = 1; step <= nsteps; step++) {
      time_op.Step(t, dt);
      measure(step, t);
    }
    time_op.PrintStats();
    const auto &st = time_op.GetStats();
    const KspSolver &used = time_op.GetLinearSolver();
    std::printf("stats: steps %lld k %lld c %lld curl %lld a_solves %lld m_solves %lld ew %lld configures %lld rebuilds %d "
                "ksp_mult %d ksp_its %d same_solver %d\nOK\n",
                st.steps, st.k_applies, st.c_applies, st.curl_applies, st.a_solves, st.m_solves, st.ew_launches, st.configures,
                rebuilds, used.NumTotalMult(), used.NumTotalMultIterations(), (int)(&used == kspA.get()));
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
