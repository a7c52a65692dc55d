// C++ host example on a mesh with hanging nodes, several ranks: solve_nc.cpp's problem with one process per rank (per GPU;
// several per GPU work too), no MPI, no Python at run time.  Each rank reads what Palace's ParMesh / ParFiniteElementSpace hold
// for it after a nonconformal refinement (dump_nc_problem_ranks.py: its elements, and per multigrid level the constrained
// Nedelec space in the local layout owned true dofs | ghost true dofs | constrained dofs, the local constraint matrix and the
// halo plan over the first two ranges), brings up the peer transport of comm.hpp as solve_ranks.cpp does (arena handles through
// files in a shared directory), and builds
//   Mesh, FiniteElementSpaceHierarchy (p = 1 .. order): every space is created with its halo and then handed its constraint
//   (SetConformingProlongation with n_shared), which makes its conforming prolongation the one parallel operator
//   P = [I; C] P_halo of the reference (linalg/rap.cpp:195-234),
//   BilinearForm + CurlCurlMassIntegrator -> Assemble(hierarchy), MultigridOperator, KspSolver (PCG + p-multigrid, Chebyshev
//   smoothers, Jacobi-PCG at level 0),
// solves (K + eps_r M) x = b and prints what solve_nc.cpp prints, with global counts.
//
//   ./solve_nc_ranks prefix rank world dir [coarse=pcg|cheb|jacobi|amg]
// coarse = amg (LinearSolver::BOOMER_AMG) is refused: an assembled level 0 across ranks is not built.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <thread>
#include <vector>

#include "ksp.hpp"

using namespace palace;

static std::vector<std::vector<char>> read_blobs(const std::string &path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) throw pa::Error("cannot open " + path);
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

// the 64-byte arena handles of all ranks through files (rank r writes dir/handle.r, reads the others')
static std::vector<char> exchange_handles(Comm &comm, const std::string &dir, int rank, int world) {
  char mine[Comm::kPeerHandleBytes];
  comm.PeerHandle(mine);
  {
    const std::string tmp = dir + "/handle." + std::to_string(rank) + ".tmp", fin = dir + "/handle." + std::to_string(rank);
    std::ofstream f(tmp, std::ios::binary);
    f.write(mine, sizeof(mine));
    f.close();
    std::rename(tmp.c_str(), fin.c_str());
  }
  std::vector<char> all((size_t)world * Comm::kPeerHandleBytes);
  for (int r = 0; r < world; r++) {
    const std::string path = dir + "/handle." + std::to_string(r);
    for (int tries = 0;; tries++) {
      std::ifstream f(path, std::ios::binary);
      if (f && f.read(&all[(size_t)r * Comm::kPeerHandleBytes], Comm::kPeerHandleBytes)) break;
      if (tries > 6000) throw pa::Error("no arena handle from rank " + std::to_string(r));
      std::this_thread::sleep_for(std::chrono::milliseconds(10));
    }
  }
  return all;
}

int main(int argc, char **argv) {
  if (argc < 5) return 2;
  const std::string prefix = argv[1], dir = argv[4], coarse = argc > 5 ? argv[5] : "pcg";
  const int rank = std::atoi(argv[2]), world = std::atoi(argv[3]);
  try {
    auto blobs = read_blobs(prefix + "." + std::to_string(rank));
    auto i32 = [&](size_t i) { return reinterpret_cast<const int32_t *>(blobs[i].data()); };
    auto f64 = [&](size_t i) { return reinterpret_cast<const double *>(blobs[i].data()); };
    const int ne = i32(0)[0], nn = i32(0)[1], order = i32(0)[2], nlev = i32(0)[3];

    hipStream_t stream;
    if (hipStreamCreate(&stream) != hipSuccess) throw pa::Error("no HIP device");
    Comm comm(rank, world);  // peer transport only
    if (world > 1) {
      const std::vector<char> handles = exchange_handles(comm, dir, rank, world);
      comm.PeerConnect(handles.data());
    }
    Context ctx;
    ctx.stream = stream, ctx.comm = &comm;

    fem::DefaultIntegrationOrder::p_trial = order;
    Mesh mesh(ctx, ne, 2, nn, i32(1), f64(2), i32(3), fem::DefaultIntegrationOrder::GetQ1d(2 * 3 - 1));

    std::vector<std::unique_ptr<Halo>> halos;
    FiniteElementSpaceHierarchy nd_fespaces;
    double constrained = 0.0;
    for (int l = 0; l < nlev; l++) {
      const size_t b = 4 + 13 * (size_t)l;
      const int p = i32(0)[4 + l], n_local = i32(b)[0], n_true = i32(b)[1], n_shared = i32(b)[2];
      const Halo *halo = nullptr;
      if (world > 1) {  // (every rank creates its plans in the same order)
        const int nnbr = (int)(blobs[b + 8].size() / 4);
        halos.push_back(std::make_unique<Halo>(comm, nnbr, i32(b + 8), i32(b + 9), i32(b + 10), i32(b + 11), i32(b + 12)));
        halo = halos.back().get();
      }
      auto nd = std::make_unique<FiniteElementSpace>(ctx, mesh, PA_FE_HCURL, p, n_local, i32(b + 1),
                                                     reinterpret_cast<const uint8_t *>(blobs[b + 2].data()), i32(b + 3), n_true, halo);
      // (int and int32_t are the same type here: the row pointer is stored as int32)
      nd->SetConformingProlongation(n_true, n_shared, reinterpret_cast<const int *>(blobs[b + 5].data()), i32(b + 6), f64(b + 7));
      nd->SetEssentialTrueDofs(i32(b + 4), (int)(blobs[b + 4].size() / 4));
      constrained = n_local - n_shared;
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
    const double rn = linalg::Norml2(ctx, res) / linalg::Norml2(ctx, rhs), sx = linalg::Dot(ctx, x, ones), nglob = linalg::Dot(ctx, ones, ones);
    comm.PeerCheck(stream);
    if (rank == 0)
      std::printf("cxx_host_nc_ranks: world %d  order %d  levels %d  global ndofs %d  constrained on rank 0 %d  coarse %s  iterations %d  "
                  "converged %d  |b - A x| / |b| %.3e  sum(x) %.12e\n",
                  world, order, nlev, (int)std::lround(nglob), (int)constrained, coarse.c_str(), ksp.GetKrylovSolver().GetNumIterations(),
                  (int)ksp.GetKrylovSolver().GetConverged(), rn, sx);
    if (world > 1) comm.Barrier(stream);  // nobody unmaps an arena a neighbour may still store into
  } catch (const std::exception &e) {
    std::fprintf(stderr, "palace_amd (rank %d): %s\n", rank, e.what());  // MFEM_ABORT in Palace
    return 1;
  }
  return 0;
}
