"""The C++ front end on a mesh with hanging nodes across ranks: examples/cxx_host/solve_nc_ranks.cpp (FiniteElementSpace with a
halo taking SetConformingProlongation with n_shared, so that every FespaceParOperator and prolongation applies P = [I; C] P_halo;
KspSolver with PCG + p-multigrid and Jacobi-PCG at level 0) as two processes sharing the GPU over the peer transport, on the
dump of the refined cylinder at orders [1, 2], against solve_nc.cpp on one rank: iterations +-1, checksum 1e-6 (the gates of
tests/test_cxx_host_gpu.py)."""
import os
import re
import shutil
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.path.join(ROOT, "examples", "cxx_host")
LINE = r"ndofs (\d+)\s+constrained (?:on rank 0 )?(\d+) .* iterations (\d+)\s+converged (\d)\s+\|b - A x\| / \|b\| (\S+)\s+sum\(x\) (\S+)"


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    d = tmp_path_factory.mktemp("cxx_nc_ranks")
    libdir = os.path.join(ROOT, "palace_amd", "lib")
    exes = {}
    for name in ("solve_nc", "solve_nc_ranks"):
        exes[name] = str(d / name)
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O2", "-w", "-I" + os.path.join(ROOT, "palace_amd", "csrc"),
                               "-I" + os.path.join(ROOT, "include"), os.path.join(CXX, name + ".cpp"), "-L" + libdir, "-lpalace_amd",
                               "-Wl,-rpath," + libdir, "-o", exes[name]])
    blob = str(d / "problem.bin")
    subprocess.check_call([sys.executable, os.path.join(CXX, "dump_nc_problem.py"), blob, "2"])
    for world in (1, 2):
        subprocess.check_call([sys.executable, os.path.join(CXX, "dump_nc_problem_ranks.py"), str(d / f"ranks{world}"), str(world), "2"])
    return exes, blob, d


def _run_ranks(exe, d, world, coarse, tag):
    """`world` fresh child processes, each with a time limit of its own; ends at the first non-zero exit."""
    hd = d / f"handles_{tag}"
    hd.mkdir()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PALACE_AMD_PEER_TIMEOUT_S="30")
    procs = [subprocess.Popen([exe, str(d / f"ranks{world}"), str(r), str(world), str(hd), coarse], env=env, stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE) for r in range(world)]
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=120))
            if p.returncode != 0:
                break
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.communicate()
    return [p.returncode for p in procs], outs


def _parse(out):
    m = re.search(LINE, out)
    assert m, out
    n, ncon, its, conv = (int(m.group(i)) for i in range(1, 5))
    return n, ncon, its, conv, float(m.group(5)), float(m.group(6))


def test_cxx_nc_two_processes_match_one_rank(built):
    exes, blob, d = built
    one = subprocess.check_output([exes["solve_nc"], blob, "pcg"], text=True, timeout=120)
    n1, ncon1, its1, conv1, res1, sx1 = _parse(one)
    assert conv1 == 1 and ncon1 > 0
    rcs, outs = _run_ranks(exes["solve_nc_ranks"], d, 2, "pcg", "two")
    assert rcs == [0, 0], (rcs, [o[1].decode()[-600:] for o in outs])
    two = outs[0][0].decode()
    n2, ncon2, its2, conv2, res2, sx2 = _parse(two)
    print(one.strip(), "|", two.strip())
    assert conv2 == 1 and res2 < 1e-8 and n2 == n1, two
    assert abs(its2 - its1) <= 1, (one, two)
    assert abs(sx2 - sx1) < 1e-6 * abs(sx1), (one, two)


def test_cxx_nc_ranks_one_process_and_amg_refusal(built):
    """world = 1 through the same driver (no halo, n_shared == n_true) gives solve_nc's numbers; BOOMER_AMG on a level whose
    conforming prolongation is the distributed object is refused with a clear message."""
    exes, blob, d = built
    n1, _, its1, conv1, _, sx1 = _parse(subprocess.check_output([exes["solve_nc"], blob, "pcg"], text=True, timeout=120))
    rcs, outs = _run_ranks(exes["solve_nc_ranks"], d, 1, "pcg", "one")
    assert rcs == [0], outs[0][1].decode()[-600:]
    n, ncon, its, conv, res, sx = _parse(outs[0][0].decode())
    assert conv == 1 and n == n1 and ncon > 0 and abs(its - its1) <= 1 and abs(sx - sx1) < 1e-6 * abs(sx1)
    rcs, outs = _run_ranks(exes["solve_nc_ranks"], d, 1, "amg", "amg")
    err = outs[0][1].decode()
    assert rcs == [1] and "across ranks" in err and "halo" in err and "JACOBI_PCG" in err, err
