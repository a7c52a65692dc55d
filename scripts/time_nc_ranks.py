"""What a hanging-node space costs across ranks: the mesh of scripts/time_conform.py (an O-grid cylinder of about --elements
elements, the elements inside a ball that holds about --fraction of them refined once; 172 380 leaves at the defaults) at order
3, cut by recursive coordinate bisection over --world processes that SHARE ONE GPU (peer transport, as tests/test_peer_gpu.py).
Per rank, device events after warm-up:
  * ParOperator::Mult with the Conforming that carries the halo (P = [I; C] P_halo, local apply, P^T);
  * the whole of P and of P^T;
  * their three pieces each (pa_conform_time_pieces): masked copy, halo exchange, rows of C; fold, halo exchange, epilogue.
    The exchange pieces include the wait for the other rank.
The ranks share the GPU, so every figure is taken while the other rank runs the same piece on the same device; set beside the
one-rank figures of profiles/r16_conform.json they are an upper bound of what a rank with a GPU of its own would see.
Writes profiles/r19_nc_ranks.json (or --out)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402


def _worker(rank, args):
    import torch
    import torch.distributed as dist

    world = args.world
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(args.port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)  # every rank on the same GPU
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from palace_amd import ceed, linalg
        from palace_amd.fem import nchex, rcb
        from palace_amd.fem.fespace import NDHexSpace
        from palace_amd.fem.mesh import ogrid_cylinder
        from palace_amd.fem.ncpart import PartitionedNCSpace
        from tests import util

        p = args.order
        n = max(1, int(round((args.elements / (5 * 1.2)) ** (1.0 / 3.0))))
        nz = max(1, int(round(args.elements / (5 * n * n))))
        t0 = time.perf_counter()
        m0 = ogrid_cylinder(n, nz)
        ctr = m0.x[m0.elem_nodes[:, 13]]
        lo, hi = m0.bounding_box()
        d = np.linalg.norm(ctr - 0.5 * (lo + hi) - np.array([0.3, 0.2, 0.1]) * (hi - lo), axis=1)
        marked = np.argsort(d, kind="stable")[: int(round(args.fraction * m0.ne))]
        mesh = nchex.refine_local(m0, marked)
        s = nchex.NCSpace(NDHexSpace(mesh, p))
        part = rcb.rcb(mesh.x[mesh.elem_nodes[:, 13]], world)
        v = PartitionedNCSpace(s, part, rank, world)
        res = dict(rank=rank, elements=int(v.mesh.ne), n_true=int(v.n_true), n_shared=int(v.n_shared), n_local=int(v.n_local),
                   dependency_only_ghosts=int(v.n_dep), nnz_C=int(v.C.nnz), neighbours=len(v.nbr),
                   host_setup_s=round(time.perf_counter() - t0, 1))
        print(res, flush=True)

        ctx = linalg.Context()
        if world > 1:
            ctx.init_comm_peer_from_torch_distributed()
        halo = linalg.Halo(ctx, v.nbr, v.send, v.recv) if world > 1 else None
        conf = linalg.Conforming(ctx, v, halo=halo, n_shared=v.n_shared)
        bm, bc = util.make_ctx("scalar")[1], util.make_ctx("identity")[1]
        geom = ceed.GeomFactorData(v.mesh, p + 1)
        local = ceed.curlcurlmass_operator(geom, v, bm, bc)
        A = linalg.ParOperator(ctx, local, v.ess_dofs(), linalg.DIAG_ONE, conforming=conf)
        res["lanes"], res["lanes_T"] = conf.lanes(), conf.lanes(True)

        def new(k):
            return torch.rand(k, dtype=torch.float64, device="cuda")

        xt, yt, xl, yl = new(v.n_true), new(v.n_true), new(v.n_local), new(v.n_local)
        mask = torch.zeros(v.n_true, dtype=torch.uint8, device="cuda")
        mask[torch.from_numpy(v.ess_dofs().astype(np.int64)).cuda()] = 1
        forms = {
            "mult": lambda: A.mult(xt, yt),
            "prolongate": lambda: conf.prolongate(xt, xl, mask),
            "restrict": lambda: conf.restrict(yl, yt, conf.FIX_ONE, 1.0, mask, xt),
            "local_apply": lambda: local.mult(xl, yl),
        }
        for f in forms.values():  # (every rank runs the same sequence: the exchanges are collective)
            for _ in range(20):
                f()
        times = {k: [] for k in forms}
        with torch.cuda.stream(ctx.torch_stream):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(5):
                for k, f in forms.items():
                    torch.cuda.synchronize()
                    dist.barrier()
                    e0.record()
                    for _ in range(args.reps):
                        f()
                    e1.record()
                    torch.cuda.synchronize()
                    times[k].append(e0.elapsed_time(e1) / args.reps * 1e3)
        res["us"] = {k: dict(median=round(float(np.median(t)), 2), min=round(min(t), 2), max=round(max(t), 2)) for k, t in times.items()}
        pieces = []
        for _ in range(3):
            dist.barrier()
            pieces.append(conf.time_pieces(xt, xl, yl, yt, mask, args.reps))
        res["pieces_us"] = {k: round(float(np.median([q[k] for q in pieces])), 2) for k in pieces[0]}
        if world > 1:
            ctx.peer_check()
        print(rank, res["us"], res["pieces_us"], flush=True)
        gathered = [None] * world
        dist.all_gather_object(gathered, res)
        if rank == 0:
            one = json.load(open(os.path.join("profiles", "r16_conform.json")))["us"]
            out = dict(world=world, ranks_share_one_gpu=True, order=p, elements=int(mesh.ne), n_true_global=int(s.n_true),
                       n_local_global=int(s.n_local), reps=args.reps, ranks=gathered,
                       one_rank_r16_us=dict(mult=one["mult_constrained"]["median"], prolongate=one["prolongate"]["median"],
                                            restrict=one["restrict"]["median"]))
            os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1)
                f.write("\n")
        dist.barrier()
    finally:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elements", type=float, default=1e5)
    ap.add_argument("--fraction", type=float, default=0.10)
    ap.add_argument("--order", type=int, default=3)
    ap.add_argument("--world", type=int, default=2)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--port", type=int, default=29719)
    ap.add_argument("--out", default=os.path.join("profiles", "r19_nc_ranks.json"))
    args = ap.parse_args()
    import torch.multiprocessing as mp

    mp.spawn(_worker, args=(args,), nprocs=args.world, join=True)


if __name__ == "__main__":
    main()
