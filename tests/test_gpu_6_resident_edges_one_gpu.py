"""The resident solves of the block-column driver with PEERS on the one GPU a test box has: two and three ranks, gloo
for the collectives (RCCL refuses two ranks on one device), everything else the product -- HipBlockOps, csrc/dist.hip
through the C ABI -- at every block edge of ``tests/_block_column_cases.py``.  The only place where these run on the
device: a rank that owns NO block column (N = 100 and 128 at both world sizes, N = 129 at world 3, the gradient's
N = 300 in blocks of 256 at world 3), owners that alternate under the local-column offsets ``k / G`` into the factor,
``xloc`` and ``yloc``, ``tgp_dist_gather_owned``, and chunks of K^-1 whose ``first`` / ``stop`` block lies away from
block 0 and belongs to another rank.  One spawn per world size runs the whole case list (at most three processes hold
the GPU); every rank's results are held to the references and, to the bit, to rank 0's."""
import functools
import os
import sys
from pathlib import Path

import pytest

import _block_column_cases as bc

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


def _worker(rank, world, port, q):
    sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), LOCAL_RANK="0")
    import torch
    import torch.distributed as dist

    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import _block_column_cases as cases
        from tinygp_amd.distributed import BlockCyclicCholesky, HipBlockOps

        def make(kernel, X, diag, nb):
            return BlockCyclicCholesky(kernel, X, diag, nb=nb, ops=HipBlockOps(0), dist=dist)

        q.put((rank, cases.run_all(make)))
    finally:
        dist.destroy_process_group()


@functools.lru_cache(maxsize=None)
def _results(world):
    """{case: [rank 0's results, rank 1's, ..]} -- one spawn per world size."""
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29950 + (os.getpid() % 200)
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    [p.start() for p in procs]
    out = [o for _, o in sorted((q.get(timeout=300) for _ in range(world)), key=lambda t: t[0])]
    [p.join(60) for p in procs]
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    return {c: [o[c] for o in out] for c in bc.CASES + bc.GRAD_CASES}


@pytest.mark.parametrize("case", bc.CASES, ids=bc.case_id)
@pytest.mark.parametrize("world", [2, 3])
def test_resident_solves_at_every_block_edge_with_peers(world, case):
    led = bc.check(case, world, _results(world)[case], on_device=True)
    print(led.line(f"{bc.case_id(case)} world {world}"))


@pytest.mark.parametrize("case", bc.GRAD_CASES, ids=bc.case_id)
@pytest.mark.parametrize("world", [2, 3])
def test_gradient_chunks_at_every_block_edge_with_peers(world, case):
    led = bc.check_grad(case, world, _results(world)[case])
    print(led.line(f"{bc.case_id(case)} world {world}"))
