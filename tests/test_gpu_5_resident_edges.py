"""The resident solves of the block-column driver through the REAL per-rank operations (HipBlockOps: csrc/dist.hip
through the C ABI) at world size 1, every collective an RCCL self-collective, at every block edge of
``tests/_block_column_cases.py``: one ragged block, exactly one block, a last block of one row, three and nine blocks
of one tile, blocks of two and four tiles -- every width of right-hand sides and test points on both sides of the
128-column padding, both forms of the forward solve, chunked and unchunked test points and K^-1 columns -- against the
LAPACK and long-double references of ``_dense_np.py`` / ``_dense_grad_np.py`` at the dense solver's bars.  One solver
per case, factored once; no panel is factored again.  (``test_block_column_resident_cpu.py`` runs the same cases on
the stand-in first; ``test_gpu_6_resident_edges_one_gpu.py`` runs them with peers.)"""
import os

import pytest

import _block_column_cases as bc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pg():
    import torch
    import torch.distributed as dist

    keep = {k: os.environ.get(k) for k in ("MASTER_ADDR", "MASTER_PORT")}
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29617")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    yield dist
    dist.destroy_process_group()
    for k, v in keep.items():
        os.environ.pop(k, None) if v is None else os.environ.update({k: v})


def _make(dist):
    from tinygp_amd.distributed import BlockCyclicCholesky

    return lambda kernel, X, diag, nb: BlockCyclicCholesky(kernel, X, diag, nb=nb, dist=dist)


@pytest.mark.parametrize("case", bc.CASES, ids=bc.case_id)
def test_resident_solves_at_every_block_edge_hip(pg, case):
    res = bc.drive(_make(pg), *case)  # (closes the solver's communicator, then its operations)
    led = bc.check(case, 1, [res], on_device=True)
    print(led.line(f"{bc.case_id(case)} world 1"))


@pytest.mark.parametrize("case", bc.GRAD_CASES, ids=bc.case_id)
def test_gradient_chunks_at_every_block_edge_hip(pg, case):
    """Chunks of K^-1 that start inside a block column (GRAD_CHUNK 128 in blocks of 256) and at blocks 4 and 8
    (GRAD_CHUNK 512 in blocks of 128): ``first`` / ``stop`` of the forward and backward solves away from block 0."""
    res = bc.drive_grad(_make(pg), *case)
    led = bc.check_grad(case, 1, [res])
    print(led.line(f"{bc.case_id(case)} world 1"))
