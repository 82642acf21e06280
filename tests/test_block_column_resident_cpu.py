"""The resident-solve sweep of ``_block_column_cases.py`` without a GPU: the block-column driver's own Python -- block
ownership, ``first`` / ``stop``, the chunking of test points and of K^-1 columns, the transposed read-back of the Gram
blocks -- on the NumPy stand-in for the per-rank operations under gloo, at world sizes 1 (in this process), 2 and 3 (one
spawn each: the workers run the whole case list and return their arrays, the parent asserts).  The same cases,
references and bars as the two GPU files, so that what those hold the device to is known to be sound first."""
import contextlib
import functools
import os
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest

import _block_column_cases as bc
import _dense_grad_np as dg
import _dense_np as dn

ROOT = Path(__file__).resolve().parent.parent


def _make(dist):
    from _numpy_blockops import NumpyBlockOps
    from tinygp_amd.distributed import BlockCyclicCholesky

    return lambda kernel, X, diag, nb: BlockCyclicCholesky(kernel, X, diag, nb=nb, ops=NumpyBlockOps(), dist=dist)


def _worker(rank, world, port, q):
    sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1")
    import torch.distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import _block_column_cases as cases

        q.put((rank, cases.run_all(_make(dist))))
    finally:
        dist.destroy_process_group()


@contextlib.contextmanager
def _one_blas_thread():
    """The in-process run on one BLAS thread where the pools can be told (a matter of speed alone)."""
    import torch

    keep = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        try:
            from threadpoolctl import threadpool_limits
        except ImportError:
            yield
        else:
            with threadpool_limits(limits=1):
                yield
    finally:
        torch.set_num_threads(keep)


@functools.lru_cache(maxsize=None)
def _results(world):
    """{case: [rank 0's results, rank 1's, ..]} -- computed once per world size."""
    if world == 1:
        import torch.distributed as dist

        with tempfile.TemporaryDirectory() as tmp, _one_blas_thread():
            dist.init_process_group("gloo", init_method=f"file://{tmp}/store", rank=0, world_size=1)
            try:
                out = [bc.run_all(_make(dist))]
            finally:
                dist.destroy_process_group()
    else:
        import torch.multiprocessing as mp

        ctx = mp.get_context("spawn")
        q = ctx.Queue()
        port = 33500 + (os.getpid() % 2000)
        procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
        # one BLAS thread per rank, set where the children inherit it (they import numpy before _worker runs): the
        # products are a block wide, and thread pools of several ranks spinning against each other cost 20x the work
        keep = {k: os.environ.get(k) for k in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS")}
        os.environ.update(OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1")
        try:
            [p.start() for p in procs]
        finally:
            for k, v in keep.items():
                os.environ.pop(k, None) if v is None else os.environ.update({k: v})
        out = [o for _, o in sorted((q.get(timeout=600) for _ in range(world)), key=lambda t: t[0])]
        [p.join(60) for p in procs]
        assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    return {c: [o[c] for o in out] for c in bc.CASES + bc.GRAD_CASES}


def test_the_sweep_reaches_every_block_edge():
    """The shapes: one ragged block, exactly one, a last block of one row, blocks of two and four tiles, ranks without
    a block column, chunks of K^-1 that start inside a block and at blocks 4 and 8."""
    shapes = {(n, nb) for n, nb, _ in bc.CASES}
    assert {(100, 128), (128, 128), (129, 128), (257, 128), (300, 128), (1100, 128), (1100, 256), (1100, 512)} <= shapes
    assert {n for n, _, _ in bc.CASES} <= set(dn.NS)  # no N of this sweep is new to _dense_np
    assert bc.nblocks(100, 128) < 2 and bc.nblocks(129, 128) < 3  # a rank with nloc = 0 at world 2, and at world 3
    for name, n, nb, chunk in bc.GRAD_CASES:
        firsts = [c0 // nb for c0 in range(0, n, chunk)]
        assert (nb == 256 and chunk == 128 and any(c0 % nb for c0 in range(0, n, chunk))) or \
               (nb == 128 and chunk == 512 and firsts == [0, 4, 8])
    assert {n for _, n, _, _ in bc.GRAD_CASES} == {300, 1100}
    assert {r % 128 for r in bc.R_WIDTHS} >= {0, 1, 127} and max(bc.R_WIDTHS) > 256
    assert (300, 128, "float32") in bc.CASES


@pytest.mark.parametrize("n,dtype", sorted({(n, dt) for n, _, dt in bc.CASES}))
def test_the_references_meet_their_conditions(n, dtype):
    """``check_factor`` on the float64 reference (in ``reference``) and ``check_cross`` (in ``cross_refs`` and
    ``conditional``) at every N and every number of test points of the sweep, for both kernels."""
    dn.reference(n, bc.D, dtype)
    for m in sorted(set(bc.VAR_MS) | set(bc.GRAM_MS)):
        for other in (False, True):
            var, gram, Kss = bc.cross_refs(n, dtype, m, other)
            np.testing.assert_allclose(np.diag(gram), var, rtol=1e-13)
            C = dn.conditional(bc.D, n, m, True, False, other, dtype)[0]
            np.testing.assert_allclose(Kss - gram, C, rtol=0, atol=1e-13 * np.abs(Kss).max())
    fwd, bwd = bc.solve_refs(n, dtype)
    ref = dn.reference(n, bc.D, dtype)
    Y = dn.rhs(n, dtype)[:, :max(bc.R_WIDTHS)].astype(np.float64)
    np.testing.assert_allclose(ref.L @ fwd, Y, rtol=0, atol=1e-11 * np.abs(fwd).max())
    np.testing.assert_allclose(ref.L.T @ bwd, Y, rtol=0, atol=1e-11 * np.abs(bwd).max())
    ll, rll, alpha, mean = bc.vector_refs(n, dtype)
    np.testing.assert_allclose(ref.K @ alpha, bc.other_resid(n, dtype).astype(np.float64), rtol=0, atol=1e-9)
    assert np.isfinite(ll) and np.isfinite(rll) and mean.shape == (bc.MEAN_M,)


@pytest.mark.parametrize("case", bc.GRAD_CASES, ids=bc.case_id)
def test_the_gradient_reference_meets_its_conditions(case):
    name, n, nb, chunk = case
    ref = dg.reference(name, n)  # asserts cond(K), the two routes and the weight of every tile of K^-1
    assert ref.min_tile >= dg.WEIGHT_FACTOR["float64"]


@pytest.mark.parametrize("case", bc.CASES, ids=bc.case_id)
@pytest.mark.parametrize("world", bc.WORLDS)
def test_resident_solves_at_every_block_edge_on_the_stand_in(world, case):
    led = bc.check(case, world, _results(world)[case], on_device=False)
    print(led.line(f"{bc.case_id(case)} world {world}"))


@pytest.mark.parametrize("case", bc.GRAD_CASES, ids=bc.case_id)
@pytest.mark.parametrize("world", bc.WORLDS)
def test_gradient_chunks_at_every_block_edge_on_the_stand_in(world, case):
    led = bc.check_grad(case, world, _results(world)[case])
    print(led.line(f"{bc.case_id(case)} world {world}"))
