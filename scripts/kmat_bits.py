#!/usr/bin/env python
"""Every output of the dense path's kernel evaluation (csrc/kmat.hip) on a fixed, seeded case list, for bit-for-bit
comparison of two builds.

    python scripts/kmat_bits.py dump FILE.npz
    python scripts/kmat_bits.py compare A.npz B.npz

`dump` runs the cases on the device with whatever `libtgp_hip.so` the package loads (`TGP_HIP_LIBRARY` names another
build) and stores every array.  `compare` requires `np.array_equal` on every array (NaNs equal where both have one)
and exits non-zero on the first difference, naming the array.  Run both dumps on the same machine.

Cases, per dtype (float64, float32), program and input dimension d in {1, 3, 7} (d <= 3 takes the straight-line
assembly kernel for the fast programs, d = 7 the general one): fast L1 and L2 leaves with and without an amplitude, a
general exp-family sum, a family-0 program (`RationalQuadratic * Cosine`) and a family-2 program
(`DotProduct` + `Polynomial`).  Per case: `K(X1, X2)` at (129, 127) and (300, 300); `K(X, X)` plus a noise diagonal
at 256 and 300; the kernel diagonal; `matmul` with 1, 8 and 9 vectors at (257, 513); and everything
`log_probability_and_grad` returns at N = 127, 128, 129, 300, 640.  Per dtype: gradients through `transforms.Linear`
(d = 3, N = 300) and the block-column gradient at world size 1 with N = 300, nb = 128, GRAD_CHUNK = 128.

For d > 1, and for the family-2 program, the noise diagonal of a gradient case is raised, row by row, by the excess of
the row's off-diagonal absolute sum over its diagonal entry (taken from the device's own K): several of these kernels
are not positive definite on the L1 distance in more than one dimension, the polynomial is too ill-conditioned for a
float32 factorisation, and a failed factorisation would compare NaN with NaN.
"""
import ctypes as C
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

DTYPES = ("float64", "float32")
DIMS = (1, 3, 7)
GRAD_SIZES = (127, 128, 129, 300, 640)


def programs(k):
    l2 = k.L2Distance()
    return {
        "exp_l1": k.Exp(1.3),
        "amp_m32_l1": 1.8 * k.Matern32(1.5),
        "expsq_l2": k.ExpSquared(1.7),
        "amp_m52_l2": 0.9 * k.Matern52(1.1, distance=l2),
        "expfam_sum": 1.5**2 * k.ExpSquared(2.5) + 0.3 * k.Matern32(1.2),
        "fam0_rq_cos": k.RationalQuadratic(1.1, alpha=0.8) * k.Cosine(3.0),
        "fam2_dot_poly": 0.3 * k.DotProduct() + k.Polynomial(order=2, scale=8.0, sigma=0.5),
    }


def points(rng, n, d, dtype):
    X = np.sort(rng.uniform(0, max(n, 40) / 40.0, n)) if d == 1 else rng.uniform(0, 3, (n, d))
    return X.astype(dtype)


def kmat_noise(prog, P, diag):
    """K(X, X) + diag through tgp_kmat's fused noise diagonal, (n, n) as the device wrote it."""
    from tinygp_amd import _ffi

    ctx = _ffi.default_ctx()
    dt = P.dtype
    n, d = P.shape
    kp, nops = _ffi.as_kprog(prog)
    dX, dd = ctx.upload(P), ctx.upload(np.ascontiguousarray(diag, dtype=dt))
    out = ctx.malloc(n * n * dt.itemsize)
    try:
        _ffi.check(_ffi.lib().tgp_kmat(ctx.handle, _ffi.dtype_code(dt), kp, nops, n, n, d, C.c_void_p(dX),
                                       C.c_void_p(dX), C.c_void_p(dd), C.c_void_p(out), n, n, n, 0), "tgp_kmat")
        return ctx.download(out, (n, n), dt)
    finally:
        ctx.free(dX), ctx.free(dd), ctx.free(out)


def put_grad(out, tag, ll, g):
    out[tag + "ll"] = np.asarray(ll)
    out[tag + "kernel"] = np.asarray(g["kernel"], dtype=np.float64)
    out[tag + "noise_diag"] = np.asarray(g["noise_diag"])
    out[tag + "mean"] = np.asarray(g["mean"])
    if g.get("transform") is not None:
        out[tag + "transform"] = np.asarray(g["transform"], dtype=np.float64)


def safe_diag(K, noise):
    """noise, raised so that K + diag is strictly diagonally dominant"""
    K = np.abs(K.astype(np.float64))
    excess = K.sum(axis=1) - 2 * np.diag(K)
    return (noise + np.maximum(excess, 0.0)).astype(noise.dtype)


def run_case(name, d, dtype, seed, out):
    from tinygp_amd import GaussianProcess, _device, kernels

    rng = np.random.default_rng(seed)
    k = programs(kernels)[name]
    tag = f"{dtype}/{name}/d{d}/"

    def lower(X):
        prog, P = k._lower(X)
        return prog, _device.points(P, X.dtype)

    for n1, n2 in ((129, 127), (300, 300)):
        X1, X2 = points(rng, n1, d, dtype), points(rng, n2, d, dtype)
        prog, P1 = lower(X1)
        out[tag + f"K_{n1}x{n2}"] = _device.kmat(prog, P1, lower(X2)[1])
    for n in (256, 300):
        X = points(rng, n, d, dtype)
        prog, P = lower(X)
        out[tag + f"Knoise_{n}"] = kmat_noise(prog, P, rng.uniform(0.05, 0.15, n))
        out[tag + f"diag_{n}"] = _device.kdiag(prog, P)
    X1, X2 = points(rng, 257, d, dtype), points(rng, 513, d, dtype)
    prog, P1 = lower(X1)
    V = rng.standard_normal((513, 9)).astype(dtype)
    for nv in (1, 8, 9):
        out[tag + f"matmul_{nv}"] = _device.kmat_gemv(prog, P1, lower(X2)[1], V[:, 0] if nv == 1 else V[:, :nv])
    for n in GRAD_SIZES:
        X = points(rng, n, d, dtype)
        y = (np.sin(X if d == 1 else X[:, 0]) + 0.1 * rng.standard_normal(n)).astype(dtype)
        noise = rng.uniform(0.05, 0.15, n).astype(dtype)
        if d > 1 or name.startswith("fam2"):
            prog, P = lower(X)
            noise = safe_diag(_device.kmat(prog, P, P), noise)
        gp = GaussianProcess(k, X, diag=noise)
        ll, g = gp.log_probability_and_grad(y)
        out[tag + f"grad_{n}/info"] = np.asarray(gp.solver.info)
        put_grad(out, tag + f"grad_{n}/", ll, g)


def run_linear(dtype, seed, out):
    from tinygp_amd import GaussianProcess, kernels, transforms

    rng = np.random.default_rng(seed)
    n, d = 300, 3
    X = points(rng, n, d, dtype)
    y = (np.sin(X[:, 0]) + 0.3 * np.cos(2 * X[:, 1]) + 0.1 * rng.standard_normal(n)).astype(dtype)
    noise = rng.uniform(0.05, 0.15, n).astype(dtype)
    s = np.array([0.5, 2.0, 1.3])
    trees = {
        "linear_expsq": 1.5 * transforms.Linear(s, kernels.ExpSquared(1.2)),
        "linear_poly": transforms.Linear(s, 0.8 * kernels.ExpSquared(1.2)
                                         + kernels.Polynomial(order=2, scale=8.0, sigma=0.5)),
    }
    for name, k in trees.items():
        gp = GaussianProcess(k, X, diag=noise)
        ll, g = gp.log_probability_and_grad(y)
        out[f"{dtype}/{name}/info"] = np.asarray(gp.solver.info)
        put_grad(out, f"{dtype}/{name}/", ll, g)


def run_block_column(dist, dtype, seed, out):
    from tinygp_amd import kernels
    from tinygp_amd.distributed import BlockCyclicCholesky

    rng = np.random.default_rng(seed)
    n = 300
    X = points(rng, n, 1, dtype)
    y = (np.sin(X) + 0.1 * rng.standard_normal(n)).astype(dtype)
    noise = rng.uniform(0.05, 0.15, n).astype(dtype)
    for name in ("expfam_sum", "fam2_dot_poly"):
        s = BlockCyclicCholesky(programs(kernels)[name], X, noise, nb=128, dist=dist)
        s.GRAD_CHUNK = 128
        ll, g = s.log_probability_and_grad(y)
        put_grad(out, f"{dtype}/block_column/{name}/", ll, g)
        s.ops.close()


def dump(path):
    import torch
    import torch.distributed as dist

    from tinygp_amd import kernels

    out = {}
    seed = 500
    for dtype in DTYPES:
        for name in programs(kernels):
            for d in DIMS:
                seed += 1
                run_case(name, d, dtype, seed, out)
            print(f"{dtype} {name}: done", flush=True)
        run_linear(dtype, seed + 1000, out)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29655")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        for dtype in DTYPES:
            run_block_column(dist, dtype, 77, out)
    finally:
        dist.destroy_process_group()
    bad = sorted(key for key, a in out.items() if a.dtype.kind == "f" and not np.all(np.isfinite(a)))
    print(f"{len(bad)} arrays with a non-finite entry" + (f": {bad[:8]}" if bad else ""))
    np.savez(path, **out)
    print(f"{len(out)} arrays -> {path}")


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    if sorted(a.files) != sorted(b.files):
        print(f"different sets of arrays: {sorted(set(a.files) ^ set(b.files))}")
        return 1
    for key in sorted(a.files):
        x, y = a[key], b[key]
        if x.shape != y.shape or x.dtype != y.dtype or not np.array_equal(x, y, equal_nan=x.dtype.kind == "f"):
            where = ""
            if x.shape == y.shape and x.size:
                bad = np.flatnonzero(~((x == y) | ((x != x) & (y != y))).ravel())
                where = f": {bad.size} of {x.size} entries, first at flat index {bad[0]}"
            print(f"DIFFERENT {key}{where}")
            return 1
    print(f"{len(a.files)} arrays bit-identical")
    return 0


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
        return 0
    if len(sys.argv) == 4 and sys.argv[1] == "compare":
        return compare(sys.argv[2], sys.argv[3])
    print(__doc__)
    return 2


if __name__ == "__main__":
    sys.exit(main())
