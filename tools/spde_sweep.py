#!/usr/bin/env python3
"""Timing of SPDEGS (gss_spde_create / gss_spde_realize) on device arrays with a warm pool.

  Meshes   grid_1e5 / grid_1e6: triangulated grids of 316^2 and 1000^2 nodes, spacing 1, `range` 10 and 40 spacings;
           sphere_7: an icosphere of 7 subdivisions (163 842 vertices), range 0.05.
  Rows (one JSON line per mesh, range and block width NB; NB is compiled in and chosen by GSS_SPDE_NB, so every NB runs
  in a child process of its own):
    create_ms, sort_ms   gss_spde_create and the share of its radix sort (profile scopes "spde_assemble", "spde_sort")
    iter_us              time per CG iteration of one block: a call with maxiter = 232 minus one with maxiter = 40, both
                         with an rtol no column reaches, over 192
    copy_us, ratio       a device copy that moves the bytes one iteration must move,
                             12 nnz + 16 nv + 8 NB nv * 10
                         (val and col; rowptr and 1/diag; the spmv reads r and p and writes p and Ap, the update reads
                         x, r, p, Ap and writes x, r: ten sweeps of the block), and iter_us / copy_us
    iters, call_ms       iterations to rtol = 1e-10 and the time of a call for 16 realisations (NB = 16 only)
    torch_iter_us        the same CG with torch.sparse_csr products on the same matrix and block (NB = 16 only)
    dense_ms             for scale, at 128^2 = 16 384 vertices: gss_dev_potrf_inverse of the dense precision and one
                         gss_dev_gemm with 16 columns, the reference's method (spde.jl:64-68, 99), beside the CG call

Method: every timed call is warmed `--warmup` times, then measured `--reps` times between events on the stream (the
calls end with a wait, so this is the call as a user sees it); medians, with min .. max.  profiles/spde_sweep.jsonl.
python tools/spde_sweep.py [--reps 5] [--warmup 2] [--small]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "geostatssolvers.jl_amd"), os.path.join(ROOT, "tests")]


def worker(a):
    import numpy as np
    import torch

    import gss
    import spde_ref as R
    from gss import _lib
    from gss.engine import SPDEHandle

    nb = a.worker
    lib = _lib.lib()

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        t = [event_ms(fn) for _ in range(a.reps)]
        return statistics.median(t), min(t), max(t)

    def grid(n):
        m = gss.triangulate(gss.CartesianGrid(n - 1, n - 1))
        return m.vertices, m.triangles

    k = 10 if a.small else 1
    cases = [("grid_1e5", grid(316 // k), 10.0), ("grid_1e5", None, 40.0), ("grid_1e6", grid(1000 // k), 10.0),
             ("grid_1e6", None, 40.0), ("sphere_7", R.icosphere(3 if a.small else 7), 0.05)]
    mesh = None
    for name, m, rng in cases:
        mesh = m or mesh
        V, T = (torch.as_tensor(np.ascontiguousarray(x), device="cuda") for x in mesh)
        row = dict(mesh=name, nv=int(V.shape[0]), nt=int(T.shape[0]), range=rng, NB=nb)
        handles = []

        def create():
            handles.append(SPDEHandle(V, T, sill=1.0, range=rng))
            if len(handles) > 1:
                handles.pop(0).close()
        if nb == 16:
            create()
            _lib.profile_enable(True)
            _lib.profile_reset()
            row["create_ms"] = timed(create)
            ms, n = _lib.profile_read("spde_sort")
            row["sort_ms"] = ms / max(n, 1)
            _lib.profile_enable(False)
        else:
            create()
        h = handles[-1]
        row["nnz"] = h.nnz
        vout = torch.empty((nb, h.nv), dtype=torch.float64, device="cuda")

        def run(n, rtol, maxiter):
            return lib.gss_spde_realize(h._h, 1, 0, n, None, rtol, maxiter, _lib.ptr(vout), None, _lib.MEM_DEVICE,
                                        _lib.current_stream())
        lo, hi = timed(lambda: run(nb, 1e-300, 40)), timed(lambda: run(nb, 1e-300, 232))
        row["iter_us"] = 1e3 * (hi[0] - lo[0]) / 192
        row["fixed_ms"] = [lo, hi]
        nbytes = 12 * h.nnz + 16 * h.nv + 8 * nb * h.nv * 10
        src = torch.empty(nbytes // 16, dtype=torch.float64, device="cuda")
        dst = torch.empty_like(src)
        cp = timed(lambda: [dst.copy_(src) for _ in range(20)])
        row["bytes_per_iter"] = nbytes
        row["copy_us"] = 1e3 * cp[0] / 20
        row["ratio_to_copy"] = row["iter_us"] / row["copy_us"]
        del src, dst
        if nb == 16:
            row["call_ms"] = timed(lambda: _lib.check(run(16, 1e-10, 0)))
            row["iters"] = h.last_solve()[0]
            try:
                rowptr, col, val, _ = h.operator()
                # (torch wants both index arrays of one width and does not check unless asked to)
                S = torch.sparse_csr_tensor(torch.as_tensor(rowptr, device="cuda"),
                                            torch.as_tensor(col.astype(np.int64), device="cuda"),
                                            torch.as_tensor(val, device="cuda"), size=(h.nv, h.nv), check_invariants=True)
                rows = np.repeat(np.arange(h.nv), np.diff(rowptr))
                dinv = 1.0 / torch.as_tensor(val[col == rows], device="cuda")[:, None]
                b = torch.randn((h.nv, 16), dtype=torch.float64, device="cuda")

                def torch_cg(n):
                    x, r = torch.zeros_like(b), b.clone()
                    z = dinv * r
                    p, rho = z.clone(), (r * z).sum(0)
                    for _ in range(n):
                        Ap = S @ p
                        alpha = rho / (p * Ap).sum(0)
                        x += alpha * p
                        r -= alpha * Ap
                        z = dinv * r
                        rho2 = (r * z).sum(0)
                        p = z + (rho2 / rho) * p
                        rho = rho2
                    return x
                t1, t2 = timed(lambda: torch_cg(10)), timed(lambda: torch_cg(60))
                row["torch_iter_us"] = 1e3 * (t2[0] - t1[0]) / 50
                row["torch_ratio"] = row["torch_iter_us"] / row["iter_us"]
            except Exception as e:                         # torch.sparse_csr not usable on this build
                row["torch_error"] = repr(e)[:200]
        print(json.dumps(row), flush=True)
        for x in handles:
            x.close()
        handles.clear()
    if nb == 16:                                           # the reference's method, for scale
        n1 = 128 // k
        Vh, Th = grid(n1)
        n = Vh.shape[0]
        h = SPDEHandle(Vh, Th, sill=1.0, range=10.0)
        rowptr, col, val, mass = h.operator()
        S = torch.zeros((n, n), dtype=torch.float64)
        S[torch.as_tensor(np.repeat(np.arange(n), np.diff(rowptr))), torch.as_tensor(col.astype(np.int64))] = \
            torch.as_tensor(val)
        S = S.cuda()
        A = S / torch.as_tensor(mass, device="cuda")[:, None]
        Q0 = (A.T @ A) / h.tau2
        Q, W = torch.empty_like(Q0), torch.empty_like(Q0)
        w, z = torch.randn((16, n), dtype=torch.float64, device="cuda"), torch.empty((16, n), dtype=torch.float64,
                                                                                      device="cuda")
        st = _lib.current_stream()

        def dense():
            Q.copy_(Q0)
            _lib.check(lib.gss_dev_potrf_inverse(_lib.ptr(Q), n, n, _lib.ptr(W), n, st))
            _lib.check(lib.gss_dev_gemm(n, 16, n, 1.0, _lib.ptr(W), 1, n, _lib.ptr(w), 1, n, 0.0, _lib.ptr(z), 1, n, 0, st))
        vout = torch.empty((16, n), dtype=torch.float64, device="cuda")
        row = dict(mesh="grid_%d" % n, nv=n, range=10.0, NB=16, dense_ms=timed(dense),
                   call_ms=timed(lambda: _lib.check(lib.gss_spde_realize(h._h, 1, 0, 16, None, 1e-10, 0, _lib.ptr(vout),
                                                                         None, _lib.MEM_DEVICE, st))),
                   iters=h.last_solve()[0])
        row["dense_over_cg"] = row["dense_ms"][0] / row["call_ms"][0]
        print(json.dumps(row), flush=True)
        h.close()


def conditional(a):
    """--conditional: gss_spde_condition and conditional realisations on grid_1e5 (range 10) and sphere_7 with 100 and
    1 000 observations at random points (barycentric rows, error variance 0.01), NB = 16.  One JSON line per case:
      locate_ms                gss_spde_locate of the observation points (brute force)
      setup_ms, w_ms, gram_ms, factor_ms   gss_spde_condition and its profile scopes "spde_cond_w" (the nd solves),
                               "spde_cond_gram" (diag(s) W and the product), "spde_cond_factor"
      uncond_ms, cond_ms, ratio   16 realisations without and with the data in the same session (floor: 2, two solves)
      combine_us, copy_us      the combine kernel of a block (profile scope "spde_combine") beside a device copy of
                               W's bytes (8 nv nd, nd rounded up to 16)
      lambda_us                the two triangular products with inv(L) of a block (profile scope "spde_lambda")
      mean_ms                  gss_spde_mean
    profiles/spde_cond_sweep.jsonl."""
    import numpy as np
    import torch

    import gss
    import spde_ref as R
    from gss import _lib
    from gss.engine import SPDEHandle

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        t = [event_ms(fn) for _ in range(a.reps)]
        return statistics.median(t), min(t), max(t)

    def scope(name):
        ms, n = _lib.profile_read(name)
        return ms / max(n, 1)

    k = 10 if a.small else 1
    g = gss.triangulate(gss.CartesianGrid(316 // k - 1, 316 // k - 1))
    cases = [("grid_1e5", (g.vertices, g.triangles), 10.0), ("sphere_7", R.icosphere(3 if a.small else 7), 0.05)]
    lines = []
    for name, (V, T), rng in cases:
        h = SPDEHandle(V, T, sill=1.0, range=rng)
        for nd in (100 // k, 1000 // k):
            gen = np.random.default_rng(nd)
            tri = gen.choice(len(T), size=nd, replace=False)
            pts = np.einsum("ik,ikd->id", gen.dirichlet(np.ones(3), size=nd), V[T[tri]])
            row = dict(mesh=name, nv=h.nv, nt=h.nt, range=rng, nd=nd, NB=16)
            row["locate_ms"] = timed(lambda: h.locate(pts))
            where, w = h.locate(pts)
            assert np.array_equal(where, tri)
            y, r = gen.normal(size=nd), np.full(nd, 0.01)
            h.condition_clear()
            row["uncond_ms"] = timed(lambda: h.realize(1, 0, 16, device=True))
            row["uncond_iters"] = h.last_solve()[0]
            _lib.profile_enable(True)
            _lib.profile_reset()
            row["setup_ms"] = timed(lambda: h.condition(T[where], w, y, r))
            row["w_ms"], row["gram_ms"], row["factor_ms"] = (scope(s) for s in ("spde_cond_w", "spde_cond_gram",
                                                                                "spde_cond_factor"))
            row["w_iters"] = h.last_solve()[0]
            _lib.profile_reset()
            row["cond_ms"] = timed(lambda: h.realize(1, 0, 16, device=True))
            row["cond_iters"] = h.last_solve()[0]
            row["combine_us"], row["lambda_us"] = 1e3 * scope("spde_combine"), 1e3 * scope("spde_lambda")
            _lib.profile_enable(False)
            row["ratio"] = row["cond_ms"][0] / row["uncond_ms"][0]
            row["mean_ms"] = timed(lambda: h.mean(device=True))
            nbytes = 8 * h.nv * ((nd + 15) // 16 * 16)
            row["w_bytes"] = nbytes
            src = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
            dst = torch.empty_like(src)
            row["copy_us"] = 1e3 * timed(lambda: [dst.copy_(src) for _ in range(10)])[0] / 10
            del src, dst
            print(json.dumps(row), flush=True)
            lines.append(json.dumps(row))
        h.close()
    if not a.small:
        with open(os.path.join(ROOT, "profiles", "spde_cond_sweep.jsonl"), "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--small", action="store_true", help="a tenth of every size (a quick check of the tool itself)")
    ap.add_argument("--conditional", action="store_true", help="the conditioning path (profiles/spde_cond_sweep.jsonl)")
    ap.add_argument("--worker", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if a.conditional:
        return conditional(a)
    lines = []
    for nb in (16, 8, 32):
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", str(nb), "--reps", str(a.reps), "--warmup",
               str(a.warmup)] + (["--small"] if a.small else [])
        r = subprocess.run(cmd, env=dict(os.environ, GSS_SPDE_NB=str(nb)), capture_output=True, text=True, timeout=360)
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:
            raise SystemExit("worker NB=%d failed with status %d" % (nb, r.returncode))
        for line in r.stdout.splitlines():
            if line.startswith("{"):
                print(line, flush=True)
                lines.append(line)
    if not a.small:
        with open(os.path.join(ROOT, "profiles", "spde_sweep.jsonl"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
